// k_plane_copy: k_span_copy (span_copy.h) for BYTE-PLANE entries — any number of rows in one launch, each from one device address to
// another, and on the way the bytes of its k-byte elements are grouped into k planes (SPLIT: the caller's tensor into the codec's
// staging, which the encoders then read) or put back (JOIN: a decoded slot to the caller's tensor).  The layout, the row table, the work
// items and the launches: plane_copy_plan.h.
#pragma once
#include "zpk_device.h"
#include "plane_copy_plan.h"

namespace zpk {

__device__ __forceinline__ v4u32 pc_ld(const u8* p) { return *(const ZPK_GLOBAL v4u32_u*)p; }
__device__ __forceinline__ void pc_st(u8* p, v4u32 v) { *(ZPK_GLOBAL v4u32_u*)p = v; }
// bytes 0..3 of `sel` say which byte of lo (0..3) or hi (4..7) each byte of the result is: one v_perm_b32
__device__ __forceinline__ u32 pc_perm(u32 hi, u32 lo, u32 sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
// the 4 x 4 byte matrix whose rows are a, b, c, d, transposed: r[p] holds byte p of a, b, c, d in that order.  Its own inverse.
struct PcT4 { u32 r[4]; };
__device__ __forceinline__ PcT4 pc_t4(u32 a, u32 b, u32 c, u32 d)
{
    const u32 ab01 = pc_perm(b, a, 0x05010400u), cd01 = pc_perm(d, c, 0x05010400u);  // a0 b0 a1 b1, c0 d0 c1 d1
    const u32 ab23 = pc_perm(b, a, 0x07030602u), cd23 = pc_perm(d, c, 0x07030602u);  // a2 b2 a3 b3, c2 d2 c3 d3
    return PcT4{ { pc_perm(cd01, ab01, 0x05040100u), pc_perm(cd01, ab01, 0x07060302u), pc_perm(cd23, ab23, 0x05040100u), pc_perm(cd23, ab23, 0x07060302u) } };
}
// 16 elements of K bytes: x[0, K) are the K consecutive 16-byte words of the plain side, y[p] is the 16-byte word of plane p.
// SPLIT makes y of x, JOIN x of y.  All indices are constants once unrolled: registers only.
template <u32 K, bool JOIN> __device__ __forceinline__ void pc_group(const v4u32 (&in)[K], v4u32 (&out)[K])
{
    if constexpr (K == 1) { out[0] = in[0]; }
    else if constexpr (K == 2) {
        #pragma unroll
        for (u32 q = 0; q < 4; q++) {
            if constexpr (!JOIN) {                                                     // words 2q, 2q + 1 hold the elements 4q .. 4q + 3
                const u32 lo = in[q >> 1][(q & 1) * 2], hi = in[q >> 1][(q & 1) * 2 + 1];
                out[0][q] = pc_perm(hi, lo, 0x06040200u); out[1][q] = pc_perm(hi, lo, 0x07050301u);
            } else {
                out[q >> 1][(q & 1) * 2] = pc_perm(in[1][q], in[0][q], 0x05010400u);
                out[q >> 1][(q & 1) * 2 + 1] = pc_perm(in[1][q], in[0][q], 0x07030602u);
            }
        }
    } else if constexpr (K == 4) {
        #pragma unroll
        for (u32 q = 0; q < 4; q++) {                                                  // word q of the plain side's 16-byte word j is element 4j + q
            if constexpr (!JOIN) { const PcT4 t = pc_t4(in[q][0], in[q][1], in[q][2], in[q][3]); out[0][q] = t.r[0]; out[1][q] = t.r[1]; out[2][q] = t.r[2]; out[3][q] = t.r[3]; }
            else                 { const PcT4 t = pc_t4(in[0][q], in[1][q], in[2][q], in[3][q]); out[q][0] = t.r[0]; out[q][1] = t.r[1]; out[q][2] = t.r[2]; out[q][3] = t.r[3]; }
        }
    } else {
        static_assert(K == 8, "element sizes: plane_elem_valid");
        #pragma unroll
        for (u32 q = 0; q < 4; q++) {                                                  // the elements 4q .. 4q + 3 are the words 2q, 2q + 1: low halves x, z, high halves y, w
            #pragma unroll
            for (u32 h = 0; h < 2; h++) {
                if constexpr (!JOIN) {
                    const PcT4 t = pc_t4(in[2 * q][h], in[2 * q][2 + h], in[2 * q + 1][h], in[2 * q + 1][2 + h]);
                    out[4 * h][q] = t.r[0]; out[4 * h + 1][q] = t.r[1]; out[4 * h + 2][q] = t.r[2]; out[4 * h + 3][q] = t.r[3];
                } else {
                    const PcT4 t = pc_t4(in[4 * h][q], in[4 * h + 1][q], in[4 * h + 2][q], in[4 * h + 3][q]);
                    out[2 * q][h] = t.r[0]; out[2 * q][2 + h] = t.r[1]; out[2 * q + 1][h] = t.r[2]; out[2 * q + 1][2 + h] = t.r[3];
                }
            }
        }
    }
}

// One item of a row with element size K: `plain` and `planes` are the row's two sides (both whole: the planes of an item lie apart by m),
// P what the item covers.  Group g of the item — 16 elements — is 16 * K plain bytes at from + g * 16 * K and 16 bytes in each plane at
// p * m + from / K + g * 16; lane l takes the groups l, l + 64, ...: a wave step reads 1024 * K contiguous bytes and writes K runs of
// 1 KiB (SPLIT; JOIN the other way round), U steps at once so that at least four 16-byte loads are in flight as in k_span_copy.
template <u32 K, bool JOIN> __device__ __forceinline__ void pc_item(const u8* src, u8* dst, u64 n, PlanePiece P, int lane)
{
    constexpr u32 U = K == 1 ? 4 : K == 2 ? 2 : 1;
    const u64 m = n / K;
    const u8* const s_pl = src + (JOIN ? P.from / K : P.from);                         // this item's first byte on the source's side (plane 0 of a join)
    u8* const d_pl = dst + (JOIN ? P.from : P.from / K);
    const u32 groups = (u32)((P.wide_end - P.from) / (16u * K));
    u32 g = (u32)lane;
    for (; g + (U - 1) * WAVE < groups; g += U * WAVE) {
        v4u32 x[U][K], y[U][K];
        #pragma unroll
        for (u32 t = 0; t < U; t++)
            #pragma unroll
            for (u32 p = 0; p < K; p++) x[t][p] = JOIN ? pc_ld(s_pl + p * m + (u64)(g + t * WAVE) * 16u) : pc_ld(s_pl + ((u64)(g + t * WAVE) * K + p) * 16u);
        #pragma unroll
        for (u32 t = 0; t < U; t++) pc_group<K, JOIN>(x[t], y[t]);
        #pragma unroll
        for (u32 t = 0; t < U; t++)
            #pragma unroll
            for (u32 p = 0; p < K; p++) { if (JOIN) pc_st(d_pl + ((u64)(g + t * WAVE) * K + p) * 16u, y[t][p]); else pc_st(d_pl + p * m + (u64)(g + t * WAVE) * 16u, y[t][p]); }
    }
    if constexpr (U > 1)
        for (; g < groups; g += WAVE) {
            v4u32 x[K], y[K];
            #pragma unroll
            for (u32 p = 0; p < K; p++) x[p] = JOIN ? pc_ld(s_pl + p * m + (u64)g * 16u) : pc_ld(s_pl + ((u64)g * K + p) * 16u);
            pc_group<K, JOIN>(x, y);
            #pragma unroll
            for (u32 p = 0; p < K; p++) { if (JOIN) pc_st(d_pl + ((u64)g * K + p) * 16u, y[p]); else pc_st(d_pl + p * m + (u64)g * 16u, y[p]); }
        }
    // the elements behind the last whole group and the tail: fewer than 16 * K + K bytes, byte by byte through the index map
    for (u64 i = P.wide_end + (u32)lane; i < P.to; i += WAVE) {
        const u64 j = plane_stored_index(n, K, i);
        if (JOIN) st8(dst + i, ld8(src + j)); else st8(dst + j, ld8(src + i));
    }
}

// One wave per work item = (row, 16 KiB piece of its plain side), four waves per workgroup; wave w of the launch has item item0 + w and
// finds its row as the last one with item_base <= item (item_base ascends: plane_copy_plan.h).  Source, destination and every plane
// start may have any alignment.  Every byte is read once and written once; nothing outside [src, src + len) is read, nothing outside
// [dst, dst + len) is written.  No LDS, no scratch.
__global__ __launch_bounds__(256) void k_plane_copy(const PlaneCopyRow* __restrict__ rows, u32 nrows, u64 item0, u64 nitems)
{
    const int lane = lane_id();
    const u64 w = uni64((u64)blockIdx.x * 4 + (threadIdx.x >> 6));
    if (w >= nitems) return;
    const u64 item = item0 + w;
    u32 lo = 0, hi = nrows;                                                           // last row with item_base <= item
    while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (rows[mid].item_base <= item) lo = mid; else hi = mid; }
    const PlaneCopyRow r = rows[lo];
    const u64 n = uni64(r.len), piece = uni64(item - r.item_base);
    const u32 k = uni(r.elem), join = uni(r.join);
    if (piece >= plane_copy_items(n)) return;                                         // (not an item of this table)
    const u8* const s = uni_ptr((const u8*)r.src);
    u8* const d = uni_ptr((u8*)r.dst);
    const PlanePiece P = plane_piece(n, k, piece);
    if (join) {
        if (k == 2) pc_item<2, true>(s, d, n, P, lane); else if (k == 4) pc_item<4, true>(s, d, n, P, lane);
        else if (k == 8) pc_item<8, true>(s, d, n, P, lane); else if (k == 1) pc_item<1, true>(s, d, n, P, lane);
    } else {
        if (k == 2) pc_item<2, false>(s, d, n, P, lane); else if (k == 4) pc_item<4, false>(s, d, n, P, lane);
        else if (k == 8) pc_item<8, false>(s, d, n, P, lane); else if (k == 1) pc_item<1, false>(s, d, n, P, lane);
    }
}

}  // namespace zpk
