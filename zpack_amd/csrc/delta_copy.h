// k_delta_copy: k_plane_copy (plane_copy.h) for DELTA entries — any number of rows in one launch, each from one device address to
// another, and on the way the bytes are XORed with the row's BASE and grouped into byte planes (SPLIT: stored = split_k(plain ^ base),
// the caller's tensor into the codec's staging) or put back (JOIN: plain = join_k(stored) ^ base, a decoded slot to the caller's
// tensor).  The layout and the row table: delta_copy_plan.h; items, pieces and launches: plane_copy_plan.h; the byte permutes
// (pc_group) and the 16-byte accesses (pc_ld, pc_st): plane_copy.h, used as they are.
//
// IN PLACE.  On a join base == dst exactly is legal.  Item t reads base[from, to) and writes dst[from, to), the same plain range; the
// items tile the plain side, so no item writes what another reads; inside an item a lane loads the base bytes of its groups before it
// stores to the same addresses, and lanes own disjoint groups — with U > 1 every load of a step stands before its first store.  So
// `base` and `dst` are NOT __restrict__ (the compiler must take them for aliases and keep that order), and the base loads of a step are
// not hoisted over the stores of the step before.  Any other overlap of base and dst the host refuses (delta_overlap_ok).
#pragma once
#include "plane_copy.h"
#include "delta_copy_plan.h"

namespace zpk {

// One item of a row with element size K.  Group g of the item — 16 elements — is 16 * K plain bytes at from + g * 16 * K, the same
// 16 * K bytes of the base, and 16 bytes in each plane at p * m + from / K + g * 16; lane l takes the groups l, l + 64, ...  A wave step
// reads 1024 * K contiguous bytes of the plain side's source AND of the base: 2 * U * K loads of 16 bytes in flight per lane where
// k_plane_copy has U * K (8, 8, 8, 16 against 4, 4, 4, 8 for K = 1, 2, 4, 8).
template <u32 K, bool JOIN> __device__ __forceinline__ void dc_item(const u8* src, u8* dst, const u8* base, u64 n, PlanePiece P, int lane)
{
    constexpr u32 U = K == 1 ? 4 : K == 2 ? 2 : 1;
    const u64 m = n / K;
    const u8* const s_pl = src + (JOIN ? P.from / K : P.from);                         // this item's first byte on the source's side (plane 0 of a join)
    u8* const d_pl = dst + (JOIN ? P.from : P.from / K);
    const u8* const b_pl = base + P.from;                                              // the base lies beside the plain side
    const u32 groups = (u32)((P.wide_end - P.from) / (16u * K));
    u32 g = (u32)lane;
    for (; g + (U - 1) * WAVE < groups; g += U * WAVE) {
        v4u32 x[U][K], b[U][K], y[U][K];
        #pragma unroll
        for (u32 t = 0; t < U; t++)
            #pragma unroll
            for (u32 p = 0; p < K; p++) {
                x[t][p] = JOIN ? pc_ld(s_pl + p * m + (u64)(g + t * WAVE) * 16u) : pc_ld(s_pl + ((u64)(g + t * WAVE) * K + p) * 16u);
                b[t][p] = pc_ld(b_pl + ((u64)(g + t * WAVE) * K + p) * 16u);
            }
        #pragma unroll
        for (u32 t = 0; t < U; t++) {
            if constexpr (!JOIN) {
                #pragma unroll
                for (u32 p = 0; p < K; p++) x[t][p] ^= b[t][p];
            }
            pc_group<K, JOIN>(x[t], y[t]);
            if constexpr (JOIN) {
                #pragma unroll
                for (u32 p = 0; p < K; p++) y[t][p] ^= b[t][p];
            }
        }
        #pragma unroll
        for (u32 t = 0; t < U; t++)
            #pragma unroll
            for (u32 p = 0; p < K; p++) { if (JOIN) pc_st(d_pl + ((u64)(g + t * WAVE) * K + p) * 16u, y[t][p]); else pc_st(d_pl + p * m + (u64)(g + t * WAVE) * 16u, y[t][p]); }
    }
    if constexpr (U > 1)
        for (; g < groups; g += WAVE) {
            v4u32 x[K], b[K], y[K];
            #pragma unroll
            for (u32 p = 0; p < K; p++) {
                x[p] = JOIN ? pc_ld(s_pl + p * m + (u64)g * 16u) : pc_ld(s_pl + ((u64)g * K + p) * 16u);
                b[p] = pc_ld(b_pl + ((u64)g * K + p) * 16u);
            }
            if constexpr (!JOIN) {
                #pragma unroll
                for (u32 p = 0; p < K; p++) x[p] ^= b[p];
            }
            pc_group<K, JOIN>(x, y);
            if constexpr (JOIN) {
                #pragma unroll
                for (u32 p = 0; p < K; p++) y[p] ^= b[p];
            }
            #pragma unroll
            for (u32 p = 0; p < K; p++) { if (JOIN) pc_st(d_pl + ((u64)g * K + p) * 16u, y[p]); else pc_st(d_pl + p * m + (u64)g * 16u, y[p]); }
        }
    // the elements behind the last whole group and the tail: fewer than 16 * K + K bytes, byte by byte through the index map, XORed alike
    for (u64 i = P.wide_end + (u32)lane; i < P.to; i += WAVE) {
        const u64 j = plane_stored_index(n, K, i);
        const u8 bb = ld8(base + i);
        if (JOIN) st8(dst + i, delta_byte(ld8(src + j), bb)); else st8(dst + j, delta_byte(ld8(src + i), bb));
    }
}

// One wave per work item = (row, 16 KiB piece of its plain side), four waves per workgroup, the row found as k_plane_copy finds it.
// Source, destination, base and every plane start may have any alignment.  Nothing outside [src, src + len) and [base, base + len) is
// read, nothing outside [dst, dst + len) is written; every byte of the three is touched once.  No LDS, no scratch.
__global__ __launch_bounds__(256) void k_delta_copy(const DeltaCopyRow* __restrict__ rows, u32 nrows, u64 item0, u64 nitems)
{
    const int lane = lane_id();
    const u64 w = uni64((u64)blockIdx.x * 4 + (threadIdx.x >> 6));
    if (w >= nitems) return;
    const u64 item = item0 + w;
    u32 lo = 0, hi = nrows;                                                           // last row with item_base <= item
    while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (rows[mid].item_base <= item) lo = mid; else hi = mid; }
    const DeltaCopyRow r = rows[lo];
    const u64 n = uni64(r.len), piece = uni64(item - r.item_base);
    const u32 k = uni(r.elem), join = uni(r.join);
    if (piece >= plane_copy_items(n)) return;                                         // (not an item of this table)
    const u8* const s = uni_ptr((const u8*)r.src);
    u8* const d = uni_ptr((u8*)r.dst);
    const u8* const b = uni_ptr((const u8*)r.base);
    const PlanePiece P = plane_piece(n, k, piece);
    if (join) {
        if (k == 2) dc_item<2, true>(s, d, b, n, P, lane); else if (k == 4) dc_item<4, true>(s, d, b, n, P, lane);
        else if (k == 8) dc_item<8, true>(s, d, b, n, P, lane); else if (k == 1) dc_item<1, true>(s, d, b, n, P, lane);
    } else {
        if (k == 2) dc_item<2, false>(s, d, b, n, P, lane); else if (k == 4) dc_item<4, false>(s, d, b, n, P, lane);
        else if (k == 8) dc_item<8, false>(s, d, b, n, P, lane); else if (k == 1) dc_item<1, false>(s, d, b, n, P, lane);
    }
}

}  // namespace zpk
