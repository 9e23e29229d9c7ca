// row_copy.h — the device parts the four ROW COPIES share (the kernels themselves: row_copy.hip): how a wave finds its row and its piece
// (copy_item_of), the dispatch on a row's element size (copy_dispatch), the byte permutes (pc_group) and the 16-byte accesses (pc_ld,
// pc_st), and the two item bodies that use them — pc_item, one 16 KiB piece of a byte-plane or delta row, and wc_item, one of a window
// row or, PITCHED, of a placed row.  The tables, the items and the launches: copy_rows_plan.h and the five *_copy_plan.h.
#pragma once
#include <type_traits>
#include "zpk_device.h"
#include "place_copy_plan.h"                     // (... and window_copy_plan.h, delta_copy_plan.h, plane_copy_plan.h, copy_rows_plan.h through it)

namespace zpk {

// One wave per work item = (row, 16 KiB piece of it), four waves per workgroup; wave w of the launch has item item0 + w and finds its row
// as the last one with item_base <= item (item_base ascends: copy_rows_plan.h).  false: a wave past the launch's items.  true: `r` is
// the row, its len uniform over the wave, and `piece` the number of the item in it — an item of this table when piece < copy_items(r.len),
// which the kernel asks once it has made the row's other members uniform (the order its instructions have always had; it also reads
// r.len through uni64 once more, which costs no instruction and keeps the compiler's schedule).
template <class Row> __device__ __forceinline__ bool copy_item_of(const Row* __restrict__ rows, u32 nrows, u64 item0, u64 nitems, Row& r, u64& piece)
{
    const u64 w = uni64((u64)blockIdx.x * 4 + (threadIdx.x >> 6));
    const bool ok = w < nitems;
    if (ok) {
        const u64 item = item0 + w;
        u32 lo = 0, hi = nrows;                                                       // last row with item_base <= item
        while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (rows[mid].item_base <= item) lo = mid; else hi = mid; }
        r = rows[lo];
        r.len = uni64(r.len);
        piece = uni64(item - r.item_base);
    }
    return ok;
}

// f(K, FLAG) with the row's element size k and a flag of it as constants: std::integral_constant<u32, K> and std::bool_constant<FLAG>.
// An element size that is none (plane_elem_valid; the host refuses it) runs nothing.
template <class F> __device__ __forceinline__ void copy_dispatch(u32 k, bool flag, F f)
{
    auto by_k = [&](auto FLAG) {
        if (k == 2) f(std::integral_constant<u32, 2>{}, FLAG); else if (k == 4) f(std::integral_constant<u32, 4>{}, FLAG);
        else if (k == 8) f(std::integral_constant<u32, 8>{}, FLAG); else if (k == 1) f(std::integral_constant<u32, 1>{}, FLAG);
    };
    if (flag) by_k(std::true_type{}); else by_k(std::false_type{});
}

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

// One item of a byte-plane (BASE false; `base` unused) or delta (BASE true) row with element size K: `src` and `dst` are the row's two
// sides (both whole: the planes of an item lie apart by m), P what the item covers.  Group g of the item — 16 elements — is 16 * K plain
// bytes at from + g * 16 * K, the same 16 * K bytes of the base, and 16 bytes in each plane at p * m + from / K + g * 16; lane l takes
// the groups l, l + 64, ...: a wave step reads 1024 * K contiguous bytes of the plain side's source (and of the base) and writes K runs
// of 1 KiB (SPLIT; JOIN the other way round), U steps at once so that at least four 16-byte loads are in flight as in k_span_copy:
// U * K per lane without a base (4, 4, 4, 8 for K = 1, 2, 4, 8), twice that with one.
//
// IN PLACE.  On a join base == dst exactly is legal.  Item t reads base[from, to) and writes dst[from, to), the same plain range; the
// items tile the plain side, so no item writes what another reads; inside an item a lane loads the base bytes of its groups before it
// stores to the same addresses, and lanes own disjoint groups — with U > 1 every load of a step stands before its first store.  So
// `base` and `dst` are NOT __restrict__ (the compiler must take them for aliases and keep that order), and the base loads of a step are
// not hoisted over the stores of the step before.  Any other overlap of base and dst the host refuses (delta_overlap_ok).
template <u32 K, bool JOIN, bool BASE> __device__ __forceinline__ void pc_item(const u8* src, u8* dst, const u8* base, u64 n, PlanePiece P, int lane)
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
                if constexpr (BASE) b[t][p] = pc_ld(b_pl + ((u64)(g + t * WAVE) * K + p) * 16u);
            }
        #pragma unroll
        for (u32 t = 0; t < U; t++) {
            if constexpr (BASE && !JOIN) {
                #pragma unroll
                for (u32 p = 0; p < K; p++) x[t][p] ^= b[t][p];
            }
            pc_group<K, JOIN>(x[t], y[t]);
            if constexpr (BASE && JOIN) {
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
                if constexpr (BASE) b[p] = pc_ld(b_pl + ((u64)g * K + p) * 16u);
            }
            if constexpr (BASE && !JOIN) {
                #pragma unroll
                for (u32 p = 0; p < K; p++) x[p] ^= b[p];
            }
            pc_group<K, JOIN>(x, y);
            if constexpr (BASE && JOIN) {
                #pragma unroll
                for (u32 p = 0; p < K; p++) y[p] ^= b[p];
            }
            #pragma unroll
            for (u32 p = 0; p < K; p++) { if (JOIN) pc_st(d_pl + ((u64)g * K + p) * 16u, y[p]); else pc_st(d_pl + p * m + (u64)g * 16u, y[p]); }
        }
    // the elements behind the last whole group and the tail: fewer than 16 * K + K bytes, byte by byte through the index map, XORed alike
    for (u64 i = P.wide_end + (u32)lane; i < P.to; i += WAVE) {
        const u64 j = plane_stored_index(n, K, i);
        if constexpr (BASE) {
            const u8 bb = ld8(base + i);
            if (JOIN) st8(dst + i, delta_byte(ld8(src + j), bb)); else st8(dst + j, delta_byte(ld8(src + i), bb));
        } else {
            if (JOIN) st8(dst + i, ld8(src + j)); else st8(dst + j, ld8(src + i));
        }
    }
}

// the geometry of a window row, uniform over the wave; pitch: a placed row's (place_copy_plan.h), not looked at otherwise
struct WcGeom { u64 n, row_bytes, row0, col0, cols, pitch; };

// One item of a window row with element size K.  Group G of the item — 16 elements of ONE window row — is 16 * K destination bytes at
// window_dst_of, the same 16 * K bytes of the base, and 16 bytes in each plane at p * m + e, e the group's first plain element; lane l
// takes the groups l, l + 64, ... of the WHOLE item, whichever window rows they lie in, so a window of short rows keeps the wave as
// busy as one long row does.  U groups per lane and step as in pc_item: U * K loads of 16 bytes in flight per lane without a base
// (4, 4, 4, 8 for K = 1, 2, 4, 8), twice that with one.
//
// IN PLACE.  base == dst exactly is legal.  The base is indexed by DESTINATION byte, so item t reads base[from, to) and writes
// dst[from, to), the same range; the items tile the destination, so no item writes what another reads; inside an item a lane loads the
// base bytes of its groups before it stores to the same addresses, and lanes own disjoint groups — with U > 1 every load of a step
// stands before its first store.  So `base` and `dst` are NOT __restrict__, as in pc_item.  Any other overlap the host refuses
// (window_overlap_ok).
//
// PITCHED: one item of a PLACED row (k_place_copy).  The item is the same 16 KiB of window bytes, the same groups and loose bytes and the
// same plain indices; only where a place lies in `dst` and `base` differs — place_dst_of, window row r at r * pitch — so the rows of an
// item lie apart and the gaps between them are neither written nor read.  The in-place argument holds over the placed bytes
// (place_copy_plan.h); any other overlap of the two extents the host refuses (place_overlap_ok).  Without PITCHED g.pitch is not looked
// at and the instructions are those the item had before there was one.
template <u32 K, bool BASE, bool PITCHED = false> __device__ __forceinline__ void wc_item(const u8* src, u8* dst, const u8* base, WcGeom g, WindowPiece P, int lane)
{
    constexpr u32 U = K == 1 ? 4 : K == 2 ? 2 : 1;
    const u64 m = g.n / K;
    const u64 d_row0 = P.r0 * g.cols;                                                  // destination byte of (window row r0, column 0)
    const u64 i_row0 = (g.row0 + P.r0) * g.row_bytes + g.col0;                         // ... and its plain index
    u32 G = (u32)lane;
    for (; G + (U - 1) * WAVE < P.groups; G += U * WAVE) {
        v4u32 x[U][K], b[U][K], y[U][K];
        u64 d[U];
        #pragma unroll
        for (u32 t = 0; t < U; t++) {
            const WindowAt a = window_group_at(P, K, G + t * WAVE);
            d[t] = PITCHED ? place_dst_of(P, g.pitch, a) : d_row0 + (u64)a.row * g.cols + a.col;
            const u64 e = (i_row0 + (u64)a.row * g.row_bytes + a.col) / K;
            #pragma unroll
            for (u32 p = 0; p < K; p++) {
                x[t][p] = pc_ld(src + p * m + e);
                if constexpr (BASE) b[t][p] = pc_ld(base + d[t] + p * 16u);
            }
        }
        #pragma unroll
        for (u32 t = 0; t < U; t++) {
            pc_group<K, true>(x[t], y[t]);
            if constexpr (BASE) {
                #pragma unroll
                for (u32 p = 0; p < K; p++) y[t][p] ^= b[t][p];
            }
        }
        #pragma unroll
        for (u32 t = 0; t < U; t++)
            #pragma unroll
            for (u32 p = 0; p < K; p++) pc_st(dst + d[t] + p * 16u, y[t][p]);
    }
    if constexpr (U > 1)
        for (; G < P.groups; G += WAVE) {
            v4u32 x[K], b[K], y[K];
            const WindowAt a = window_group_at(P, K, G);
            const u64 d = PITCHED ? place_dst_of(P, g.pitch, a) : d_row0 + (u64)a.row * g.cols + a.col;
            const u64 e = (i_row0 + (u64)a.row * g.row_bytes + a.col) / K;
            #pragma unroll
            for (u32 p = 0; p < K; p++) {
                x[p] = pc_ld(src + p * m + e);
                if constexpr (BASE) b[p] = pc_ld(base + d + p * 16u);
            }
            pc_group<K, true>(x, y);
            if constexpr (BASE) {
                #pragma unroll
                for (u32 p = 0; p < K; p++) y[p] ^= b[p];
            }
            #pragma unroll
            for (u32 p = 0; p < K; p++) pc_st(dst + d + p * 16u, y[p]);
        }
    // what does not fill a group at the end of a window-row segment: byte by byte through the map, dealt over the whole item likewise
    for (u32 B = (u32)lane; B < P.loose; B += WAVE) {
        const WindowAt a = window_loose_at(P, K, B);
        const u64 d = PITCHED ? place_dst_of(P, g.pitch, a) : d_row0 + (u64)a.row * g.cols + a.col;
        const u64 i = i_row0 + (u64)a.row * g.row_bytes + a.col;
        const u8 v = ld8(src + (i % K) * m + i / K);                                   // plane_stored_index of an entry without a tail (window_valid)
        st8(dst + d, BASE ? delta_byte(v, ld8(base + d)) : v);
    }
}

}  // namespace zpk
