// k_window_copy: k_delta_copy's join (delta_copy.h) for WINDOW reads — any number of rows in one launch, each a 2-D sub-block of a
// decoded entry, seen as a matrix of rows x row_bytes, written densely to a destination of window size; on the way the byte planes are
// joined and, where the row has one, the BASE is XORed in.  The window, the map, the row table and what an item covers:
// window_copy_plan.h; items and launches: plane_copy_plan.h; the byte permutes (pc_group) and the 16-byte accesses (pc_ld, pc_st):
// plane_copy.h, used as they are.
//
// IN PLACE.  base == dst exactly is legal.  The base is indexed by DESTINATION byte, so item t reads base[from, to) and writes
// dst[from, to), the same range; the items tile the destination, so no item writes what another reads; inside an item a lane loads the
// base bytes of its groups before it stores to the same addresses, and lanes own disjoint groups — with U > 1 every load of a step
// stands before its first store.  So `base` and `dst` are NOT __restrict__, as in k_delta_copy.  Any other overlap the host refuses
// (window_overlap_ok).
#pragma once
#include "plane_copy.h"
#include "window_copy_plan.h"

namespace zpk {

// the geometry of a row, uniform over the wave
struct WcGeom { u64 n, row_bytes, row0, col0, cols; };

// One item of a row with element size K.  Group G of the item — 16 elements of ONE window row — is 16 * K destination bytes at
// window_dst_of, the same 16 * K bytes of the base, and 16 bytes in each plane at p * m + e, e the group's first plain element; lane l
// takes the groups l, l + 64, ... of the WHOLE item, whichever window rows they lie in, so a window of short rows keeps the wave as
// busy as one long row does.  U groups per lane and step as in k_plane_copy / k_delta_copy: U * K loads of 16 bytes in flight per lane
// without a base (4, 4, 4, 8 for K = 1, 2, 4, 8), twice that with one.
template <u32 K, bool BASE> __device__ __forceinline__ void wc_item(const u8* src, u8* dst, const u8* base, WcGeom g, WindowPiece P, int lane)
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
            d[t] = d_row0 + (u64)a.row * g.cols + a.col;
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
            const u64 d = d_row0 + (u64)a.row * g.cols + a.col;
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
        const u64 d = d_row0 + (u64)a.row * g.cols + a.col;
        const u64 i = i_row0 + (u64)a.row * g.row_bytes + a.col;
        const u8 v = ld8(src + (i % K) * m + i / K);                                   // plane_stored_index of an entry without a tail (window_valid)
        st8(dst + d, BASE ? delta_byte(v, ld8(base + d)) : v);
    }
}

// One wave per work item = (row, 16 KiB piece of its destination), four waves per workgroup, the row found as k_plane_copy finds it.
// Source, destination, base and every plane start may have any alignment.  Nothing outside [src, src + n) and [base, base + len) is
// read, nothing outside [dst, dst + len) is written; every destination byte is written once.  No LDS, no scratch.
__global__ __launch_bounds__(256) void k_window_copy(const WindowCopyRow* __restrict__ rows, u32 nrows, u64 item0, u64 nitems)
{
    const int lane = lane_id();
    const u64 w = uni64((u64)blockIdx.x * 4 + (threadIdx.x >> 6));
    if (w >= nitems) return;
    const u64 item = item0 + w;
    u32 lo = 0, hi = nrows;                                                           // last row with item_base <= item
    while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (rows[mid].item_base <= item) lo = mid; else hi = mid; }
    const WindowCopyRow r = rows[lo];
    const u64 len = uni64(r.len), piece = uni64(item - r.item_base);
    const u32 k = uni(r.elem);
    if (piece >= plane_copy_items(len)) return;                                       // (not an item of this table)
    const u8* const s = uni_ptr((const u8*)r.src);
    u8* const d = uni_ptr((u8*)r.dst);
    const u8* const b = uni_ptr((const u8*)r.base);
    const WcGeom g = { uni64(r.n), uni64(r.row_bytes), uni64(r.row0), uni64(r.col0), uni64(r.cols) };
    const WindowPiece P = window_piece(len, g.cols, k, piece);
    if (b) {
        if (k == 2) wc_item<2, true>(s, d, b, g, P, lane); else if (k == 4) wc_item<4, true>(s, d, b, g, P, lane);
        else if (k == 8) wc_item<8, true>(s, d, b, g, P, lane); else if (k == 1) wc_item<1, true>(s, d, b, g, P, lane);
    } else {
        if (k == 2) wc_item<2, false>(s, d, b, g, P, lane); else if (k == 4) wc_item<4, false>(s, d, b, g, P, lane);
        else if (k == 8) wc_item<8, false>(s, d, b, g, P, lane); else if (k == 1) wc_item<1, false>(s, d, b, g, P, lane);
    }
}

}  // namespace zpk
