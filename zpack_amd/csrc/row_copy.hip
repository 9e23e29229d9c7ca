// row_copy.hip — the five ROW COPIES that move plaintext between the codec's staging and the caller's device buffers, as one code object:
// k_span_copy (plain bytes), k_plane_copy (byte planes), k_delta_copy (byte planes XORed against a base), k_window_copy (a 2-D cut of
// a decoded entry) and k_place_copy (that cut set into a sub-block of a larger tensor), each with the one host function that launches it.  zpk_codec.hip builds the row tables and calls the launchers;
// keeping the kernels out of that file keeps its code object, and where every other kernel lies in it, unchanged.  What the kernels
// share: row_copy.h; the tables, the items and the launches: copy_rows_plan.h and the five *_copy_plan.h.
#include <hip/hip_runtime.h>
#include "row_copy.h"
#include "seq_exec.h"                            // gcopy_upto16
#include "span_copy_plan.h"

namespace zpk {

// k_span_copy: any number of byte spans, each from one device address to another, in one launch — what moves a sub-batch's plaintext
// between the codec's staging slots and the caller's per-entry DEVICE buffers (zpk_codec_decode_batch_host_dptr,
// zpk_codec_encode_batch_dsrc), where the host-pointer paths scatter and gather on the host.  One hipMemcpyAsync per entry would be
// 100 000 calls for a bench-sized batch.
// One wave per work item (copy_item_of).  Source and destination may have any alignment, independent of each other: 16 bytes per lane at
// any address, four loads in flight (the body of k_big_gather), the rest of the piece through gcopy_upto16, whose accesses are as wide
// as what is left.  Every byte is read once and written once; nothing outside [src, src + len) is read, nothing outside
// [dst, dst + len) is written.  No LDS.
__global__ __launch_bounds__(256) void k_span_copy(const SpanCopyRow* __restrict__ rows, u32 nrows, u64 item0, u64 nitems)
{
    const int lane = lane_id();
    SpanCopyRow r;
    u64 piece;
    if (!copy_item_of(rows, nrows, item0, nitems, r, piece)) return;
    const u64 span = uni64(r.len), from = uni64(piece * ZPK_COPY_PIECE);
    if (from >= span) return;                                                         // (not an item of this table)
    const u32 len = (u32)(span - from < ZPK_COPY_PIECE ? span - from : ZPK_COPY_PIECE);
    const u8* const s = uni_ptr((const u8*)r.src + from);
    u8* const d = uni_ptr((u8*)r.dst + from);
    u32 i = (u32)lane * 16u;
    for (; i + 3u * WAVE * 16u + 16u <= len; i += 4u * WAVE * 16u) {
        u128 v[4];
        #pragma unroll
        for (u32 t = 0; t < 4; t++) v[t] = ld128(s + i + t * WAVE * 16u);
        #pragma unroll
        for (u32 t = 0; t < 4; t++) st128(d + i + t * WAVE * 16u, v[t]);
    }
    for (; i < len; i += WAVE * 16u) gcopy_upto16(d + i, s + i, len - i < 16u ? len - i : 16u);
}

// k_plane_copy: k_span_copy for BYTE-PLANE entries — on the way the bytes of a row's k-byte elements are grouped into k planes (SPLIT:
// the caller's tensor into the codec's staging, which the encoders then read) or put back (JOIN: a decoded slot to the caller's tensor).
// The layout: plane_copy_plan.h.  Source, destination and every plane start may have any alignment.  Every byte is read once and
// written once; nothing outside [src, src + len) is read, nothing outside [dst, dst + len) is written.  No LDS, no scratch.
__global__ __launch_bounds__(256) void k_plane_copy(const PlaneCopyRow* __restrict__ rows, u32 nrows, u64 item0, u64 nitems)
{
    const int lane = lane_id();
    PlaneCopyRow r;
    u64 piece;
    if (!copy_item_of(rows, nrows, item0, nitems, r, piece)) return;
    const u64 n = uni64(r.len);
    const u32 k = uni(r.elem), join = uni(r.join);
    if (piece >= copy_items(n)) return;                                               // (not an item of this table)
    const u8* const s = uni_ptr((const u8*)r.src);
    u8* const d = uni_ptr((u8*)r.dst);
    const PlanePiece P = plane_piece(n, k, piece);
    copy_dispatch(k, join, [&](auto K, auto JOIN) { pc_item<decltype(K)::value, decltype(JOIN)::value, false>(s, d, nullptr, n, P, lane); });
}

// k_delta_copy: k_plane_copy for DELTA entries — on the way the bytes are XORed with the row's BASE and grouped into byte planes (SPLIT:
// stored = split_k(plain ^ base)) or put back (JOIN: plain = join_k(stored) ^ base).  The layout: delta_copy_plan.h.  IN PLACE: pc_item.
// Source, destination, base and every plane start may have any alignment.  Nothing outside [src, src + len) and [base, base + len) is
// read, nothing outside [dst, dst + len) is written; every byte of the three is touched once.  No LDS, no scratch.
__global__ __launch_bounds__(256) void k_delta_copy(const DeltaCopyRow* __restrict__ rows, u32 nrows, u64 item0, u64 nitems)
{
    const int lane = lane_id();
    DeltaCopyRow r;
    u64 piece;
    if (!copy_item_of(rows, nrows, item0, nitems, r, piece)) return;
    const u64 n = uni64(r.len);
    const u32 k = uni(r.elem), join = uni(r.join);
    if (piece >= copy_items(n)) return;                                               // (not an item of this table)
    const u8* const s = uni_ptr((const u8*)r.src);
    u8* const d = uni_ptr((u8*)r.dst);
    const u8* const b = uni_ptr((const u8*)r.base);
    const PlanePiece P = plane_piece(n, k, piece);
    copy_dispatch(k, join, [&](auto K, auto JOIN) { pc_item<decltype(K)::value, decltype(JOIN)::value, true>(s, d, b, n, P, lane); });
}

// k_window_copy: k_delta_copy's join for WINDOW reads — each row a 2-D sub-block of a decoded entry, seen as a matrix of rows x row_bytes,
// written densely to a destination of window size; on the way the byte planes are joined and, where the row has one, the BASE is XORed
// in.  The window, the map and what an item covers: window_copy_plan.h; an item is 16 KiB of the row's DESTINATION.  IN PLACE: wc_item.
// Source, destination, base and every plane start may have any alignment.  Nothing outside [src, src + n) and [base, base + len) is
// read, nothing outside [dst, dst + len) is written; every destination byte is written once.  No LDS, no scratch.
__global__ __launch_bounds__(256) void k_window_copy(const WindowCopyRow* __restrict__ rows, u32 nrows, u64 item0, u64 nitems)
{
    const int lane = lane_id();
    WindowCopyRow r;
    u64 piece;
    if (!copy_item_of(rows, nrows, item0, nitems, r, piece)) return;
    const u64 len = uni64(r.len);
    const u32 k = uni(r.elem);
    if (piece >= copy_items(len)) return;                                             // (not an item of this table)
    const u8* const s = uni_ptr((const u8*)r.src);
    u8* const d = uni_ptr((u8*)r.dst);
    const u8* const b = uni_ptr((const u8*)r.base);
    const WcGeom g = { uni64(r.n), uni64(r.row_bytes), uni64(r.row0), uni64(r.col0), uni64(r.cols), 0 };
    const WindowPiece P = window_piece(len, g.cols, k, piece);
    copy_dispatch(k, b != nullptr, [&](auto K, auto BASE) { wc_item<decltype(K)::value, decltype(BASE)::value>(s, d, b, g, P, lane); });
}

// k_place_copy: k_window_copy for PLACED reads — the window of each row is written into a sub-block of a larger tensor, window row r at
// r * pitch of the destination, so that several entries land side by side in one buffer; the base, where the row has one, is the
// caller's previous checkpoint in that merged layout and is read at the very bytes that are written.  The pitch, the rule, the map and
// the placed offset: place_copy_plan.h; an item is 16 KiB of the row's WINDOW bytes, cut as k_window_copy's are.  IN PLACE: wc_item.
// Source, destination, base, pitch and every plane start may have any alignment.  Nothing outside [src, src + n) is read; of
// [dst, dst + place_extent) and [base, base + place_extent) only the placed bytes are touched, each destination byte written once — the
// gaps [cols, pitch) of every row belong to the neighbours.  No LDS, no scratch.
__global__ __launch_bounds__(256) void k_place_copy(const PlaceCopyRow* __restrict__ rows, u32 nrows, u64 item0, u64 nitems)
{
    const int lane = lane_id();
    PlaceCopyRow r;
    u64 piece;
    if (!copy_item_of(rows, nrows, item0, nitems, r, piece)) return;
    const u64 len = uni64(r.len);
    const u32 k = uni(r.elem);
    if (piece >= copy_items(len)) return;                                             // (not an item of this table)
    const u8* const s = uni_ptr((const u8*)r.src);
    u8* const d = uni_ptr((u8*)r.dst);
    const u8* const b = uni_ptr((const u8*)r.base);
    const WcGeom g = { uni64(r.n), uni64(r.row_bytes), uni64(r.row0), uni64(r.col0), uni64(r.cols), uni64(r.pitch) };
    const WindowPiece P = window_piece(len, g.cols, k, piece);
    copy_dispatch(k, b != nullptr, [&](auto K, auto BASE) { wc_item<decltype(K)::value, decltype(BASE)::value, true>(s, d, b, g, P, lane); });
}

void span_copy_launch(const SpanCopyRow* d_rows, u32 nrows, u64 item0, u64 nitems, u32 grid, hipStream_t st)
{
    hipLaunchKernelGGL(k_span_copy, dim3(grid), dim3(256), 0, st, d_rows, nrows, item0, nitems);
}
void plane_copy_launch(const PlaneCopyRow* d_rows, u32 nrows, u64 item0, u64 nitems, u32 grid, hipStream_t st)
{
    hipLaunchKernelGGL(k_plane_copy, dim3(grid), dim3(256), 0, st, d_rows, nrows, item0, nitems);
}
void delta_copy_launch(const DeltaCopyRow* d_rows, u32 nrows, u64 item0, u64 nitems, u32 grid, hipStream_t st)
{
    hipLaunchKernelGGL(k_delta_copy, dim3(grid), dim3(256), 0, st, d_rows, nrows, item0, nitems);
}
void window_copy_launch(const WindowCopyRow* d_rows, u32 nrows, u64 item0, u64 nitems, u32 grid, hipStream_t st)
{
    hipLaunchKernelGGL(k_window_copy, dim3(grid), dim3(256), 0, st, d_rows, nrows, item0, nitems);
}

void place_copy_launch(const PlaceCopyRow* d_rows, u32 nrows, u64 item0, u64 nitems, u32 grid, hipStream_t st)
{
    hipLaunchKernelGGL(k_place_copy, dim3(grid), dim3(256), 0, st, d_rows, nrows, item0, nitems);
}

}  // namespace zpk
