// k_span_copy: any number of byte spans, each from one device address to another, in one launch — what moves a sub-batch's plaintext
// between the codec's staging slots and the caller's per-entry DEVICE buffers (zpk_codec_decode_batch_host_dptr,
// zpk_codec_encode_batch_dsrc), where the host-pointer paths scatter and gather on the host.  One hipMemcpyAsync per entry would be
// 100 000 calls for a bench-sized batch.  The row table, the work items and the launches: span_copy_plan.h.
#pragma once
#include "zpk_device.h"
#include "seq_exec.h"                            // gcopy_upto16
#include "span_copy_plan.h"

namespace zpk {

// One wave per work item = (row, 16 KiB piece of its span), four waves per workgroup; wave w of the launch has item item0 + w and finds
// its row as the last one with item_base <= item (item_base ascends: span_copy_plan.h).  Source and destination may have any alignment,
// independent of each other: 16 bytes per lane at any address, four loads in flight (the body of k_big_gather), the rest of the piece
// through gcopy_upto16, whose accesses are as wide as what is left.  Every byte is read once and written once; nothing outside
// [src, src + len) is read, nothing outside [dst, dst + len) is written.  No LDS.
__global__ __launch_bounds__(256) void k_span_copy(const SpanCopyRow* __restrict__ rows, u32 nrows, u64 item0, u64 nitems)
{
    const int lane = lane_id();
    const u64 w = uni64((u64)blockIdx.x * 4 + (threadIdx.x >> 6));
    if (w >= nitems) return;
    const u64 item = item0 + w;
    u32 lo = 0, hi = nrows;                                                           // last row with item_base <= item
    while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (rows[mid].item_base <= item) lo = mid; else hi = mid; }
    const SpanCopyRow r = rows[lo];
    const u64 span = uni64(r.len), from = uni64((item - r.item_base) * ZPK_SC_PIECE);
    if (from >= span) return;                                                         // (not an item of this table)
    const u32 len = (u32)(span - from < ZPK_SC_PIECE ? span - from : ZPK_SC_PIECE);
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

}  // namespace zpk
