// k_sink_cut, k_sink_place: one sub-batch of zpk_codec_encode_batch_dsink committed to the caller's sink in DEVICE memory — the reference's
// append loop (lib/zpack_write.c:287-339: the files in front of the first failing one are appended) for a whole batch, without the host
// seeing a compressed byte.  Behind the encode and the pack scan: results[0, n), offsets[0, n] and span_first[0, n] (dsink_plan.h) are on
// the device; k_sink_cut finds where the batch ends, k_sink_place moves the payloads in front of that from their slots to the sink.
// The rules — what stops the batch, the items, an item's bytes —: dsink_plan.h.
#pragma once
#include "zpk_device.h"
#include "seq_exec.h"                            // gcopy_upto16
#include "dsink_plan.h"

namespace zpk {

// ONE workgroup.  f = the first entry that stops the batch (sink_stops), n when none does: every thread keeps the first such entry of its
// stride, one min across the wave, one across the four waves.
__global__ __launch_bounds__(256) void k_sink_cut(const zpk_encode_result* __restrict__ res, const u64* __restrict__ offsets, u32 n, u64 room,
                                                  u64* __restrict__ rec)
{
    __shared__ u32 part[4];
    u32 f = n;
    for (u32 i = threadIdx.x; i < n; i += 256u)
        if (sink_stops(res[i].status, offsets[i + 1], room)) { f = i; break; }
    #pragma unroll
    for (int k = 32; k >= 1; k >>= 1) { const u32 o = (u32)__shfl_xor((int)f, k, 64); f = o < f ? o : f; }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = f;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) f = part[w] < f ? part[w] : f;
        rec[0] = f; rec[1] = offsets[f]; rec[2] = 0;
    }
}

// `len` bytes from s to d, any alignment of either, by one wave: 16 bytes per lane, four loads in flight (the body of k_big_gather and
// k_span_copy), the rest through gcopy_upto16, whose accesses are as wide as what is left.  Every byte is read once and written once.
__device__ __forceinline__ void sink_wave_copy(u8* d, const u8* s, u32 len, int lane)
{
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

// A persistent grid, four waves per workgroup: a wave takes the next slot of four items of [0, span_first[f]) — the count is read from the
// device, no host bound sizes the work — finds the first item's entry among [0, f) by binary search over span_first, walks on from there
// for the others, and copies each item's bytes from its entry's slot (slots + slot_off[e]) to sink + offsets[e].  Only entries in front
// of the cut have items here, every one of them ends at or in front of offsets[f] = rec[1]: nothing is stored at or behind
// sink + rec[1].  No LDS.
__global__ __launch_bounds__(256) void k_sink_place(const u8* __restrict__ slots, const u64* __restrict__ slot_off,
                                                    const zpk_encode_result* __restrict__ res, const u64* __restrict__ offsets,
                                                    const u64* __restrict__ span_first, u64* __restrict__ rec, u8* __restrict__ sink)
{
    const int lane = lane_id();
    const u64 f = uni64(rec[0]), bytes = uni64(rec[1]);
    if (f == 0) return;
    const u64 items = uni64(span_first[f]);
    if (items > 0xFFFFFFFFull) return;                                               // (the host turns down a sub-batch that could hold more)
    const u32 count = (u32)sink_slots(items);
    u32* const head = (u32*)(rec + 2);
    u32 slot;
    while (dequeue(head, 0, count, lane, slot)) {
        u64 t = (u64)slot * ZPK_SINK_SLOT_ITEMS;
        const u64 t_end = t + ZPK_SINK_SLOT_ITEMS < items ? t + ZPK_SINK_SLOT_ITEMS : items;
        u64 e = sink_entry_of(span_first, f, t);
        u64 next = uni64(span_first[e + 1]);                                         // (e + 1 <= f)
        for (; t < t_end; t++) {
            while (t >= next) { e++; next = uni64(span_first[e + 1]); }              // (t < span_first[f]: e stays in front of f)
            const u64 at = uni64(offsets[e]);
            const SinkSpan sp = sink_span(uni64(res[e].comp_size), uni64(span_first[e]), t);
            if (sp.len == 0 || at + sp.from > bytes || sp.len > bytes - (at + sp.from)) continue;    // (never taken: an entry in front of the cut ends inside rec[1])
            sink_wave_copy(uni_ptr(sink + at + sp.from), uni_ptr(slots + slot_off[e] + sp.from), sp.len, lane);
        }
    }
}

}  // namespace zpk
