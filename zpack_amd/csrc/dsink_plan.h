// dsink_plan.h — a batch compressed INTO A BOUNDED SINK IN DEVICE MEMORY (zpk_codec_encode_batch_dsink), decided in one place for the host
// code that stages and chains the sub-batches and for the two kernels that commit one (sink_commit.h): where the batch is cut — the
// reference's append rule, lib/zpack_write.c:299-303, with "does not fit" as one more way to fail —, the span table of the copy, the room
// a sub-batch finds behind the one before it, the staging slots and the sub-batches.
// Plain C++17, dimage_plan.h (span_copy_plan.h) and standard headers only: tools/hostfuzz builds this file with g++ under ASan + UBSan
// (g++ knows no HIP), which keeps it so.  The predicates are also device code (k_sink_cut, k_sink_place): ZPK_HD is empty on a CPU build.
#pragma once
#include "dimage_plan.h"

#ifndef ZPK_HD
#ifdef __HIPCC__
#define ZPK_HD __host__ __device__
#else
#define ZPK_HD
#endif
#endif

namespace zpk {

// ---- the cut ---------------------------------------------------------------------------------------------------------------------------
// offsets[0, n] = the exclusive prefix sums of the comp_size of the entries with status 0 (a failed entry takes no room: the pack scan).
// Entry i STOPS the batch when it failed or when it would end behind the room: status != 0 || offsets[i + 1] > room.  The cut f is the
// first such entry, n when there is none; entries [0, f) are placed at sink + offsets[i], offsets[f] bytes in all, and nothing is written
// at or behind sink + offsets[f].  The sums ascend, so "first" is one min over the entries that stop.
struct SinkCut { u64 placed, bytes; };
// The record the two kernels share and the host reads: rec[0] = the cut f, rec[1] = offsets[f], the bytes placed; rec[2] = the head of
// k_sink_place's dequeue (a u32 in its low half), which k_sink_cut sets to 0 for every launch.
#define SINK_REC_WORDS 3
ZPK_HD static inline bool sink_stops(int32_t status, u64 end_offset, u64 room) { return status != 0 || end_offset > room; }
// the restatement the kernel is checked against: statuses and sizes as the encoders leave them, the sums taken here
static inline SinkCut sink_cut(const int32_t* status, const u64* comp_size, u64 n, u64 room)
{
    SinkCut c = { 0, 0 };
    for (; c.placed < n; c.placed++) {
        if (status[c.placed] != 0) break;
        const u64 size = comp_size[c.placed];
        if (size > room || c.bytes > room - size) break;                             // (c.bytes + size > room, without the sum)
        c.bytes += size;
    }
    return c;
}

// ---- the span table ----------------------------------------------------------------------------------------------------------------------
// A WORK ITEM of the copy is (entry, span of ZPK_SINK_SPAN bytes of its payload), one wave's; entry i owns the items
// [span_first[i], span_first[i + 1]), span_first = the exclusive prefix sums of sink_spans(size of i when status 0).  The items of the
// entries in front of the cut are [0, span_first[f]).  An entry without bytes owns no item.
// What the persistent grid dequeues is a SLOT of ZPK_SINK_SLOT_ITEMS consecutive items, [slot * 4, slot * 4 + 4) — across entries where
// they end: one atomic on the queue's head per 64 KiB copied (one per item, 60 000 for 20 000 entries of 64 KiB, was what the kernel
// waited for: 13 ns each, 0.79 ms for 0.77 GB).
#define ZPK_SINK_SPAN (16u << 10)
#define ZPK_SINK_SLOT_ITEMS 4u
ZPK_HD static inline u64 sink_spans(u64 size) { return size / ZPK_SINK_SPAN + (size % ZPK_SINK_SPAN ? 1 : 0); }
ZPK_HD static inline u64 sink_slots(u64 items) { return items / ZPK_SINK_SLOT_ITEMS + (items % ZPK_SINK_SLOT_ITEMS ? 1 : 0); }
// the entry of item t: the LAST one with span_first[e] <= t (entries without items share their successor's value and are passed over)
ZPK_HD static inline u64 sink_entry_of(const u64* span_first, u64 n, u64 t)
{
    u64 lo = 0, hi = n;
    while (hi - lo > 1) { const u64 mid = lo + ((hi - lo) >> 1); if (span_first[mid] <= t) lo = mid; else hi = mid; }
    return lo;
}
// bytes of item t of an entry of `size` bytes whose first item is `first`: [from, from + len) of its payload; len 0: not an item of it
struct SinkSpan { u64 from; u32 len; };
ZPK_HD static inline SinkSpan sink_span(u64 size, u64 first, u64 t)
{
    SinkSpan s = { (t - first) * (u64)ZPK_SINK_SPAN, 0 };
    if (t < first || s.from >= size) return s;
    s.len = (u32)(size - s.from < ZPK_SINK_SPAN ? size - s.from : ZPK_SINK_SPAN);
    return s;
}
// an upper bound of the items of a sub-batch that needs no result (it only caps the grid): every entry has at most sink_spans(capacity)
static inline u64 sink_items_bound(u64 bound_so_far, u64 dst_capacity)
{
    const u64 s = sink_spans(dst_capacity);
    return bound_so_far > ~0ull - s ? ~0ull : bound_so_far + s;
}
// workgroups of the persistent launch: four waves each, no more than the chip holds at once and no more than there can be slots
static inline u32 sink_grid(u64 items_bound, u32 resident_groups)
{
    const u64 slots = sink_slots(items_bound), want = slots / 4 + (slots % 4 ? 1 : 0);
    const u64 g = want < resident_groups ? want : resident_groups;
    return (u32)(g ? g : 1);
}

// ---- room and chaining --------------------------------------------------------------------------------------------------------------------
// What is left of a sink of `capacity` bytes of which `used` are taken (the library: the writer's file_size; between sub-batches: what
// the ones before placed).  A sub-batch whose cut is short of its entries ends the call: the entry at the cut is the one the caller
// judges (its status, or BUFFER_TOO_SMALL), nothing behind it is looked at — the reference's loop stops at the first failing file.
ZPK_HD static inline u64 sink_room(u64 capacity, u64 used) { return used < capacity ? capacity - used : 0; }
struct SinkChain { u64 placed, bytes; bool open; };                                  // over the whole call; open: the next sub-batch runs
static inline void sink_chain(SinkChain& ch, u64 sub_entries, SinkCut cut)
{
    ch.placed += cut.placed; ch.bytes += cut.bytes;
    if (cut.placed < sub_entries) ch.open = false;
}

// ---- staging ---------------------------------------------------------------------------------------------------------------------------
// A sub-batch's sources lie in the codec's staging as the host path's do (span_copy_write_slot: multiples of 256, 16 bytes of slack behind
// each), its frames in slots of the caller's capacity at multiples of 256 — saturated where the sum would wrap, as dimage_slot is.  The
// sub-batches are cut by the bytes of those output slots (dimage_cut): an entry larger than the chunk goes alone.
static inline u64 sink_slot(u64 dst_capacity) { return dst_capacity > ZPK_DIMAGE_SLOT_MAX ? ZPK_DIMAGE_SLOT_MAX : (dst_capacity + 255) & ~255ull; }
static inline u64 sink_src_slot(u64 size) { return size > ZPK_DIMAGE_SLOT_MAX - 256 ? ZPK_DIMAGE_SLOT_MAX : span_copy_write_slot(size); }

}  // namespace zpk
