// span_copy_plan.h — the plaintext of a batch moved between the codec's staging and the CALLER'S DEVICE BUFFERS by one kernel
// (k_span_copy, span_copy.h), decided in one place for zpk_codec_decode_batch_host_dptr, zpk_codec_encode_batch_dsrc and
// zpk_codec_copy_spans_device: the row table the kernel reads, its work items and launches, where a sub-batch's slots lie in the staging
// (both directions), the offsets of the packed read, and the range test a caller's pointer has to pass before anything is enqueued
// (span_copy_in_range; who asks HIP for the allocation and under which policy: zpk_codec.hip, device_range_of and PtrRule — the one rule
// of every batch call and of zpk_codec_fetch_device / _store_device.  span_copy_enqueue there fills the row table from a callable).
// Plain C++17, pj_types.h and standard headers only: tools/hostfuzz builds this file with g++ under ASan + UBSan (g++ knows no HIP),
// which keeps it so.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "pj_types.h"                            // (the typedefs)

namespace zpk {

// ---- the row table ---------------------------------------------------------------------------------------------------------------------
// A WORK ITEM is 16 KiB of one span, one wave's: 64 lanes x 16 bytes x 4 loads in flight, four times.  Row k owns the items
// [item_base, item_base + span_copy_items(len)); item_base ascends without gaps, so the wave of item t finds its row as the LAST one with
// item_base <= t (the search of k_stored_span over part_base).  A span of no bytes takes no row and no item.
#define ZPK_SC_PIECE (16u << 10)
struct SpanCopyRow { u64 src, dst, len, item_base; };                                // src, dst: device addresses
struct SpanCopyPlan { u64 nrows, items; };
#define ZPK_SC_MAX_ROWS 0xFFFFFFFFull                // the kernel searches with 32-bit row numbers
static inline u64 span_copy_items(u64 len) { return len / ZPK_SC_PIECE + (len % ZPK_SC_PIECE ? 1 : 0); }       // (no sum that could wrap)
// Appends the span to the table.  false: the table is full (ZPK_SC_MAX_ROWS) — nothing is written.
static inline bool span_copy_emit(u64 src, u64 dst, u64 len, SpanCopyRow* rows, SpanCopyPlan& p)
{
    if (len == 0) return true;
    if (p.nrows >= ZPK_SC_MAX_ROWS) return false;
    rows[p.nrows] = SpanCopyRow{ src, dst, len, p.items };
    p.nrows++; p.items += span_copy_items(len);
    return true;
}
// the row of item t, as the kernel finds it
static inline u64 span_copy_row_of(const SpanCopyRow* rows, u64 nrows, u64 t)
{
    u64 lo = 0, hi = nrows;
    while (hi - lo > 1) { const u64 mid = (lo + hi) >> 1; if (rows[mid].item_base <= t) lo = mid; else hi = mid; }
    return lo;
}

// ---- the launches ----------------------------------------------------------------------------------------------------------------------
// Four items per workgroup; a grid holds at most max_items of them (the x limit of a grid), a table with more goes in several launches
// over the SAME table: launch j takes the items [j * max_items, ...), the kernel adds that base to its wave number.
#define ZPK_SC_MAX_ITEMS (4ull * 0x7FFFFFFFull)
struct SpanCopyLaunch { u64 item0, items; u32 grid; };
static inline u64 span_copy_launches(u64 items, u64 max_items = ZPK_SC_MAX_ITEMS) { return items / max_items + (items % max_items ? 1 : 0); }
static inline SpanCopyLaunch span_copy_launch(u64 items, u64 j, u64 max_items = ZPK_SC_MAX_ITEMS)
{
    SpanCopyLaunch L;
    L.item0 = j * max_items;
    L.items = items - L.item0 < max_items ? items - L.item0 : max_items;
    L.grid = (u32)((L.items + 3) / 4);
    return L;
}

// ---- where a sub-batch's slots lie in the staging ----------------------------------------------------------------------------------------
// Reading (c->d_dst): a stored entry copies exactly uncomp_size bytes (lib/zpack_read.c:366), the decoders may fill all of max_size; the
// slots follow each other at multiples of 256.  What goes to the caller is [slot, slot + produced).
static inline u64 span_copy_read_slot_bytes(bool stored, u64 uncomp_size, u64 dst_capacity) { return stored && uncomp_size < dst_capacity ? uncomp_size : dst_capacity; }
static inline u64 span_copy_read_slot(bool stored, u64 uncomp_size, u64 dst_capacity) { return (span_copy_read_slot_bytes(stored, uncomp_size, dst_capacity) + 255) & ~255ull; }
// The descriptor the device sees of an entry staged at `slot_offset` (Desc: zpk_decode_desc; `stored`: its method is NONE): the caller's,
// with dst_offset = the slot.  The device still judges `max_size < uncomp_size` on the caller's capacity, so dst_capacity stays as given —
// except for a stored entry that passes that guard: it writes uncomp_size bytes and its slot is that long.
template <class Desc> static inline Desc span_copy_staged_desc(const Desc& d, bool stored, u64 slot_offset)
{
    Desc s = d;
    s.dst_offset = slot_offset;
    if (stored && d.dst_capacity >= d.uncomp_size) s.dst_capacity = span_copy_read_slot_bytes(true, d.uncomp_size, d.dst_capacity);
    return s;
}
// Writing (c->d_src): the sources follow each other at multiples of 256 with at least 16 bytes behind each — the slack the encode
// kernels' 16-byte loads ask for, which a caller's own allocation cannot promise.
static inline u64 span_copy_write_slot(u64 size) { return (size + 255 + 16) & ~255ull; }

// ---- the packed read ---------------------------------------------------------------------------------------------------------------------
// zpack_amd_read_files_device_packed: entry i lands at the running sum of the uncomp_size of the entries before it, each rounded up to 256
// (every entry starts on a boundary the 16-byte accesses like, whatever the sizes before it).  Saturates instead of wrapping: a position
// past every buffer leaves no room, which is BUFFER_TOO_SMALL.
static inline u64 span_copy_packed_stride(u64 uncomp_size) { return uncomp_size > ~0ull - 255 ? ~0ull & ~255ull : (uncomp_size + 255) & ~255ull; }
static inline u64 span_copy_packed_next(u64 pos, u64 uncomp_size)
{
    const u64 s = span_copy_packed_stride(uncomp_size);
    return pos > (~0ull & ~255ull) - s ? ~0ull & ~255ull : pos + s;
}

// ---- the pointer test ---------------------------------------------------------------------------------------------------------------------
// [ptr, ptr + len) lies inside the allocation [base, base + size).  Every sum is a difference: ptr + len may wrap, this does not.  A span
// of no bytes touches nothing and passes wherever it points.
static inline bool span_copy_in_range(u64 ptr, u64 len, u64 base, u64 size)
{
    if (len == 0) return true;
    return ptr >= base && ptr - base <= size && len <= size - (ptr - base);
}

}  // namespace zpk
