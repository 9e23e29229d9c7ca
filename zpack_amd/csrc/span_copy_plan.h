// span_copy_plan.h — the plaintext of a batch moved between the codec's staging and the CALLER'S DEVICE BUFFERS by one kernel
// (k_span_copy, row_copy.hip), decided in one place for zpk_codec_decode_batch_host_dptr, zpk_codec_encode_batch_dsrc and
// zpk_codec_copy_spans_device: the row table the kernel reads (items and launches: copy_rows_plan.h), where a sub-batch's slots lie in the
// staging (both directions), the offsets of the packed read, and the range test a caller's pointer has to pass before anything is enqueued
// (span_copy_in_range; who asks HIP for the allocation and under which policy: zpk_codec.hip, device_range_of and PtrRule — the one rule
// of every batch call and of zpk_codec_fetch_device / _store_device.  span_copy_enqueue there fills the row table from a callable).
// Plain C++17, pj_types.h and standard headers only: tools/hostfuzz builds this file with g++ under ASan + UBSan (g++ knows no HIP),
// which keeps it so.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "pj_types.h"                            // (the typedefs)
#include "copy_rows_plan.h"                      // the 16 KiB item, the search and the launches that the four row copies share

namespace zpk {

// ---- the row table ---------------------------------------------------------------------------------------------------------------------
// The 16 KiB work item, the items of a row, the search and the launches: copy_rows_plan.h.  A span of no bytes takes no row and no item.
struct SpanCopyRow { u64 src, dst, len, item_base; };                                // src, dst: device addresses
// Appends the span to the table.  false: the table is full (ZPK_COPY_MAX_ROWS) — nothing is written.
static inline bool span_copy_emit(u64 src, u64 dst, u64 len, SpanCopyRow* rows, CopyPlan& p)
{
    if (len == 0) return true;
    if (p.nrows >= ZPK_COPY_MAX_ROWS) return false;
    rows[p.nrows] = SpanCopyRow{ src, dst, len, p.items };
    p.nrows++; p.items += copy_items(len);
    return true;
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
