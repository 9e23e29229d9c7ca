// dimage_plan.h — a batch read out of an archive image in DEVICE memory (zpk_codec_decode_batch_dimage), cut into sub-batches whose
// output slots fit the codec's staging: the slot of an entry, where the slots of a sub-batch lie, where a sub-batch ends.  The slots are
// the read slots of span_copy_plan.h — what the entry may produce, at multiples of 256, the host path's layout — because the
// block-parallel readers want their outputs on 256-byte boundaries: nothing is decoded straight into a caller's pointer.
// Plain C++17, span_copy_plan.h and standard headers only: tools/hostfuzz builds this file with g++ under ASan + UBSan (g++ knows no
// HIP), which keeps it so.
#pragma once
#include "span_copy_plan.h"

namespace zpk {

#ifndef ZPK_HOST_CHUNK_BYTES
#define ZPK_HOST_CHUNK_BYTES (4ull << 30)        // (dec_plan.h: output slots of one device sub-batch of the host path)
#endif
#define ZPK_DIMAGE_MAX_ENTRIES 0x7FFFFFF0ull     // entries of one sub-batch: what zpk_codec_decode_big_batch_device takes

// ZPK_OPT_DIMAGE_CHUNK: bytes of staging slots per sub-batch, 0 = the default
static inline u64 dimage_chunk(u64 option) { return option ? option : ZPK_HOST_CHUNK_BYTES; }

// The slot of one entry: span_copy_read_slot, which rounds up to 256 — saturated where that sum would wrap (a capacity within 255 bytes
// of 2^64): such a slot is larger than every chunk and than every allocation, the entry goes alone and its staging is refused.
#define ZPK_DIMAGE_SLOT_MAX (~0ull & ~255ull)
static inline u64 dimage_slot(bool stored, u64 uncomp_size, u64 dst_capacity)
{
    const u64 bytes = span_copy_read_slot_bytes(stored, uncomp_size, dst_capacity);
    return bytes > ZPK_DIMAGE_SLOT_MAX ? ZPK_DIMAGE_SLOT_MAX : span_copy_read_slot(stored, uncomp_size, dst_capacity);
}

// The sub-batch that starts at entry `first` of n, in the order given: entries [first, first + count), entry first + k at byte at[k] of
// the staging, out_total bytes in all.  It closes when the next slot would take it past `chunk` (or it holds max_entries); its first
// entry always joins, so an entry larger than the chunk goes alone.  Nothing wraps: every sum is compared as a difference.
// slot(i) = the slot of entry i; at = nullptr: the count and the total only.
struct DimageCut { u64 count, out_total; };
template <class SlotFn>
static inline DimageCut dimage_cut(u64 first, u64 n, u64 chunk, SlotFn slot, u64* at = nullptr, u64 max_entries = ZPK_DIMAGE_MAX_ENTRIES)
{
    DimageCut c = { 0, 0 };
    while (first + c.count < n && c.count < max_entries) {
        const u64 s = slot(first + c.count);
        if (c.count && (c.out_total > chunk || s > chunk - c.out_total)) break;
        if (at) at[c.count] = c.out_total;
        c.out_total += s;                                                            // (a first slot, or a sum that stays within chunk)
        c.count++;
    }
    return c;
}
}  // namespace zpk
