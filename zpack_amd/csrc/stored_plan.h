// stored_plan.h — the large STORED entries of a device-resident batch, copied and hashed by the whole chip (k_stored_span, stored_span.h),
// decided in one place for zpk_codec_decode_big_batch_device and zpk_codec_decode_big_device: which entries are taken, the span table the
// two kernels read.  The guards and the verdict of a finished entry are dec_plan.h's, shared with the compressed entries of the same calls.
// Plain C++17, the public header, dec_plan.h and standard headers only: tools/hostfuzz builds this file with g++ under ASan + UBSan (g++
// knows no HIP), which keeps it so.
#pragma once
#include "dec_plan.h"                            // (the public header, the typedefs, ZPK_HD)

namespace zpk {

// ---- the layout of the partial sums (xxh3_span.h) -------------------------------------------------------------------------------------
// A span of `len` bytes has (len - 1) >> 10 full 1 KiB blocks in front of the block with its last byte; a GROUP is 64 of them, one wave's
// work in k_xxh3_partials / k_stored_span, and a span's partial sums start at a multiple of 64 (part_base).
#define ZPK_SPAN_GROUP 64u                       // = XS_GROUP
ZPK_HD static inline u64 xxh3_span_blocks(u64 len) { return (((len - 1) >> 10) + ZPK_SPAN_GROUP - 1) / ZPK_SPAN_GROUP * ZPK_SPAN_GROUP; }   // partial-sum slots of one span

// ---- which entries are taken ------------------------------------------------------------------------------------------------------------
// The guards are dec_plan.h's (lib/zpack_read.c:328-348) and :354, with the answers that lead to k_stored: an entry that fails one stays
// with the one-wave launch, whose k_classify alone says BUFFER_TOO_SMALL / FILE_OFFSET_INVALID / FILE_SIZE_INVALID, in the reference's order.
// A span without a full block has no group to carry its tail: 1025 bytes is the least.  threshold: zpk_codec::stored_span_min (~0: never).
#define ZPK_STORED_SPAN_LEAST 1025ull
ZPK_HD static inline bool stored_span_takes(const zpk_decode_desc& d, u64 archive_size, u64 dst_size, u64 threshold)
{
    if (d.method != ZPK_METHOD_NONE) return false;
    if (!dec_guards_pass(d, archive_size)) return false;                             // :328 (OK, nothing produced), :329, :331
    if (d.uncomp_size > d.comp_size) return false;                                   // :354
    if (!dec_slot_in_dst(d, dst_size)) return false;
    return d.uncomp_size >= (threshold > ZPK_STORED_SPAN_LEAST ? threshold : ZPK_STORED_SPAN_LEAST);
}

// ---- the span table ---------------------------------------------------------------------------------------------------------------------
// Row k of `rows` is the zpk_span of xxh3_span.h (k_xxh3_chain reads the rows as they are: off = the SOURCE offset, so the chain hashes
// block sums and a tail that came from the source), dst_off[k] the byte offset of the span's copy.  part_base ascends in multiples of 64.
struct StoredSpanRow { u64 off, len, part_base; };
struct StoredPlan { u64 nspans, part_blocks, groups; };                              // part_blocks = 64 * groups: partial-sum slots of all spans
// one launch: four groups per workgroup, the grid's x limit; one chain wave per span
#define ZPK_STORED_MAX_GROUPS (4ull * 0x7FFFFFFFull)
#define ZPK_STORED_MAX_SPANS 0x7FFFFFFFull
// Appends entry d (one that stored_span_takes) to the table.  false: its groups no longer fit the launch (max_groups) — nothing is
// written, the entry and every later one stay with the one-wave launch.
static inline bool stored_span_emit(const zpk_decode_desc& d, StoredSpanRow* rows, u64* dst_off, StoredPlan& p, u64 max_groups = ZPK_STORED_MAX_GROUPS)
{
    const u64 g = xxh3_span_blocks(d.uncomp_size) / ZPK_SPAN_GROUP;
    if (p.nspans >= ZPK_STORED_MAX_SPANS || g > max_groups || p.groups > max_groups - g) return false;
    rows[p.nspans] = StoredSpanRow{ d.src_offset, d.uncomp_size, p.part_blocks };
    dst_off[p.nspans] = d.dst_offset;
    p.nspans++; p.groups += g; p.part_blocks += g * ZPK_SPAN_GROUP;
    return true;
}

// ---- the verdict: dec_hash_verdict (dec_plan.h), field for field what k_stored writes (lib/zpack_read.c:466-468) --------------------------
ZPK_HD static inline zpk_decode_result stored_span_verdict(const zpk_decode_desc& d, u64 hash) { return dec_hash_verdict(d, hash); }

}  // namespace zpk
