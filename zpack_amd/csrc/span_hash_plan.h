// span_hash_plan.h — XXH3-64 of ARBITRARY spans of device memory, spans that are no entries of an archive (the bases of delta entries, a
// tensor a caller wants to compare with an entry's recorded hash): k_span_hash (span_hash.h) gives a row one wave, a long row goes
// chip-wide through the partial sums and the chain of xxh3_span.h.  Decided here, in one place: which rows go where, the two tables the
// kernels read, where the hashes and the partial sums lie, the launches, and for every row the exact bytes its 16-byte loads touch.
// Plain C++17, stored_plan.h (for xxh3_span_blocks and the group size) and standard headers only: tools/hostfuzz builds this file with
// g++ under ASan + UBSan (g++ knows no HIP), which keeps it so.
#pragma once
#include "stored_plan.h"

namespace zpk {

// ---- which rows go chip-wide --------------------------------------------------------------------------------------------------------------
// One wave hashes at its load latency, ~1 GiB/s: a row of at least `threshold` bytes (zpk_codec::span_hash_min, ~0: never) is cut into
// groups of 64 blocks of 1 KiB, one wave each, whose block sums one chain wave folds (xxh3_span.h).  A row without a full block in front
// of the block with its last byte has no group: 1025 bytes is the least, as for the stored spans (stored_plan.h).
#define ZPK_SPAN_HASH_LEAST ZPK_STORED_SPAN_LEAST
ZPK_HD static inline bool span_hash_wide(u64 len, u64 threshold)
{
    return threshold != ~0ull && len >= (threshold > ZPK_SPAN_HASH_LEAST ? threshold : ZPK_SPAN_HASH_LEAST);
}

// ---- the two tables ---------------------------------------------------------------------------------------------------------------------
// The one-wave rows, in the order given: row j of the table is hashed by wave j and its hash is out[j].
struct SpanHashRow { u64 addr, len; };
// The chip-wide rows, in the order given: row k is the zpk_span of xxh3_span.h with the source pointer null, so `off` IS the address;
// part_base ascends in multiples of 64; its hash is out[nwave + k].
struct SpanHashWide { u64 off, len, part_base; };
struct SpanHashPlan { u64 nwave, nwide, part_blocks, groups; };                       // part_blocks = 64 * groups: partial-sum slots of all chip-wide rows
#define ZPK_SPAN_HASH_MAX_ROWS 0x7FFFFFFFull                                          // k_xxh3_partials searches with 32-bit row numbers
// where[i] of a row given as i: its slot in `out` (one-wave rows first, then the chip-wide ones)
#define ZPK_SPAN_HASH_WIDE_BIT (1ull << 63)
// Appends row (addr, len) to the table it belongs to and returns what the caller keeps for it: the row's index in ITS table, with
// ZPK_SPAN_HASH_WIDE_BIT set for a chip-wide row.  ~0: the tables are full — nothing is written.
static inline u64 span_hash_emit(u64 addr, u64 len, u64 threshold, SpanHashRow* wave, SpanHashWide* wide, SpanHashPlan& p)
{
    if (p.nwave + p.nwide >= ZPK_SPAN_HASH_MAX_ROWS) return ~0ull;
    if (!span_hash_wide(len, threshold)) { wave[p.nwave] = SpanHashRow{ addr, len }; return p.nwave++; }
    const u64 g = xxh3_span_blocks(len) / ZPK_SPAN_GROUP;
    wide[p.nwide] = SpanHashWide{ addr, len, p.part_blocks };
    p.groups += g; p.part_blocks += g * ZPK_SPAN_GROUP;
    return ZPK_SPAN_HASH_WIDE_BIT | p.nwide++;
}
ZPK_HD static inline u64 span_hash_out_slot(u64 kept, u64 nwave) { return kept & ZPK_SPAN_HASH_WIDE_BIT ? nwave + (kept & ~ZPK_SPAN_HASH_WIDE_BIT) : kept; }

// ---- one block of device memory (and its pinned twin): tables going up, hashes coming home, the partial sums --------------------------------
// [ one-wave rows | chip-wide rows | out: nwave + nwide hashes | partial sums: 64 bytes per slot ]; the partial sums start at a multiple of
// 256 and exist on the device only.
struct SpanHashLayout { u64 wave_rows, wide_rows, out, partial, bytes, up_bytes; };   // byte offsets; up_bytes: what the upload copies (both tables)
static inline SpanHashLayout span_hash_layout(const SpanHashPlan& p)
{
    SpanHashLayout L;
    L.wave_rows = 0;
    L.wide_rows = p.nwave * sizeof(SpanHashRow);
    L.up_bytes = L.wide_rows + p.nwide * sizeof(SpanHashWide);
    L.out = L.up_bytes;
    L.partial = (L.out + (p.nwave + p.nwide) * 8 + 255) & ~255ull;
    L.bytes = L.partial + p.part_blocks * 64;
    return L;
}

// ---- the launches ----------------------------------------------------------------------------------------------------------------------
// k_span_hash: four rows per workgroup; k_xxh3_partials: four groups per workgroup; k_xxh3_chain: one row per workgroup.  A grid holds at
// most `max` of them (the x limit of a grid), more go in several launches over the SAME tables: launch j takes [j * max, ...).
#define ZPK_SPAN_HASH_MAX_WAVE_ROWS (4ull * 0x7FFFFFFFull)
#define ZPK_SPAN_HASH_MAX_GROUPS ZPK_STORED_MAX_GROUPS
#define ZPK_SPAN_HASH_MAX_CHAINS ZPK_STORED_MAX_SPANS
struct SpanHashLaunch { u64 first, count; u32 grid; };
static inline u64 span_hash_launches(u64 total, u64 max) { return total / max + (total % max ? 1 : 0); }
// per: rows or groups per workgroup (4: k_span_hash, k_xxh3_partials; 1: k_xxh3_chain)
static inline SpanHashLaunch span_hash_launch(u64 total, u64 j, u64 max, u32 per)
{
    SpanHashLaunch L;
    L.first = j * max;
    L.count = total - L.first < max ? total - L.first : max;
    L.grid = (u32)((L.count + per - 1) / per);
    return L;
}
// the chip-wide row of group g, as k_xxh3_partials finds it: the last one with part_base / 64 <= g
static inline u64 span_hash_wide_of(const SpanHashWide* wide, u64 nwide, u64 g)
{
    u64 lo = 0, hi = nwide;
    while (hi - lo > 1) { const u64 mid = (lo + hi) >> 1; if (wide[mid].part_base / ZPK_SPAN_GROUP <= g) lo = mid; else hi = mid; }
    return lo;
}

// ---- the bytes a row's loads touch -------------------------------------------------------------------------------------------------------
// Of a row of len > 240 bytes: the `blocks` full 1 KiB blocks in front of the block with the last byte, [0, blocks << 10), by 16-byte
// loads, lane l of a block at 16 l (one wave: block after block; chip-wide: group g of the row takes the blocks [64 g, 64 g + 64) and
// writes their sums to the slots part_base + 64 g ...); then `stripes` whole 64-byte stripes behind them, [blocks << 10, stripes_end), and
// the LAST stripe [len - 64, len), which overlaps what came before it as the hash defines — both by Xxh3Wave::finish.  stripes_end < len
// and len - stripes_end <= 64: together they cover the row, and no load leaves it.  A row of len <= 240 is read by xxh3_short, every load
// of which lies inside [0, len) (xxh3_device.h); len == 0 reads nothing.
struct SpanHashLoads { u64 blocks, stripes, stripes_end, last_from; };
ZPK_HD static inline SpanHashLoads span_hash_loads(u64 len)
{
    SpanHashLoads L;
    L.blocks = (len - 1) >> 10;
    L.stripes = ((len - 1) - (L.blocks << 10)) >> 6;
    L.stripes_end = (L.blocks << 10) + (L.stripes << 6);
    L.last_from = len - 64;
    return L;
}

}  // namespace zpk
