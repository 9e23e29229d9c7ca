// dec_plan.h — a LARGE entry's route on the read side, decided in one place for zpk_codec_decode_batch_host, zpk_codec_decode_big_device
// and zpk_codec_decode_big_batch_device (the read-side counterpart of enc_plan.h): the guards of lib/zpack_read.c as named predicates,
// which entries may leave the one-wave path at all, which of the accepted single frames earn a turn of the whole chip, the staging
// layout of k_big_walk (big_walk.h), the verdict of a finished entry.
// Plain C++17, the public header, pj_types.h / host_walk.h and standard headers only: tools/hostfuzz builds this file with g++ under
// ASan + UBSan (g++ knows no HIP), which keeps it so.  ZPK_HD is empty on a CPU build.
#pragma once
#include <algorithm>
#include <vector>
#include "../../include/zpack_codec.h"
#include "host_walk.h"                           // pj_types.h, walk_lz4_capacity / walk_zstd_capacity, ZPK_HD

namespace zpk {

#ifndef ZPK_HOST_CHUNK_BYTES
#define ZPK_HOST_CHUNK_BYTES (4ull << 30)        // output slots of one device sub-batch of the host path (an entry larger than this goes alone)
#endif
#define ZPK_DEC_SPLIT_MIN_DEFAULT (256ull << 10)     // (round 5: a single 512 KiB LZ4 entry is 0.66 ms block-parallel against 3.3 ms by one wave, 1 MiB of Zstandard 4.3 against 31.7: tools/mid_entry_rate.py)

// ---- the guards ------------------------------------------------------------------------------------------------------------------------
// k_classify evaluates lib/zpack_read.c:328-348 in the reference's order and alone says BUFFER_TOO_SMALL / FILE_OFFSET_INVALID /
// FILE_SIZE_INVALID: an entry that fails one of these stays with the one-wave launch.  Nothing here wraps: every sum is a difference.
ZPK_HD static inline bool dec_has_payload(const zpk_decode_desc& d) { return d.comp_size != 0; }                           // :328 — else OK, nothing produced
ZPK_HD static inline bool dec_capacity_holds(const zpk_decode_desc& d) { return d.dst_capacity >= d.uncomp_size; }         // :329
// :331 as the reference states it, STRICT: offset + comp_size < file_size — an entry that ends where the image ends fails
ZPK_HD static inline bool dec_src_passes(const zpk_decode_desc& d, u64 image_size) { return d.src_offset <= image_size && d.comp_size < image_size - d.src_offset; }
// ... and NOT strict: the entry's bytes lie inside the image, so they can be staged — whether or not :331 then lets it pass
ZPK_HD static inline bool dec_src_in_image(const zpk_decode_desc& d, u64 image_size) { return d.src_offset <= image_size && d.comp_size <= image_size - d.src_offset; }
// the slot [dst_offset, dst_offset + uncomp_size) lies inside dst (the device-resident calls: not the reference's, the kernels' own bound)
ZPK_HD static inline bool dec_slot_in_dst(const zpk_decode_desc& d, u64 dst_size) { return d.dst_offset <= dst_size && d.uncomp_size <= dst_size - d.dst_offset; }
// every guard of :328-348 passes: what is left for the entry is OK or a hash mismatch
ZPK_HD static inline bool dec_guards_pass(const zpk_decode_desc& d, u64 image_size) { return dec_has_payload(d) && dec_capacity_holds(d) && dec_src_passes(d, image_size); }

// ---- which entries may leave the one-wave path -------------------------------------------------------------------------------------------
// split_min: zpk_codec::dec_split_min (~0: none).  The host form takes the three methods (a stored entry may go in pieces, a compressed one
// as a sequence of frames or as one block-parallel frame) ...
ZPK_HD static inline bool dec_big_candidate(const zpk_decode_desc& d, u64 archive_size, u64 split_min)
{
    if (split_min == ~0ull || d.uncomp_size < split_min || d.uncomp_size > ZPK_HOST_CHUNK_BYTES) return false;
    return d.method <= ZPK_METHOD_LZ4 && dec_guards_pass(d, archive_size);
}
// ... the device-resident forms the compressed ones whose slot lies inside dst (the stored ones: stored_plan.h)
ZPK_HD static inline bool dec_big_candidate_device(const zpk_decode_desc& d, u64 archive_size, u64 dst_size, u64 split_min) { return d.method != ZPK_METHOD_NONE && dec_big_candidate(d, archive_size, split_min) && dec_slot_in_dst(d, dst_size); }

// ---- which single frames go block-parallel ----------------------------------------------------------------------------------------------
// One at a time, each fills the chip: a fixed cost + its bytes at ~12 GiB/s — while the entries of the usual batch all run side by side,
// one wave each: a batch of a hundred 3 MiB entries is done in the time of ONE of them there.  The batch's time is (the block-parallel
// entries, one after the other) + (the longest one-wave entry left): the largest entries go block-parallel as long as that sum shrinks.
// (measured, tools/mid_entry_rate.py + big_frame_rate.py)
#define DEC_WAVE_GIBS_LZ4         0.15           // one wave, LZ4
#define DEC_WAVE_GIBS_LZ4_STORED  1.0            // ... when the entry did not compress
#define DEC_WAVE_GIBS_ZSTD        0.031          // one wave, Zstandard
#define DEC_WAVE_GIBS_ZSTD_STORED 0.9            // ... when the entry did not compress
#define DEC_PJ_FIXED_MS_LZ4       0.6            // block-parallel: 0.6 ms + 12 GiB/s LZ4
#define DEC_PJ_FIXED_MS_ZSTD      4.2            // ... 4.2 ms + 12 GiB/s Zstandard
#define DEC_PJ_GIBS               12.0
#define DEC_CHOOSE_SLACK          1.1            // the estimates are rough: as many as come within 10 % of the best
#define DEC_WAVE_OTHER_MIN        (64u << 10)    // a non-candidate shorter than this never is the longest one-wave entry
static inline double dec_wave_ms(const zpk_decode_desc& d)
{
    const double mib = (double)d.uncomp_size / (1 << 20);
    const bool stored_like = d.comp_size >= d.uncomp_size - d.uncomp_size / 16;
    return mib / 1.024 / (d.method == ZPK_METHOD_LZ4 ? (stored_like ? DEC_WAVE_GIBS_LZ4_STORED : DEC_WAVE_GIBS_LZ4) : (stored_like ? DEC_WAVE_GIBS_ZSTD_STORED : DEC_WAVE_GIBS_ZSTD));
}
static inline double dec_pj_ms(const zpk_decode_desc& d) { return (d.method == ZPK_METHOD_LZ4 ? DEC_PJ_FIXED_MS_LZ4 : DEC_PJ_FIXED_MS_ZSTD) + (double)d.uncomp_size / (1 << 20) / DEC_PJ_GIBS / 1.024; }
// cand[0, nc) = the entries of desc[0, n) whose frames the walk accepted.  -> the POSITIONS in `cand` of those that go block-parallel, in
// the order they are to run (the longest by one wave first); every other entry stays with the one-wave launch.
static inline std::vector<u64> dec_choose(const zpk_decode_desc* desc, u64 n, const u64* cand, u64 nc)
{
    std::vector<u64> order(nc);
    if (nc == 0) return order;
    for (u64 k = 0; k < nc; k++) order[k] = k;
    std::sort(order.begin(), order.end(), [&](u64 a, u64 b) { return dec_wave_ms(desc[cand[a]]) > dec_wave_ms(desc[cand[b]]); });
    double other = 0;                                                         // the longest entry that is not a candidate at all
    { std::vector<u8> is_cand(n, 0); for (u64 k = 0; k < nc; k++) is_cand[cand[k]] = 1;
      for (u64 i = 0; i < n; i++) if (!is_cand[i] && desc[i].method != ZPK_METHOD_NONE && desc[i].uncomp_size >= DEC_WAVE_OTHER_MIN) { const double t = dec_wave_ms(desc[i]); if (t > other) other = t; } }
    std::vector<double> tk(nc + 1);
    double best = 1e300, acc = 0;
    for (u64 k = 0; k <= nc; k++) {                                           // the first k block-parallel
        const double rest_ms = k < nc ? dec_wave_ms(desc[cand[order[k]]]) : 0.0;
        tk[k] = acc + (rest_ms > other ? rest_ms : other);
        if (tk[k] < best) best = tk[k];
        if (k < nc) acc += dec_pj_ms(desc[cand[order[k]]]);
    }
    u64 keep = nc;
    while (keep > 0 && tk[keep] > DEC_CHOOSE_SLACK * best) keep--;
    order.resize(keep);
    return order;
}

// ---- the staging of k_big_walk -----------------------------------------------------------------------------------------------------------
struct BigWalkItem {                     // host -> device, one per candidate
    u64 src_off, comp, uncomp;           // the entry: d_archive + src_off, comp bytes (inside the archive: the caller's guards passed), its stated size
    u64 tab_off;                         // its table in the staging buffer (byte offset, 16-aligned)
    u32 cap, method;                     // table capacity in blocks (walk_*_capacity: a function of uncomp alone); ZPK_METHOD_LZ4 / _ZSTD
};
struct BigWalkRec {                      // device -> host, one per candidate
    u32 accepted, nblocks;               // 1: the frame is the block-parallel readers' and tab[0, nblocks) is its table; 0: the one-wave decoder's
    u32 independent, pad;                // LZ4: the blocks do not reach into each other
    u64 slots, lit_total;                // Zstandard: sequence slots, bytes of the literal arena
};
// [ items | records | tables ], the same layout on the device and in pinned host memory: items[k] describes candidate cand[k] and says
// where its table lies and how many blocks it holds.  rec_off = where the records start, total = the end of the last table.
struct BigWalkLayout { u64 rec_off, total; };
static inline BigWalkLayout dec_walk_layout(const zpk_decode_desc* desc, const u64* cand, u64 nc, std::vector<BigWalkItem>& items)
{
    BigWalkLayout L;
    L.rec_off = (nc * sizeof(BigWalkItem) + 255) & ~255ull;
    L.total = L.rec_off + ((nc * sizeof(BigWalkRec) + 255) & ~255ull);
    items.resize(nc);
    for (u64 k = 0; k < nc; k++) {
        const zpk_decode_desc& d = desc[cand[k]];
        const bool lz4 = d.method == ZPK_METHOD_LZ4;
        const u64 cap = lz4 ? walk_lz4_capacity(d.uncomp_size) : walk_zstd_capacity(d.uncomp_size);
        BigWalkItem& it = items[k];
        it.src_off = d.src_offset; it.comp = d.comp_size; it.uncomp = d.uncomp_size; it.tab_off = L.total; it.cap = (u32)cap; it.method = d.method;
        L.total += (cap * (lz4 ? sizeof(PjBlock) : sizeof(ZpjBlock)) + 15) & ~15ull;
    }
    return L;
}

// ---- the verdict ------------------------------------------------------------------------------------------------------------------------
// Of an entry that was decoded in full and hashed: field for field what the reference leaves (lib/zpack_read.c:466-468) — the hash is
// always produced, ZPK_DF_SKIP_HASH keeps it out of the status.
enum : int { DEC_R_OK = 0, DEC_R_FILE_HASH_MISMATCH = 15 };
ZPK_HD static inline zpk_decode_result dec_hash_verdict(const zpk_decode_desc& d, u64 hash)
{
    zpk_decode_result r;
    r.status = (!(d.flags & ZPK_DF_SKIP_HASH) && hash != d.expect_hash) ? DEC_R_FILE_HASH_MISMATCH : DEC_R_OK;
    r.detail = 0; r.produced = d.uncomp_size; r.hash = hash;
    return r;
}

}  // namespace zpk
