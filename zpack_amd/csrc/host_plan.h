// host_plan.h — the HOST-POINTER read path (zpk_codec_decode_batch_host, its _dptr forms, zpk_codec_verify_batch_host), decided in one
// place: the staging slot of an entry and what a sub-batch holds, the image that is staged for it (the archive's span or the gathered
// payloads), the pieces of the three-stage pipeline and why a sub-batch does not take it, the geometry of the double-buffered copies
// through the pinned buffers and what each host thread moves, the groups of frame-parallel entries and their staging, and the small
// rules of delivery.  zpk_codec.hip holds the grows, copies, events, launches and threads.
// The sub-batches are cut by dimage_cut (dimage_plan.h) over read_slot: ONE cut for the host path and the device image.  A slot that
// saturates (a compressed entry whose dst_capacity lies within 255 bytes of 2^64) therefore closes its sub-batch alone and its staging is
// refused before anything is enqueued (host_staging_refused) — the earlier cut of the host path gave such an entry a slot of 0 bytes.
// Plain C++17, span_copy_plan.h, dimage_plan.h, dec_plan.h, stored_plan.h (xxh3_span_blocks, the span row) and standard headers only:
// tools/hostfuzz builds this file with g++ under ASan + UBSan (g++ knows no HIP), which keeps it so.
#pragma once
#include <vector>
#include "span_copy_plan.h"
#include "dimage_plan.h"
#include "dec_plan.h"
#include "stored_plan.h"

namespace zpk {

#ifndef ZPK_PIN_CHUNK
#define ZPK_PIN_CHUNK (32ull << 20)              // bytes of each of the two pinned staging buffers: one piece of a double-buffered copy
#endif
#ifndef ZPK_SCATTER_THREADS
#define ZPK_SCATTER_THREADS 4u                   // host threads that move one piece: one copies at ~22 GB/s, the bus brings ~50
#endif
#ifndef ZPK_PIPE_PIECE
#define ZPK_PIPE_PIECE (64ull << 20)             // least output bytes of one piece of the three-stage pipeline
#endif
// the staged image is followed by ZPK_SRC_SLACK bytes of the codec's own: the kernels may READ ZPK_SRC_READ_SLACK bytes past its
// logical end (wide loads next to an entry's last byte; the two-stage LZ4 parser fetches whole 64-byte groups) — never interpret them
#define ZPK_SRC_SLACK 192u
#define ZPK_SRC_READ_SLACK 128u

// ---- the small rules ---------------------------------------------------------------------------------------------------------------------
static inline void sat_add(u64& acc, u64 v) { acc = v > ~0ull - acc ? ~0ull : acc + v; }
// what of an entry goes to the caller: what was produced, never more than the caller's capacity (cannot happen)
static inline u64 host_delivered(const zpk_decode_desc& d, const zpk_decode_result& r) { return r.produced > d.dst_capacity ? d.dst_capacity : r.produced; }
// dense: the whole range of slots comes home through the pinned buffers and is scattered; else one copy per entry that produced anything
// — a generous max_size costs device address space, not PCIe time
static inline bool host_deliver_dense(u64 n, u64 produced_total, u64 out_total) { return n > 1 && produced_total && produced_total * 2 >= out_total; }
// a SHORT decode (rehash_short_entries): the frames of a compressed entry ended before uncomp_size bytes existed and nothing else was
// wrong — lib/zpack_read.c:466 hashes buffer[0, uncomp_size) all the same, so the slot's tail is filled and the slot hashed again
static inline bool host_short_decode(const zpk_decode_desc& d, const zpk_decode_result& r)
{
    return (r.status == DEC_R_OK || r.status == DEC_R_FILE_HASH_MISMATCH) && r.produced < d.uncomp_size && dec_capacity_holds(d) &&
           dec_has_payload(d) /* :328: OK before anything is read */ && d.method != ZPK_METHOD_NONE;
}

// ---- the slot, and what a sub-batch holds ---------------------------------------------------------------------------------------------------
// The staging slot of an entry, for the host path and the device image alike: dimage_slot, which saturates; without a destination
// (the batch is only tested: the capacity counts as uncomp_size) a stored entry has none — it is hashed where it lies.
static inline u64 read_slot(bool no_destination, const zpk_decode_desc& d)
{
    const bool stored = d.method == ZPK_METHOD_NONE;
    return no_destination && stored ? 0ull : dimage_slot(stored, d.uncomp_size, d.dst_capacity);
}
// out_total + 16 bytes are asked of the device, with up to 256 of slack: a total that reaches the saturated slot holds in no allocation
static inline bool host_staging_refused(u64 out_total) { return out_total >= ZPK_DIMAGE_SLOT_MAX; }
// Of the sub-batch desc[0, n): the methods it holds, the span [lo, hi) of the archive that its payloads cover and their bytes — over the
// entries with a payload that lies inside the archive (the others are never read); no such entry: lo = hi = 0
struct HostSub { int zstd, lz4; u64 lo, hi, comp_sum; };
static inline HostSub host_sub(const zpk_decode_desc* desc, u64 n, u64 archive_size)
{
    HostSub s = { 0, 0, ~0ull, 0, 0 };
    for (u64 i = 0; i < n; i++) {
        const zpk_decode_desc& d = desc[i];
        if (dec_has_payload(d) && dec_src_in_image(d, archive_size)) { if (d.src_offset < s.lo) s.lo = d.src_offset; if (d.src_offset + d.comp_size > s.hi) s.hi = d.src_offset + d.comp_size; s.comp_sum += d.comp_size; }
        if (d.method == ZPK_METHOD_ZSTD) s.zstd = 1;
        if (d.method == ZPK_METHOD_LZ4) s.lz4 = 1;
    }
    if (s.lo > s.hi) s.lo = s.hi = 0;
    return s;
}

// ---- the image of a sub-batch ----------------------------------------------------------------------------------------------------------------
// Sparse picks out of a large archive: only the payloads are staged, gathered into an image of their own
static inline bool host_image_sparse(u64 lo, u64 hi, u64 comp_sum) { return hi - lo > 2 * comp_sum + (1u << 20); }
// The gathered image: the entries that pass the reference's offset guard (lib/zpack_read.c:331) are packed behind each other in batch
// order, followed by one pad byte at pad_at so that the guard still passes against image_size; every other entry gets fail_offset, which
// still fails it — the device evaluates the same guards in the same order.  Writes hd[i].src_offset; the caller copies comp_size bytes
// of each entry whose offset is not fail_offset and the pad byte into a buffer of image_size + 1 bytes.
struct HostGather { u64 image_size, pad_at, fail_offset; };
static inline HostGather host_gather_layout(const zpk_decode_desc* desc, u64 n, u64 archive_size, zpk_decode_desc* hd)
{
    const u64 total = host_sub(desc, n, archive_size).comp_sum + 1;
    u64 pos = 0;
    for (u64 i = 0; i < n; i++) {
        if (dec_has_payload(desc[i]) && dec_src_passes(desc[i], archive_size)) { hd[i].src_offset = pos; pos += desc[i].comp_size; }
        else hd[i].src_offset = total + 1;
    }
    return HostGather{ total, pos, total + 1 };
}

// ---- the pieces of the three-stage pipeline ------------------------------------------------------------------------------------------------
// A sub-batch is cut into pieces of at least ZPK_PIPE_PIECE output bytes and enough entries to fill the device (one wave per LZ4 entry,
// 48 Zstandard streams per CU); a tail of less than half of that joins the last piece.  Piece k: entries [e0, e1), the span
// [clo, chi) of the image that their payloads cover (what its upload sends), the output range [olo, ohi) of their slots.
#define ZPK_HOST_MAX_PIECES 64
struct HostPiece { u64 e0, e1, clo, chi, olo, ohi; };
static inline u64 host_pipe_min_entries(bool holds_zstd) { return holds_zstd ? 12288 : 4096; }
// Why a sub-batch takes decode_host_chunk instead: too small to be worth it, more pieces than events, a piece's span outside the staged
// range, fewer than three pieces, or entries that do not lie in the archive roughly in batch order (the spans would go up many times)
enum HostPipeRefusal { HOST_PIPE_TAKEN = 0, HOST_PIPE_TOO_SMALL, HOST_PIPE_TOO_MANY, HOST_PIPE_SPAN_OUTSIDE, HOST_PIPE_FEW, HOST_PIPE_OUT_OF_ORDER };
// hd[0, n): the staged descriptors (dst_offset = the slot), [lo, hi) the staged range of the image.  -> the number of pieces in out[], or
// 0 and *why
static inline int host_pieces(const zpk_decode_desc* hd, u64 n, u64 image_size, u64 lo, u64 hi, u64 out_total, u64 min_entries,
                              HostPiece out[ZPK_HOST_MAX_PIECES], HostPipeRefusal* why = nullptr)
{
    auto ends = [&](HostPipeRefusal r, int np) { if (why) *why = r; return np; };
    if (out_total < 3 * ZPK_PIPE_PIECE || n < 3 * min_entries) return ends(HOST_PIPE_TOO_SMALL, 0);
    int np = 0;
    u64 span_sum = 0;
    for (u64 i = 0; i < n; ) {
        if (np == ZPK_HOST_MAX_PIECES) return ends(HOST_PIPE_TOO_MANY, 0);
        HostPiece& P = out[np];
        P.e0 = i; P.olo = hd[i].dst_offset; P.clo = ~0ull; P.chi = 0;
        u64 bytes = 0;
        while (i < n && (bytes < ZPK_PIPE_PIECE || i - P.e0 < min_entries || n - i < min_entries / 2)) {
            const zpk_decode_desc& d = hd[i];
            if (dec_has_payload(d) && dec_src_in_image(d, image_size)) { if (d.src_offset < P.clo) P.clo = d.src_offset; if (d.src_offset + d.comp_size > P.chi) P.chi = d.src_offset + d.comp_size; }
            bytes += (i + 1 < n ? hd[i + 1].dst_offset : out_total) - d.dst_offset;
            i++;
        }
        P.e1 = i; P.ohi = i < n ? hd[i].dst_offset : out_total;
        if (P.clo > P.chi) { P.clo = lo; P.chi = lo; }
        if (P.clo < lo || P.chi > hi) return ends(HOST_PIPE_SPAN_OUTSIDE, 0);
        span_sum += P.chi - P.clo;
        np++;
    }
    if (np < 3) return ends(HOST_PIPE_FEW, 0);
    if (span_sum > (hi - lo) + (hi - lo) / 4 + (1u << 20)) return ends(HOST_PIPE_OUT_OF_ORDER, 0);
    return ends(HOST_PIPE_TAKEN, np);
}

// ---- the double-buffered copies through the pinned buffers (d2h_scatter, h2d_gather) ---------------------------------------------------------
// A staged range of `total` bytes moves in pieces of ZPK_PIN_CHUNK bytes, piece j = [p0, p1), through buffer j & 1
struct StagedPiece { u64 p0, p1; };
static inline u64 staged_pieces(u64 total) { return (total + ZPK_PIN_CHUNK - 1) / ZPK_PIN_CHUNK; }
static inline StagedPiece staged_piece(u64 j, u64 total) { const u64 p0 = j * ZPK_PIN_CHUNK; return StagedPiece{ p0, p0 + ZPK_PIN_CHUNK < total ? p0 + ZPK_PIN_CHUNK : total }; }
// Entry i owns bytes [off(i), off(i) + len(i)) of the range, ascending in i.  The entries that may reach into [p0, p1): [ei, ej) — ei is
// kept from piece to piece and only passes entries that end at or before p0; -> ej, the first that starts at or behind p1
template <class OffFn, class LenFn>
static inline u64 staged_reach(u64 p0, u64 p1, u64 n, u64& ei, OffFn off, LenFn len)
{
    while (ei < n && off(ei) + len(ei) <= p0) ei++;
    u64 ej = ei;
    while (ej < n && off(ej) < p1) ej++;
    return ej;
}
// the host threads of a piece: a piece below 4 MiB is one thread's
static inline unsigned staged_threads(u64 p0, u64 p1) { return p1 - p0 >= (4u << 20) ? ZPK_SCATTER_THREADS : 1u; }
// Share t of T: entries [lo_i, hi_i), of each what lies in bytes [lo_b, hi_b).  Eight entries or more are dealt out by count; of a few
// large entries the piece's BYTES are cut among the threads at multiples of 4 KiB (one entry of 256 MiB came home at one thread's rate)
struct StagedShare { u64 lo_i, hi_i, lo_b, hi_b; };
static inline StagedShare staged_share(u64 p0, u64 p1, u64 ei, u64 ej, unsigned t, unsigned T)
{
    const u64 cnt = ej - ei, span = p1 - p0;
    auto cut = [&](unsigned k) { return k >= T ? p1 : p0 + ((span * k / T) & ~(u64)4095); };
    if (cnt < 8) return StagedShare{ ei, ej, cut(t), cut(t + 1) };
    return StagedShare{ ei + cnt * t / T, ei + cnt * (t + 1) / T, p0, p1 };
}
// move(i, in_entry, in_piece, bytes) copies `bytes` bytes, at in_entry of entry i and at in_piece of the piece, whichever way the caller goes
template <class OffFn, class LenFn, class MoveFn>
static inline void staged_share_move(const StagedShare& s, u64 p0, OffFn off, LenFn len, MoveFn move)
{
    for (u64 i = s.lo_i; i < s.hi_i; i++) {
        const u64 o = off(i), l = len(i);
        const u64 a = o > s.lo_b ? o : s.lo_b, z = o + l < s.hi_b ? o + l : s.hi_b;
        if (z > a) move(i, a - o, a - p0, z - a);
    }
}

// ---- the groups of frame-parallel entries (decode_big_group) ---------------------------------------------------------------------------------
struct BigEntry { u64 idx, first_sub, nsub; };   // entry idx of its batch is the frames subs[first_sub, first_sub + nsub) (host_walk.h)
// The group that starts at be[g0]: entries [g0, g1), by the size of their output; its first entry always joins.  Without a destination
// stored entries and compressed ones form groups of their own — the stored ones are hashed in the staged source.
static inline u64 host_group_cut(const zpk_decode_desc* desc, const BigEntry* be, u64 nbe, u64 g0, bool no_destination)
{
    u64 g1 = g0, out = 0;
    auto same_kind = [&](u64 g) { return !no_destination || (desc[be[g].idx].method == ZPK_METHOD_NONE) == (desc[be[g0].idx].method == ZPK_METHOD_NONE); };
    while (g1 < nbe && (g1 == g0 || (same_kind(g1) && out + desc[be[g1].idx].uncomp_size <= ZPK_HOST_CHUNK_BYTES))) { out += (desc[be[g1].idx].uncomp_size + 255) & ~255ull; g1++; }
    return g1;
}
// The staging of the group be[g0, g1), ng entries: entry k's payload at coff[k] of c->d_src and its output at ooff[k] of c->d_dst, both at
// multiples of 256 (coff[ng] = ct and ooff[ng] = ot: the totals); hd = its frames as descriptors of one device batch, nsub of them, each
// inside its entry's two ranges, hash not asked for; spans[k] = the range the entry's XXH3 is taken over, its partial sums from part_base on.
// src_only (no destination, stored entries): no frames and no output — the spans lie over the staged SOURCE.
struct HostGroup { bool src_only; u64 nsub, ct, ot, part_blocks; int zstd, lz4; };
static inline HostGroup host_group_layout(const zpk_decode_desc* desc, const BigEntry* be, u64 g0, u64 g1, const BigSub* subs, bool no_destination,
                                          u64* coff, u64* ooff, StoredSpanRow* spans, std::vector<zpk_decode_desc>& hd)
{
    const u64 ng = g1 - g0;
    HostGroup G = { no_destination && desc[be[g0].idx].method == ZPK_METHOD_NONE, 0, 0, 0, 0, 0, 0 };
    for (u64 k = g0; k < g1 && !G.src_only; k++) G.nsub += be[k].nsub;
    hd.resize(G.nsub);
    u64 j = 0;
    for (u64 k = 0; k < ng; k++) {
        const BigEntry& E = be[g0 + k];
        const zpk_decode_desc& d = desc[E.idx];
        coff[k] = G.ct; ooff[k] = G.ot;
        for (u64 f = 0; f < E.nsub && !G.src_only; f++, j++) {
            const BigSub& S = subs[E.first_sub + f];
            zpk_decode_desc& x = hd[j];
            x.src_offset = G.ct + S.src_off; x.comp_size = S.comp; x.uncomp_size = S.size; x.expect_hash = 0;
            x.dst_offset = G.ot + S.out_off; x.dst_capacity = S.size; x.method = d.method; x.flags = ZPK_DF_SKIP_HASH;
        }
        spans[k] = StoredSpanRow{ G.src_only ? G.ct : G.ot, d.uncomp_size, G.part_blocks };
        G.part_blocks += xxh3_span_blocks(d.uncomp_size);
        G.ct += (d.comp_size + 255) & ~255ull; if (!G.src_only) G.ot += (d.uncomp_size + 255) & ~255ull;
        if (d.method == ZPK_METHOD_ZSTD) G.zstd = 1;
        if (d.method == ZPK_METHOD_LZ4) G.lz4 = 1;
    }
    coff[ng] = G.ct; ooff[ng] = G.ot;
    return G;
}

}  // namespace zpk
