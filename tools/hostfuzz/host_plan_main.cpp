// zpack_amd/csrc/host_plan.h, the header the codec compiles, under ASan + UBSan: the host-pointer read path's decisions — the slot and the
// cut, the gathered image, the pipeline's pieces, the shares of the staged copies, the groups of frame-parallel entries, the small rules.
// Two legs.  EQUIVALENCE: the loops these functions replaced, copied as they stood into the model_* functions below, over random batches
// whose sizes stay below 2^62 (no sum of the old loops wraps there, so no case is left out).  PROPERTIES that hold without a model.
// Built and run by tools/hostfuzz/run_host_plan.sh (from the repository's root: the status values come from tests/golden/status_cases.json)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include <string>
#include <vector>
#include "host_plan.h"
using namespace zpk;

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd() { u64& x = rng_state; x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; }
static bool same(const zpk_decode_desc& a, const zpk_decode_desc& b)
{
    return a.src_offset == b.src_offset && a.comp_size == b.comp_size && a.uncomp_size == b.uncomp_size && a.expect_hash == b.expect_hash &&
           a.dst_offset == b.dst_offset && a.dst_capacity == b.dst_capacity && a.method == b.method && a.flags == b.flags;
}

// ================================================================ the model: the loops as they stood ==========================================
static u64 model_staging_slot(bool none, const zpk_decode_desc& d)
{
    const bool stored = d.method == ZPK_METHOD_NONE;
    return none ? (stored ? 0ull : span_copy_read_slot(false, d.uncomp_size, d.uncomp_size)) : span_copy_read_slot(stored, d.uncomp_size, d.dst_capacity);
}
struct ModelSub { u64 cnt, out_total, lo, hi, comp_sum; int has_zstd, has_lz4; };
// (hd: indexed as desc is; max_entries stood as the literal 0x7FFFFFF0)
static ModelSub model_cut(const zpk_decode_desc* desc, u64 first, u64 n, u64 archive_size, u64 chunk_bytes, bool none, zpk_decode_desc* hd, u64 max_entries)
{
    u64 out_total = 0, cnt = 0, lo = ~0ull, hi = 0, comp_sum = 0;
    int has_zstd = 0, has_lz4 = 0;
    while (first + cnt < n) {
        const zpk_decode_desc& d = desc[first + cnt];
        const u64 slot = model_staging_slot(none, d);
        if (cnt && (out_total + slot > chunk_bytes || cnt >= max_entries)) break;
        hd[first + cnt] = span_copy_staged_desc(d, d.method == ZPK_METHOD_NONE, out_total);
        out_total += slot;
        if (dec_has_payload(d) && dec_src_in_image(d, archive_size)) { if (d.src_offset < lo) lo = d.src_offset; if (d.src_offset + d.comp_size > hi) hi = d.src_offset + d.comp_size; comp_sum += d.comp_size; }
        if (d.method == ZPK_METHOD_ZSTD) has_zstd = 1;
        if (d.method == ZPK_METHOD_LZ4) has_lz4 = 1;
        cnt++;
    }
    if (lo > hi) { lo = 0; hi = 0; }
    return ModelSub{ cnt, out_total, lo, hi, comp_sum, has_zstd, has_lz4 };
}
static bool model_sparse(u64 lo, u64 hi, u64 comp_sum) { return hi - lo > 2 * comp_sum + (1u << 20); }
// the block behind that test, without its memcpys: -> total; pos = where the pad byte goes
static u64 model_gather(const zpk_decode_desc* desc, u64 first, u64 cnt, u64 archive_size, u64 comp_sum, zpk_decode_desc* hd, u64& pos)
{
    const u64 total = comp_sum + 1;
    pos = 0;
    for (u64 i = first; i < first + cnt; i++) {
        const zpk_decode_desc& d = desc[i];
        if (dec_has_payload(d) && dec_src_passes(d, archive_size)) { hd[i].src_offset = pos; pos += d.comp_size; }
        else hd[i].src_offset = total + 1;
    }
    return total;
}
static int model_pieces(const zpk_decode_desc* hd, u64 n, u64 image_size, u64 lo, u64 hi, u64 out_total, bool holds_zstd, HostPiece* pc)
{
    const u64 min_entries = holds_zstd ? 12288 : 4096;
    if (out_total < 3 * ZPK_PIPE_PIECE || n < 3 * min_entries) return 0;
    int np = 0;
    u64 span_sum = 0;
    for (u64 i = 0; i < n; ) {
        if (np == 64) return 0;
        HostPiece& P = pc[np];
        P.e0 = i; P.olo = hd[i].dst_offset; P.clo = ~0ull; P.chi = 0;
        u64 out = 0;
        while (i < n && (out < ZPK_PIPE_PIECE || i - P.e0 < min_entries || n - i < min_entries / 2)) {
            const zpk_decode_desc& d = hd[i];
            const bool ok = d.comp_size && d.src_offset <= image_size && d.comp_size <= image_size - d.src_offset;
            if (ok) { if (d.src_offset < P.clo) P.clo = d.src_offset; if (d.src_offset + d.comp_size > P.chi) P.chi = d.src_offset + d.comp_size; }
            const u64 next = i + 1 < n ? hd[i + 1].dst_offset : out_total;
            out += next - d.dst_offset;
            i++;
        }
        P.e1 = i; P.ohi = i < n ? hd[i].dst_offset : out_total;
        if (P.clo > P.chi) { P.clo = lo; P.chi = lo; }
        if (P.clo < lo || P.chi > hi) return 0;
        span_sum += P.chi - P.clo;
        np++;
    }
    if (np < 3 || span_sum > (hi - lo) + (hi - lo) / 4 + (1u << 20)) return 0;
    return np;
}
// staged_piece_copy up to its threads: the moves of share t, in order
struct Move { u64 i, in_entry, in_piece, bytes; };
static void model_piece(u64 p0, u64 p1, u64 n, u64& ei, const std::vector<u64>& offs, const std::vector<u64>& lens, unsigned& T_out, std::vector<std::vector<Move>>& moves)
{
    auto off = [&](u64 i) { return offs[i]; };
    auto len = [&](u64 i) { return lens[i]; };
    while (ei < n && off(ei) + len(ei) <= p0) ei++;
    u64 ej = ei;
    while (ej < n && off(ej) < p1) ej++;
    const u64 cnt = ej - ei, span = p1 - p0;
    const unsigned T = span >= (4u << 20) ? ZPK_SCATTER_THREADS : 1u;
    auto cut = [&](unsigned t) { return t >= T ? p1 : p0 + ((span * t / T) & ~(u64)4095); };
    auto share = [&](unsigned t) {
        const bool by_bytes = cnt < 8;
        const u64 lo_i = by_bytes ? ei : ei + cnt * t / T, hi_i = by_bytes ? ej : ei + cnt * (t + 1) / T;
        const u64 lo_b = by_bytes ? cut(t) : p0, hi_b = by_bytes ? cut(t + 1) : p1;
        for (u64 i = lo_i; i < hi_i; i++) {
            const u64 o = off(i), l = len(i);
            const u64 a = o > lo_b ? o : lo_b, z = o + l < hi_b ? o + l : hi_b;
            if (z > a) moves[t].push_back(Move{ i, a - o, a - p0, z - a });
        }
    };
    T_out = T;
    moves.assign(T, std::vector<Move>());
    for (unsigned t = 0; t < T; t++) share(t);
}
static u64 model_group_cut(const zpk_decode_desc* desc, const std::vector<BigEntry>& be, u64 g0, bool none)
{
    u64 g1 = g0, out = 0;
    auto same_kind = [&](u64 g) { return !none || (desc[be[g].idx].method == ZPK_METHOD_NONE) == (desc[be[g0].idx].method == ZPK_METHOD_NONE); };
    while (g1 < be.size() && (g1 == g0 || (same_kind(g1) && out + desc[be[g1].idx].uncomp_size <= ZPK_HOST_CHUNK_BYTES))) { out += (desc[be[g1].idx].uncomp_size + 255) & ~255ull; g1++; }
    return g1;
}
struct ModelGroup { bool src_only; u64 nsub, ct, ot, part_blocks; int has_zstd, has_lz4; std::vector<u64> coff, ooff; std::vector<StoredSpanRow> spans; std::vector<zpk_decode_desc> hd; };
static ModelGroup model_group(const zpk_decode_desc* desc, const BigEntry* be, u64 g0, u64 g1, const std::vector<BigSub>& subs, bool none)
{
    ModelGroup M;
    const u64 ng = g1 - g0;
    const bool src_only = none && desc[be[g0].idx].method == ZPK_METHOD_NONE;
    u64 nsub = 0;
    for (u64 k = g0; k < g1 && !src_only; k++) nsub += be[k].nsub;
    std::vector<u64> coff(ng + 1), ooff(ng + 1);
    std::vector<StoredSpanRow> spans(ng);
    std::vector<zpk_decode_desc> hd(nsub);
    u64 ct = 0, ot = 0, part_blocks = 0, j = 0;
    int has_zstd = 0, has_lz4 = 0;
    for (u64 k = 0; k < ng; k++) {
        const BigEntry& E = be[g0 + k];
        const zpk_decode_desc& d = desc[E.idx];
        coff[k] = ct; ooff[k] = ot;
        for (u64 f = 0; f < E.nsub && !src_only; f++, j++) {
            const BigSub& S = subs[E.first_sub + f];
            zpk_decode_desc& x = hd[j];
            x.src_offset = ct + S.src_off; x.comp_size = S.comp; x.uncomp_size = S.size; x.expect_hash = 0;
            x.dst_offset = ot + S.out_off; x.dst_capacity = S.size; x.method = d.method; x.flags = ZPK_DF_SKIP_HASH;
        }
        spans[k].off = src_only ? ct : ot; spans[k].len = d.uncomp_size; spans[k].part_base = part_blocks;
        part_blocks += xxh3_span_blocks(d.uncomp_size);
        ct += (d.comp_size + 255) & ~255ull; if (!src_only) ot += (d.uncomp_size + 255) & ~255ull;
        if (d.method == ZPK_METHOD_ZSTD) has_zstd = 1;
        if (d.method == ZPK_METHOD_LZ4) has_lz4 = 1;
    }
    coff[ng] = ct; ooff[ng] = ot;
    M.src_only = src_only; M.nsub = nsub; M.ct = ct; M.ot = ot; M.part_blocks = part_blocks; M.has_zstd = has_zstd; M.has_lz4 = has_lz4;
    M.coff = coff; M.ooff = ooff; M.spans = spans; M.hd = hd;
    return M;
}

// ================================================================ the cut and the image ========================================================
// a random batch: sizes and capacities below 2^62; `kind` picks small entries, mixed ones, or a few enormous ones; `scatter`: the payloads
// lie far apart (sparse picks) instead of behind each other; none: the descriptors of a call without a destination (capacity = uncomp_size)
static std::vector<zpk_decode_desc> random_batch(u64 n, int kind, bool scatter, bool none, u64& archive_size)
{
    std::vector<zpk_decode_desc> d(n);
    u64 pos = 10 + rnd() % 100;
    for (u64 i = 0; i < n; i++) {
        const u64 r = rnd();
        zpk_decode_desc& x = d[i];
        x.method = (u32)(r % 3); x.flags = (u32)((r >> 8) & 1); x.expect_hash = rnd(); x.dst_offset = rnd();
        x.uncomp_size = kind == 0 ? r % 5000 : kind == 1 ? r % (300u << 10) : (r % 8 ? r % 70000 : (r >> 2));
        x.comp_size = (r >> 16) % 11 == 0 ? 0 : x.method == ZPK_METHOD_NONE && (r >> 20) % 5 ? x.uncomp_size : 1 + (r >> 24) % 40000;
        const u64 cr = rnd();
        x.dst_capacity = none ? x.uncomp_size : cr % 4 == 0 ? x.uncomp_size : cr % 4 == 1 ? x.uncomp_size + cr % 1000 : cr % 4 == 2 ? (cr >> 8) % (x.uncomp_size + 1) : (cr >> 2);
        if (scatter) pos += rnd() % (8u << 20);
        x.src_offset = (r >> 30) % 13 == 0 ? rnd() >> 2 : pos;                        // (now and then anywhere: most of those lie outside the archive)
        if (x.src_offset == pos) pos += x.comp_size;
    }
    archive_size = pos + rnd() % 3;                                                   // (+0: the last entry ends where the archive ends and fails :331)
    return d;
}

static void leg_cut_and_image(u64& batches, u64& subs_seen, u64& sparse_seen)
{
    for (int it = 0; it < 3000; it++) {
        const u64 n = rnd() % 160;
        const bool none = it % 3 == 0, scatter = it % 4 == 1;
        u64 archive_size;
        const std::vector<zpk_decode_desc> desc = random_batch(n, it % 5 % 3, scatter, none, archive_size);
        const u64 chunks[] = { 1, 65536, 1u << 20, rnd() % (4u << 20), ZPK_HOST_CHUNK_BYTES };
        const u64 chunk = chunks[rnd() % 5], max_entries = it % 6 == 0 ? 1 + rnd() % 20 : ZPK_DIMAGE_MAX_ENTRIES;
        std::vector<zpk_decode_desc> mhd(n), hd(n);
        std::vector<u64> at(n + 1, 0xA5A5A5A5A5A5A5A5ull);
        u64 covered = 0;
        for (u64 first = 0; first < n; ) {
            // ---- equivalence ----
            const ModelSub M = model_cut(desc.data(), first, n, archive_size, chunk, none, mhd.data(), max_entries);
            const DimageCut cut = dimage_cut(first, n, chunk, [&](u64 i) { return read_slot(none, desc[i]); }, at.data() + first, max_entries);
            CHECK(cut.count == M.cnt && cut.out_total == M.out_total && !host_staging_refused(cut.out_total));
            for (u64 k = 0; k < cut.count; k++) {
                hd[first + k] = span_copy_staged_desc(desc[first + k], desc[first + k].method == ZPK_METHOD_NONE, at[first + k]);
                CHECK(same(hd[first + k], mhd[first + k]));
            }
            const HostSub S = host_sub(desc.data() + first, cut.count, archive_size);
            CHECK(S.lo == M.lo && S.hi == M.hi && S.comp_sum == M.comp_sum && S.zstd == M.has_zstd && S.lz4 == M.has_lz4);
            CHECK(host_image_sparse(S.lo, S.hi, S.comp_sum) == model_sparse(M.lo, M.hi, M.comp_sum));
            u64 mpos;
            const u64 mtotal = model_gather(desc.data(), first, M.cnt, archive_size, M.comp_sum, mhd.data(), mpos);
            const HostGather G = host_gather_layout(desc.data() + first, cut.count, archive_size, hd.data() + first);
            CHECK(G.image_size == mtotal && G.pad_at == mpos && G.fail_offset == mtotal + 1);
            for (u64 k = 0; k < cut.count; k++) CHECK(same(hd[first + k], mhd[first + k]));
            // ---- properties: the cut ----
            CHECK(first == covered && cut.count >= 1 && cut.count <= max_entries);
            CHECK(cut.count == 1 || cut.out_total <= chunk);
            for (u64 k = 0; k < cut.count; k++) CHECK(at[first + k] % 256 == 0 && (k == 0 ? at[first] == 0 : at[first + k] == at[first + k - 1] + read_slot(none, desc[first + k - 1])));
            if (first + cut.count < n) CHECK(at[first + cut.count] == 0xA5A5A5A5A5A5A5A5ull);
            // ---- properties: the gathered image ----
            u64 expect = 0;
            for (u64 k = 0; k < cut.count; k++) {
                const zpk_decode_desc& h = hd[first + k];
                if (h.src_offset != G.fail_offset) { CHECK(h.src_offset == expect && dec_src_passes(h, G.image_size)); expect += h.comp_size; }      // disjoint, in batch order
                else CHECK(!dec_src_passes(h, G.image_size) && !(dec_has_payload(desc[first + k]) && dec_src_passes(desc[first + k], archive_size)));
            }
            CHECK(expect == G.pad_at && G.pad_at < G.image_size);                     // ... and end at the pad byte, inside the image
            sparse_seen += host_image_sparse(S.lo, S.hi, S.comp_sum);
            covered += cut.count; first += cut.count; subs_seen++;
        }
        CHECK(covered == n);
        batches++;
    }
    // a saturated slot goes alone, wherever it stands, and its total trips the refusal; the earlier slot of such an entry was 0
    for (u64 cap : { ~0ull, ~0ull - 100, ~0ull - 254 }) {
        zpk_decode_desc d[3] = {};
        for (int i = 0; i < 3; i++) { d[i].method = ZPK_METHOD_LZ4; d[i].comp_size = 100; d[i].uncomp_size = 1000; d[i].dst_capacity = 1000; d[i].src_offset = 100 * i; }
        d[1].dst_capacity = cap;
        CHECK(read_slot(false, d[1]) == ZPK_DIMAGE_SLOT_MAX && model_staging_slot(false, d[1]) == 0);
        u64 at[3];
        u64 counts[3], totals[3], nsub = 0;
        for (u64 first = 0; first < 3; nsub++) {
            const DimageCut cut = dimage_cut(first, 3, ZPK_HOST_CHUNK_BYTES, [&](u64 i) { return read_slot(false, d[i]); }, at);
            counts[nsub] = cut.count; totals[nsub] = cut.out_total; first += cut.count;
        }
        CHECK(nsub == 3 && counts[0] == 1 && counts[1] == 1 && counts[2] == 1);
        CHECK(!host_staging_refused(totals[0]) && host_staging_refused(totals[1]) && !host_staging_refused(totals[2]));
    }
    {   // a capacity 256 bytes further from 2^64 does not saturate and is not refused here (no device holds it: the allocation fails)
        zpk_decode_desc d = {}; d.method = ZPK_METHOD_ZSTD; d.comp_size = 1; d.uncomp_size = 5; d.dst_capacity = ~0ull - 511;
        CHECK(read_slot(false, d) == ZPK_DIMAGE_SLOT_MAX - 256 && !host_staging_refused(read_slot(false, d)));
        d.method = ZPK_METHOD_NONE; d.dst_capacity = ~0ull;
        CHECK(read_slot(false, d) == 256 && read_slot(true, d) == 0);                  // a stored entry: uncomp_size when it fits; none without a destination
    }
}

// ================================================================ the pieces ===================================================================
// a sub-batch as the pipeline sees it: slots of `slot(i)` bytes behind each other, payloads of `comp` bytes at src(i)
template <class SlotFn, class SrcFn>
static std::vector<zpk_decode_desc> staged(u64 n, SlotFn slot, SrcFn src, u64 comp, u64& out_total)
{
    std::vector<zpk_decode_desc> hd(n);
    out_total = 0;
    for (u64 i = 0; i < n; i++) { hd[i] = zpk_decode_desc{ src(i), comp, slot(i), 0, out_total, slot(i), ZPK_METHOD_LZ4, 0 }; out_total += slot(i); }
    return hd;
}
static void check_pieces(const zpk_decode_desc* hd, u64 n, u64 lo, u64 hi, u64 out_total, u64 min_entries, const HostPiece* pc, int np)
{
    CHECK(np >= 3 && np <= ZPK_HOST_MAX_PIECES && pc[0].e0 == 0 && pc[np - 1].e1 == n && pc[0].olo == hd[0].dst_offset && pc[np - 1].ohi == out_total);
    for (int k = 0; k < np; k++) {
        const HostPiece& P = pc[k];
        if (k) CHECK(P.e0 == pc[k - 1].e1 && P.olo == pc[k - 1].ohi);
        CHECK(P.e0 < P.e1 && P.olo <= P.ohi && P.clo <= P.chi && P.clo >= lo && P.chi <= hi);
        if (k + 1 < np) CHECK(P.e1 - P.e0 >= min_entries && P.ohi - P.olo >= ZPK_PIPE_PIECE);
        else CHECK(P.e1 - P.e0 >= min_entries / 2);
    }
}
static void leg_pieces(u64& cases, u64& taken)
{
    static HostPiece pc[ZPK_HOST_MAX_PIECES], mpc[64];
    for (int it = 0; it < 160; it++) {
        const bool zstd = it % 5 == 0;
        const u64 min_entries = host_pipe_min_entries(zstd);
        CHECK(min_entries == (zstd ? 12288u : 4096u));
        const u64 n = it % 9 == 0 ? rnd() % (3 * min_entries) : 3 * min_entries - 2 + rnd() % (6 * min_entries);
        const u64 base = it % 7 == 0 ? 1024 : (4u << 10) << (rnd() % 5), comp = 1 + rnd() % 3000;
        const int order = (int)(rnd() % 4);                                           // in archive order, with gaps, shuffled, a few strays
        const u64 big_at = rnd() % (n + 1);
        u64 out_total;
        const std::vector<zpk_decode_desc> hd = staged(n, [&](u64 i) { return i == big_at && it % 3 == 0 ? (u64)(300u << 20) : ((base + rnd() % base) + 255) & ~255ull; },
            [&](u64 i) { return 64 + (order == 2 ? (i * 7919) % n : i) * (comp + (order == 1 ? 100 : 0)) + (order == 3 && i % 5000 == 77 ? 1u << 30 : 0); }, comp, out_total);
        u64 lo = ~0ull, hi = 0;
        const u64 image_size = 64 + n * (comp + 100) + (order == 3 && it % 2 ? 2u << 30 : 0) + 1;
        for (u64 i = 0; i < n; i++) if (dec_src_in_image(hd[i], image_size)) { if (hd[i].src_offset < lo) lo = hd[i].src_offset; if (hd[i].src_offset + comp > hi) hi = hd[i].src_offset + comp; }
        if (lo > hi) lo = hi = 0;
        HostPipeRefusal why;
        const int np = host_pieces(hd.data(), n, image_size, lo, hi, out_total, min_entries, pc, &why);
        const int mnp = model_pieces(hd.data(), n, image_size, lo, hi, out_total, zstd, mpc);
        CHECK(np == mnp && (np == 0) == (why != HOST_PIPE_TAKEN));
        for (int k = 0; k < np; k++) CHECK(!memcmp(&pc[k], &mpc[k], sizeof(HostPiece)));
        if (np) { check_pieces(hd.data(), n, lo, hi, out_total, min_entries, pc, np); taken++; }
        cases++;
    }
    // ---- each refusal, and the least sub-batch that is taken ----
    HostPipeRefusal why;
    u64 out_total;
    auto seq = [](u64 comp) { return [comp](u64 i) { return 64 + i * comp; }; };
    {   // 12 288 entries of 16 KiB: three pieces of exactly 4 096 entries and 64 MiB
        const std::vector<zpk_decode_desc> hd = staged(12288, [](u64) { return (u64)16384; }, seq(1000), 1000, out_total);
        const u64 lo = 64, hi = 64 + 12288 * 1000ull;
        CHECK(host_pieces(hd.data(), 12288, hi + 1, lo, hi, out_total, 4096, pc, &why) == 3 && why == HOST_PIPE_TAKEN && pc[1].e0 == 4096 && pc[2].e0 == 8192 && pc[0].chi == pc[1].clo);
        check_pieces(hd.data(), 12288, lo, hi, out_total, 4096, pc, 3);
        CHECK(host_pieces(hd.data(), 12288, hi + 1, lo, hi, out_total, host_pipe_min_entries(true), pc, &why) == 0 && why == HOST_PIPE_TOO_SMALL);     // too few entries for Zstandard
        CHECK(host_pieces(hd.data(), 12287, hi + 1, lo, hi, out_total - 16384, 4096, pc, &why) == 0 && why == HOST_PIPE_TOO_SMALL);                    // one entry less
        CHECK(host_pieces(hd.data(), 12288, hi + 1, lo + 1, hi, out_total, 4096, pc, &why) == 0 && why == HOST_PIPE_SPAN_OUTSIDE);                     // the first payload in front of the staged range
        CHECK(host_pieces(hd.data(), 12288, hi + 1, lo, hi - 1, out_total, 4096, pc, &why) == 0 && why == HOST_PIPE_SPAN_OUTSIDE);
        CHECK(host_pieces(hd.data(), 12288, 64, 0, 0, out_total, 4096, pc, &why) == 3);                                                                // no payload inside the image: empty spans at lo
        // a tail of 2 047 entries joins the last piece, one of 2 048 is a piece of its own
        const std::vector<zpk_decode_desc> a = staged(12288 + 2047, [](u64) { return (u64)16384; }, seq(1000), 1000, out_total);
        CHECK(host_pieces(a.data(), a.size(), ~0ull, 0, ~0ull, out_total, 4096, pc, &why) == 3 && pc[2].e1 - pc[2].e0 == 4096 + 2047);
        const std::vector<zpk_decode_desc> b = staged(12288 + 2048, [](u64) { return (u64)16384; }, seq(1000), 1000, out_total);
        CHECK(host_pieces(b.data(), b.size(), ~0ull, 0, ~0ull, out_total, 4096, pc, &why) == 4 && pc[3].e1 - pc[3].e0 == 2048);
    }
    {   // 192 MiB less one slot
        const std::vector<zpk_decode_desc> hd = staged(12288, [](u64 i) { return (u64)(i ? 16384 : 16128); }, seq(1000), 1000, out_total);
        CHECK(out_total == 3 * ZPK_PIPE_PIECE - 256 && host_pieces(hd.data(), 12288, ~0ull, 0, ~0ull, out_total, 4096, pc, &why) == 0 && why == HOST_PIPE_TOO_SMALL);
    }
    {   // one entry of 200 MiB in front of 12 287 small ones: two pieces
        const std::vector<zpk_decode_desc> hd = staged(12288, [](u64 i) { return (u64)(i ? 256 : 200u << 20); }, seq(100), 100, out_total);
        CHECK(host_pieces(hd.data(), 12288, ~0ull, 0, ~0ull, out_total, 4096, pc, &why) == 0 && why == HOST_PIPE_FEW);
    }
    {   // 65 pieces
        const u64 n = 65 * 4096;
        const std::vector<zpk_decode_desc> hd = staged(n, [](u64) { return (u64)16384; }, seq(10), 10, out_total);
        CHECK(host_pieces(hd.data(), n, ~0ull, 0, ~0ull, out_total, 4096, pc, &why) == 0 && why == HOST_PIPE_TOO_MANY);
        CHECK(host_pieces(hd.data(), n - 2049, ~0ull, 0, ~0ull, out_total - 2049 * 16384ull, 4096, pc, &why) == 64 && why == HOST_PIPE_TAKEN);
    }
    {   // payloads all over the archive: every piece's span is nearly all of it
        const u64 n = 12288;
        const std::vector<zpk_decode_desc> hd = staged(n, [](u64) { return (u64)16384; }, [n](u64 i) { return 64 + (i * 7919) % n * 1000; }, 1000, out_total);
        CHECK(host_pieces(hd.data(), n, ~0ull, 64, 64 + n * 1000, out_total, 4096, pc, &why) == 0 && why == HOST_PIPE_OUT_OF_ORDER);
    }
}

// ================================================================ the shares ===================================================================
// entries at offs/lens of a range of `total` bytes through every piece: the model's moves, and every byte of every entry moved exactly once
static void run_range(const std::vector<u64>& offs, const std::vector<u64>& lens, u64 total, u64& moves_seen)
{
    const u64 n = offs.size();
    auto off = [&](u64 i) { return offs[i]; };
    auto len = [&](u64 i) { return lens[i]; };
    std::vector<u8> want(total, 0);
    for (u64 i = 0; i < n; i++) for (u64 b = 0; b < lens[i]; b++) want[offs[i] + b]++;
    CHECK(staged_pieces(total) == (total + ZPK_PIN_CHUNK - 1) / ZPK_PIN_CHUNK);
    for (unsigned force : { 0u, 1u, 4u }) {                                           // the piece's own thread count, then T = 1 and T = 4 whatever its size
        std::vector<u8> map(total, 0);
        u64 ei = 0, mei = 0, end = 0;
        for (u64 j = 0; j < staged_pieces(total); j++) {
            const StagedPiece p = staged_piece(j, total);
            CHECK(p.p0 == end && p.p1 > p.p0 && p.p1 - p.p0 <= ZPK_PIN_CHUNK && p.p1 <= total);
            end = p.p1;
            const u64 ej = staged_reach(p.p0, p.p1, n, ei, off, len);
            for (u64 i = 0; i < ei; i++) CHECK(offs[i] + lens[i] <= p.p0);               // no entry that still reaches into this piece was passed
            for (u64 i = ej; i < n; i++) CHECK(offs[i] >= p.p1);
            unsigned mT;
            std::vector<std::vector<Move>> mm;
            model_piece(p.p0, p.p1, n, mei, offs, lens, mT, mm);
            const unsigned T = force ? force : staged_threads(p.p0, p.p1);
            CHECK(mei == ei && staged_threads(p.p0, p.p1) == mT && mT == (p.p1 - p.p0 >= (4u << 20) ? 4u : 1u));
            for (unsigned t = 0; t < T; t++) {
                size_t at = 0;
                staged_share_move(staged_share(p.p0, p.p1, ei, ej, t, T), p.p0, off, len, [&](u64 i, u64 in_entry, u64 in_piece, u64 bytes) {
                    CHECK(i >= ei && i < ej && bytes && in_entry + bytes <= lens[i] && in_piece + bytes <= p.p1 - p.p0 && offs[i] + in_entry == p.p0 + in_piece);
                    if (!force) { CHECK(at < mm[t].size()); const Move& m = mm[t][at++]; CHECK(m.i == i && m.in_entry == in_entry && m.in_piece == in_piece && m.bytes == bytes); }
                    for (u64 b = 0; b < bytes; b++) map[p.p0 + in_piece + b]++;
                    moves_seen += !force;
                });
                if (!force) CHECK(at == mm[t].size());
            }
        }
        CHECK(end == total && map == want);                                           // each byte of each entry once, no byte outside an entry
    }
}
static void leg_shares(u64& ranges, u64& moves_seen)
{
    const u64 M = 1u << 20, P = ZPK_PIN_CHUNK;
    // 7 and 8 entries in one piece (by bytes / by count), with empty entries and gaps
    for (u64 cnt : { 1, 7, 8, 9 }) {
        std::vector<u64> offs, lens;
        u64 pos = 300;
        for (u64 i = 0; i < cnt; i++) { offs.push_back(pos); lens.push_back(i == 3 ? 0 : M + 4097 * i); pos += lens.back() + (i % 2 ? 256 : 0); }
        run_range(offs, lens, pos + 77, moves_seen); ranges++;
    }
    // a piece of exactly 4 MiB and of one byte less (the last piece of a range): four threads, one thread
    for (u64 total : { P + 4 * M, P + 4 * M - 1, 4 * M, 4 * M - 1 }) {
        run_range({ 0, total / 2 }, { total / 2, total - total / 2 }, total, moves_seen); ranges++;
        std::vector<u64> offs, lens;
        for (u64 i = 0; i < 40; i++) { offs.push_back(total / 40 * i); lens.push_back(total / 40 - (i % 3)); }
        run_range(offs, lens, total, moves_seen); ranges++;
    }
    // entries that straddle p0 and p1: one over three pieces, one that ends exactly at a boundary, one that starts there
    run_range({ 5, P - 1000, 2 * P + 4096, 2 * P + 4096 + 10 }, { P - 1005 - 1000, P + 1000 + 4096, 10, 5000 }, 2 * P + 20000, moves_seen); ranges++;
    run_range({ 0, P, P + 1 }, { P, 1, 2 * M }, P + 3 * M, moves_seen); ranges++;
    for (int it = 0; it < 8; it++) {                                                  // random ranges of up to two pieces
        const u64 n = it % 3 == 0 ? 1 + rnd() % 7 : 8 + rnd() % 3000, total_want = (1 + rnd() % 44) * M + rnd() % 5000;
        std::vector<u64> offs, lens;
        u64 pos = rnd() % 3 ? 0 : rnd() % 9000;
        for (u64 i = 0; i < n; i++) {
            const u64 l = rnd() % 5 == 0 ? 0 : rnd() % (2 * total_want / n + 1);
            offs.push_back(pos); lens.push_back(l);
            pos += l + (rnd() % 4 == 0 ? rnd() % 3000 : 0);
        }
        run_range(offs, lens, pos + rnd() % 2, moves_seen); ranges++;
    }
}

// ================================================================ the groups ===================================================================
static void leg_groups(u64& batches, u64& groups, u64& src_only_groups)
{
    for (int it = 0; it < 1500; it++) {
        const bool none = it % 2 == 0;
        const u64 n = 1 + rnd() % 40;
        std::vector<zpk_decode_desc> desc(n);
        std::vector<BigEntry> be;
        std::vector<BigSub> subs;
        for (u64 i = 0; i < n; i++) {
            zpk_decode_desc& d = desc[i];
            d = zpk_decode_desc{ rnd() % (1u << 30), 0, 0, rnd(), 0, 0, (u32)(rnd() % 3), 0 };
            d.uncomp_size = rnd() % 6 == 0 ? (1ull << 30) + rnd() % (3ull << 30) : (256u << 10) + rnd() % (8u << 20);     // (what dec_big_candidate lets through: at most 4 GiB)
            if (d.uncomp_size > ZPK_HOST_CHUNK_BYTES) d.uncomp_size = ZPK_HOST_CHUNK_BYTES;
            d.comp_size = d.method == ZPK_METHOD_NONE ? d.uncomp_size : 1000 + d.uncomp_size / (2 + rnd() % 5);
            d.dst_capacity = d.uncomp_size + rnd() % 3;
            if (rnd() % 4 == 0) continue;                                             // not every entry is one of these
            const u64 nsub = 1 + rnd() % 9, s0 = subs.size();
            for (u64 f = 0; f < nsub; f++) subs.push_back(BigSub{ d.comp_size * f / nsub, d.comp_size * (f + 1) / nsub - d.comp_size * f / nsub, d.uncomp_size * f / nsub, d.uncomp_size * (f + 1) / nsub - d.uncomp_size * f / nsub });
            be.push_back(BigEntry{ i, s0, nsub });
        }
        for (u64 g0 = 0; g0 < be.size(); ) {
            const u64 g1 = host_group_cut(desc.data(), be.data(), be.size(), g0, none);
            CHECK(g1 == model_group_cut(desc.data(), be, g0, none) && g1 > g0 && g1 <= be.size());
            const u64 ng = g1 - g0;
            std::vector<u64> coff(ng + 2, 0xA5), ooff(ng + 2, 0xA5);
            std::vector<StoredSpanRow> spans(ng);
            std::vector<zpk_decode_desc> hd;
            const HostGroup G = host_group_layout(desc.data(), be.data(), g0, g1, subs.data(), none, coff.data(), ooff.data(), spans.data(), hd);
            const ModelGroup Mg = model_group(desc.data(), be.data(), g0, g1, subs, none);
            CHECK(G.src_only == Mg.src_only && G.nsub == Mg.nsub && G.ct == Mg.ct && G.ot == Mg.ot && G.part_blocks == Mg.part_blocks && G.zstd == Mg.has_zstd && G.lz4 == Mg.has_lz4);
            CHECK(hd.size() == G.nsub && coff[ng + 1] == 0xA5 && ooff[ng + 1] == 0xA5);
            for (u64 k = 0; k <= ng; k++) CHECK(coff[k] == Mg.coff[k] && ooff[k] == Mg.ooff[k]);
            for (u64 k = 0; k < ng; k++) CHECK(spans[k].off == Mg.spans[k].off && spans[k].len == Mg.spans[k].len && spans[k].part_base == Mg.spans[k].part_base);
            for (u64 j = 0; j < G.nsub; j++) CHECK(same(hd[j], Mg.hd[j]));
            // ---- properties ----
            u64 j = 0, parts = 0, out = 0;
            for (u64 k = 0; k < ng; k++) {
                const zpk_decode_desc& d = desc[be[g0 + k].idx];
                CHECK(coff[k] % 256 == 0 && ooff[k] % 256 == 0 && coff[k + 1] >= coff[k] + d.comp_size && (G.src_only ? ooff[k + 1] == 0 : ooff[k + 1] >= ooff[k] + d.uncomp_size));
                CHECK(spans[k].len == d.uncomp_size && spans[k].part_base == parts && parts % ZPK_SPAN_GROUP == 0 && spans[k].off == (G.src_only ? coff[k] : ooff[k]));
                parts += xxh3_span_blocks(d.uncomp_size);
                if (none) CHECK((d.method == ZPK_METHOD_NONE) == G.src_only);         // the kinds apart
                for (u64 f = 0; f < be[g0 + k].nsub && !G.src_only; f++, j++) {
                    const zpk_decode_desc& x = hd[j];
                    CHECK(x.src_offset >= coff[k] && x.src_offset + x.comp_size <= coff[k] + d.comp_size && x.dst_offset >= ooff[k] && x.dst_offset + x.uncomp_size <= ooff[k] + d.uncomp_size);
                    CHECK(x.dst_capacity == x.uncomp_size && x.method == d.method && x.flags == ZPK_DF_SKIP_HASH);
                }
                if (k) CHECK(out <= ZPK_HOST_CHUNK_BYTES);                             // all but the first joined a group that had room
                out += d.uncomp_size;
            }
            CHECK(j == G.nsub && parts == G.part_blocks && (!G.src_only || (G.nsub == 0 && G.ot == 0)));
            src_only_groups += G.src_only; groups++;
            g0 = g1;
        }
        batches++;
    }
}

// ================================================================ the small rules ==============================================================
// the distinct "rc" values of tests/golden/status_cases.json (the file is read as text: every `"rc": N`)
static std::set<int> golden_statuses()
{
    std::set<int> out;
    FILE* f = fopen("tests/golden/status_cases.json", "rb");
    CHECK(f != nullptr);
    std::string text;
    char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got);
    fclose(f);
    for (size_t at = text.find("\"rc\":"); at != std::string::npos; at = text.find("\"rc\":", at + 1)) out.insert(atoi(text.c_str() + at + 5));
    return out;
}
static void leg_small_rules(size_t& statuses)
{
    u64 a = 5; sat_add(a, 7); CHECK(a == 12);
    a = ~0ull - 3; sat_add(a, 3); CHECK(a == ~0ull); sat_add(a, 0); CHECK(a == ~0ull);
    a = ~0ull - 3; sat_add(a, 4); CHECK(a == ~0ull); sat_add(a, ~0ull); CHECK(a == ~0ull);
    a = 0; sat_add(a, ~0ull); CHECK(a == ~0ull);
    zpk_decode_desc d = {}; d.dst_capacity = 100;
    zpk_decode_result r = {};
    for (u64 p : { 0, 99, 100 }) { r.produced = p; CHECK(host_delivered(d, r) == p); }
    for (u64 p : { (u64)101, (u64)~0ull }) { r.produced = p; CHECK(host_delivered(d, r) == 100); }
    // dense: more than one entry, something produced, at least half of the slots' bytes
    CHECK(!host_deliver_dense(1, 100, 100) && !host_deliver_dense(2, 0, 0) && !host_deliver_dense(2, 0, 100) && host_deliver_dense(2, 50, 100) && !host_deliver_dense(2, 49, 100) &&
          host_deliver_dense(2, 100, 100) && host_deliver_dense(1000, 1, 2) && !host_deliver_dense(1000, 1, 3));
    // a short decode: every status of the golden cases and those next to the two that count; then each other clause, failed alone
    std::set<int> st = golden_statuses();
    CHECK(st.count(0) && st.count(15) && st.size() >= 6);
    statuses = st.size();
    for (int s : { -1, 1, 14, 16, 255 }) st.insert(s);
    d = zpk_decode_desc{ 0, 10, 100, 0, 0, 100, ZPK_METHOD_LZ4, 0 };
    r.produced = 60;
    for (int s : st) { r.status = s; CHECK(host_short_decode(d, r) == (s == DEC_R_OK || s == DEC_R_FILE_HASH_MISMATCH)); }
    r.status = DEC_R_FILE_HASH_MISMATCH;
    zpk_decode_desc x = d; zpk_decode_result y = r;
    CHECK(host_short_decode(x, y));
    y.produced = 99; CHECK(host_short_decode(x, y)); y.produced = 100; CHECK(!host_short_decode(x, y)); y.produced = 101; CHECK(!host_short_decode(x, y)); y = r;
    x.dst_capacity = 99; CHECK(!host_short_decode(x, y)); x.dst_capacity = 101; CHECK(host_short_decode(x, y)); x = d;
    x.comp_size = 0; CHECK(!host_short_decode(x, y)); x = d;
    x.method = ZPK_METHOD_NONE; CHECK(!host_short_decode(x, y)); x.method = ZPK_METHOD_ZSTD; CHECK(host_short_decode(x, y));
    CHECK(ZPK_SRC_READ_SLACK < ZPK_SRC_SLACK && ZPK_PIN_CHUNK % 4096 == 0 && ZPK_SCATTER_THREADS >= 1);
}

int main()
{
    u64 a = 0, b = 0, c = 0;
    leg_cut_and_image(a, b, c);
    printf("cut: %llu batches, %llu sub-batches as the earlier loop cut them, 0 skipped; they partition the batch, slots at multiples of 256, only a single entry exceeds its chunk; "
           "a saturated slot goes alone and is refused\n", (unsigned long long)a, (unsigned long long)b);
    printf("image: %llu sub-batches sparse; every gathered layout as the earlier block, packed payloads disjoint in batch order up to the pad byte, they pass the offset guard and no other entry does\n",
           (unsigned long long)c);
    a = b = 0;
    leg_pieces(a, b);
    printf("pieces: %llu sub-batches as the earlier loop, %llu taken: pieces partition entries and output, spans inside the staged range, at most 64, none below its minimum; "
           "5 refusals reached\n", (unsigned long long)a, (unsigned long long)b);
    a = b = 0;
    leg_shares(a, b);
    printf("shares: %llu ranges, %llu moves as the earlier lambda; with 1 and 4 threads every byte of every entry moved once, none outside\n", (unsigned long long)a, (unsigned long long)b);
    a = b = c = 0;
    leg_groups(a, b, c);
    printf("groups: %llu batches, %llu groups as the earlier loops, %llu over the source alone: frames inside their entries, spans by xxh3_span_blocks\n",
           (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
    size_t s = 0;
    leg_small_rules(s);
    printf("rules: sat_add, host_delivered, host_deliver_dense as tables; host_short_decode over %llu golden status values: 0 and 15 alone\n", (unsigned long long)s);
    return 0;
}
