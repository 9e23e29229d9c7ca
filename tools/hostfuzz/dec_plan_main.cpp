// zpack_amd/csrc/dec_plan.h, the header the codec compiles, under ASan + UBSan: which large entries may leave the one-wave path (every
// guard failed once next to the last value that passes it, the three methods and an unknown one, the window of sizes, the slot test),
// agreement with stored_span_takes for stored entries, the chooser against decisions RECORDED from the function it replaced, the staging
// layout of k_big_walk, the hash verdict as a table.  Built and run by tools/hostfuzz/run_dec_plan.sh
//   dec_plan --dump-batches   prints the chooser's batches as text (one line per batch: n, then method:comp:uncomp per entry, then the
//                             candidates) — what a build of an older pj_choose reads to produce the table EXPECT below
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "dec_plan.h"
#include "stored_plan.h"
using namespace zpk;

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static const u64 ARCHIVE = (1ull << 33) + 4096, DST = (1ull << 33) + 8192, SPLIT = 256u << 10;

static zpk_decode_desc good(u32 method, u64 len)
{
    zpk_decode_desc d; memset(&d, 0, sizeof(d));
    d.src_offset = 10; d.comp_size = len; d.uncomp_size = len; d.expect_hash = 0x1122334455667788ull;
    d.dst_offset = 257; d.dst_capacity = len; d.method = method;
    return d;
}
// the rules, stated once more
static bool want_host(const zpk_decode_desc& d, u64 archive, u64 split)
{
    return split != ~0ull && d.uncomp_size >= split && d.uncomp_size <= (4ull << 30) && d.method <= 2 &&
           d.comp_size != 0 && d.src_offset <= archive && d.comp_size < archive - d.src_offset && d.dst_capacity >= d.uncomp_size;
}
static bool want_device(const zpk_decode_desc& d, u64 archive, u64 dst, u64 split)
{
    return want_host(d, archive, split) && (d.method == 1 || d.method == 2) && d.dst_offset <= dst && d.uncomp_size <= dst - d.dst_offset;
}
static bool want_stored(const zpk_decode_desc& d, u64 archive, u64 dst, u64 threshold)
{
    const u64 least = threshold > 1025 ? threshold : 1025;
    return d.method == 0 && d.comp_size != 0 && d.dst_capacity >= d.uncomp_size && d.src_offset <= archive && d.comp_size < archive - d.src_offset &&
           d.uncomp_size <= d.comp_size && d.dst_offset <= dst && d.uncomp_size <= dst - d.dst_offset && d.uncomp_size >= least;
}

// ---- the chooser's batches ---------------------------------------------------------------------------------------------------------------
struct Batch { std::vector<zpk_decode_desc> desc; std::vector<u64> cand; };
static const u64 KiB = 1ull << 10, MiB = 1ull << 20, GiB = 1ull << 30;
static void add(Batch& b, u32 method, u64 uncomp, u64 comp, bool cand)
{
    zpk_decode_desc d = good(method, uncomp); d.comp_size = comp;
    if (cand) b.cand.push_back(b.desc.size());
    b.desc.push_back(d);
}
static u64 at_ratio(u64 uncomp) { return uncomp - uncomp / 16; }                   // the least comp_size that counts as "did not compress"
static std::vector<Batch> make_batches()
{
    std::vector<Batch> v;
    const u32 Z = ZPK_METHOD_ZSTD, L = ZPK_METHOD_LZ4, N = ZPK_METHOD_NONE;
    // a single candidate, alone in its batch: 256 KiB .. 4 GiB, both methods
    for (u32 m : { L, Z }) for (u64 s : { 256 * KiB, 4 * MiB, 4 * GiB }) { Batch b; add(b, m, s, s / 2, true); v.push_back(b); }
    // ... that did not compress: both sides of the 1/16 ratio
    for (u32 m : { L, Z }) for (u64 off : { 0ull, 1ull }) { Batch b; add(b, m, 4 * MiB, at_ratio(4 * MiB) - off, true); v.push_back(b); }
    // the shapes of profiles/r15: 64 x 4 MiB and 16 x 16 MiB, all-LZ4, all-Zstandard, mixed
    for (int shape = 0; shape < 2; shape++) for (int mix = 0; mix < 3; mix++) {
        Batch b;
        const u64 cnt = shape ? 16 : 64, s = shape ? 16 * MiB : 4 * MiB;
        for (u64 i = 0; i < cnt; i++) add(b, mix == 0 ? L : mix == 1 ? Z : (i & 1 ? Z : L), s, s * 2 / 5, true);
        v.push_back(b);
    }
    { Batch b; for (int i = 0; i < 100; i++) add(b, L, 3 * MiB, MiB, true); v.push_back(b); }                        // a hundred 3 MiB entries
    { Batch b; add(b, L, 256 * MiB, 100 * MiB, true); for (int i = 0; i < 63; i++) add(b, L, 256 * KiB, 100 * KiB, true); v.push_back(b); }
    { Batch b; for (int i = 0; i < 40; i++) add(b, L, 64 * KiB - 1, 20 * KiB, false); add(b, Z, 256 * MiB, 90 * MiB, true); v.push_back(b); }
    // a non-candidate longer (by one wave) than every candidate; one that does not count (stored, or below 64 KiB) and the least that does
    { Batch b; for (int i = 0; i < 4; i++) add(b, L, MiB, MiB / 3, true); add(b, Z, 8 * MiB, 3 * MiB, false); v.push_back(b); }
    { Batch b; add(b, L, 64 * MiB, 20 * MiB, false); for (int i = 0; i < 4; i++) add(b, L, MiB, MiB / 3, true); v.push_back(b); }
    { Batch b; for (int i = 0; i < 4; i++) add(b, L, MiB, MiB / 3, true); add(b, N, GiB, GiB, false); v.push_back(b); }
    { Batch b; for (int i = 0; i < 4; i++) add(b, Z, MiB, MiB / 3, true); add(b, Z, 64 * KiB - 1, 1000, false); v.push_back(b); }
    { Batch b; for (int i = 0; i < 4; i++) add(b, Z, MiB, MiB / 3, true); add(b, Z, 64 * KiB, 1000, false); v.push_back(b); }
    { Batch b; for (int i = 0; i < 6; i++) add(b, L, 8 * MiB, 2 * MiB, true); add(b, Z, 2 * MiB, MiB / 2, false); v.push_back(b); }
    // ties in wave_ms: equal entries, more of them than an insertion sort takes at once, alone and between others
    { Batch b; for (int i = 0; i < 40; i++) add(b, L, (1 + (u64)(i % 4)) * MiB, 300 * KiB, true); v.push_back(b); }
    { Batch b; for (int i = 0; i < 17; i++) add(b, Z, 2 * MiB, MiB, true); add(b, Z, 5 * MiB, MiB, true); v.push_back(b); }
    { Batch b; for (int i = 0; i < 33; i++) add(b, i % 3 == 0 ? Z : L, 2 * MiB, MiB, i % 5 != 0); v.push_back(b); }
    // the sizes 256 KiB .. 4 GiB, eight candidates and two others each
    for (u32 m : { L, Z }) for (u64 s : { 256 * KiB, MiB, 16 * MiB, 256 * MiB, GiB, 4 * GiB }) {
        Batch b;
        for (int i = 0; i < 8; i++) add(b, m, s - (u64)i * 4096, s / 3, true);
        add(b, m == L ? Z : L, 512 * KiB, 100 * KiB, false); add(b, m, 100 * KiB, 30 * KiB, false);
        v.push_back(b);
    }
    // both methods, both sides of the ratio, in one batch
    { Batch b;
      for (int i = 0; i < 4; i++) { add(b, L, 64 * MiB, at_ratio(64 * MiB), true); add(b, L, 8 * MiB, 3 * MiB, true); }
      for (int i = 0; i < 2; i++) add(b, Z, 64 * MiB, 64 * MiB, true);
      for (int i = 0; i < 6; i++) add(b, Z, 2 * MiB, at_ratio(2 * MiB) - 1, true);
      v.push_back(b); }
    // ascending and descending sizes
    { Batch b; for (int i = 0; i < 12; i++) add(b, L, (256 * KiB) << i, (100 * KiB) << i, true); v.push_back(b); }
    { Batch b; for (int i = 11; i >= 0; i--) add(b, i & 1 ? Z : L, (256 * KiB) << i, (100 * KiB) << i, true); v.push_back(b); }
    // three drawn batches (a fixed generator)
    u64 x = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { x = x * 6364136223846793005ull + 1442695040888963407ull; return x >> 33; };
    for (u64 cnt : { 50ull, 200ull, 200ull }) {
        Batch b;
        for (u64 i = 0; i < cnt; i++) {
            const u64 s = (64 * KiB) << (next() % 13), r = next() % 18;            // 64 KiB .. 256 MiB; comp = s * r / 16: both sides of the ratio
            const u32 m = (u32)(next() % 3);
            add(b, m, s, r == 0 ? 1 : s / 16 * r, m != N && s >= 256 * KiB && next() % 4 != 0);
        }
        v.push_back(b);
    }
    { Batch b; for (int i = 0; i < 5; i++) add(b, L, 4 * MiB, MiB, false); v.push_back(b); }                         // no candidate
    return v;
}

// The positions dec_choose must return, batch by batch.  RECORDED: the batches above (--dump-batches) were run through pj_choose as it
// stood in zpk_codec.hip before dec_plan.h existed (its body copied into a stand-alone program with a PjEntry that carries only idx);
// each kept entry is given by its position in the batch's candidate list, in run order.  Never regenerate this from dec_choose.
static const char* const EXPECT[] = {
    "0",
    "0",
    "0",
    "0",
    "0",
    "0",
    "0",
    "0",
    "0",
    "0",
    "48,33",
    "48,33",
    "43,23",
    "0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15",
    "0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15",
    "1,3,5,7,9,11,13,15,0,2,4,6,8,10,12,14",
    "62,74",
    "0,47,48,46",
    "0",
    "0,1,2,3",
    "0,1,2,3",
    "0,1,2,3",
    "0,1,2,3",
    "0,1,2,3",
    "0,1,2,3,4",
    "39,27",
    "17,9",
    "2",
    "0,1",
    "0,1",
    "0,1,2,3,4,5,6,7",
    "0,1,2,3,4,5,6,7",
    "0,1,2,3,4,5,6,7",
    "0,1,2,3,4,5,6,7",
    "",
    "",
    "0,1,2,3,4,5,6,7",
    "0,1,2,3,4,5,6,7",
    "0,1,2,3,4,5,6,7",
    "0,1,2,3,4,5,6,7",
    "8,9,10,11,12,13,14,15,0,2,4,6,1,3,5,7",
    "11,10,9,8,7,6,5,4,3,2,1,0",
    "0,2,1,4,3,6,5,8,7,10,9,11",
    "12,8,4,13,6,17,5,14,16,11,3,0,10,7,15,1,18,2,9",
    "71,26,75,66,36,52,22,17,8,37,45,35,19,63,43,25,34,2,30,48,10,7,18,6,51,14,83,78,81,31,58,41,62,32,29,64,15,13,0,61,1,44,28,79,16,46,49,38,68,21,57,82,40,11,20,56,4,77,69,5,74,72,12,76,59,53,54,67,55,47,80,9,33,50,70,24,65,27,23,60,73,42,39,3",
    "43,23,19,68,31,49,61,69,10,59,72,57,52,6,78,9,20,51,0,11,22,32,1,27,39,25,24,28,18,45,60,54,33,53,65,75,5,21,62,56,50,47,37,73,79,4,48,74,70,76,38,64,42,71,58,77,66,67,41,15,36,55,14,46,17,29,13,16,7,80,35,8,2,30,26,40,44,63,12,34,3,81",
    "",
};

static std::string join(const std::vector<u64>& v)
{
    std::string s;
    for (size_t k = 0; k < v.size(); k++) { s += std::to_string((unsigned long long)v[k]); if (k + 1 < v.size()) s += ","; }
    return s;
}

int main(int argc, char** argv)
{
    const std::vector<Batch> batches = make_batches();
    if (argc > 1 && !strcmp(argv[1], "--dump-batches")) {
        for (const Batch& b : batches) {
            printf("%llu", (unsigned long long)b.desc.size());
            for (const zpk_decode_desc& d : b.desc) printf(" %u:%llu:%llu", d.method, (unsigned long long)d.comp_size, (unsigned long long)d.uncomp_size);
            printf(" | %llu", (unsigned long long)b.cand.size());
            for (u64 i : b.cand) printf(" %llu", (unsigned long long)i);
            printf("\n");
        }
        return 0;
    }

    // ---- the candidate rule ----
    {
        u64 rows = 0, taken = 0, failed = 0;
        auto row = [&](const zpk_decode_desc& d, u64 archive, u64 dst, u64 split, bool host, bool device) {
            CHECK(dec_big_candidate(d, archive, split) == host && host == want_host(d, archive, split));
            CHECK(dec_big_candidate_device(d, archive, dst, split) == device && device == want_device(d, archive, dst, split));
            if (d.method == ZPK_METHOD_NONE) {                                           // the stored entries: the same predicates decide
                const bool stored = stored_span_takes(d, archive, dst, split);
                CHECK(stored == want_stored(d, archive, dst, split));
                CHECK(stored == (dec_guards_pass(d, archive) && d.uncomp_size <= d.comp_size && dec_slot_in_dst(d, dst) && d.uncomp_size >= (split > 1025 ? split : 1025)));
                if (d.uncomp_size <= ZPK_HOST_CHUNK_BYTES && d.uncomp_size <= d.comp_size && split > 1025) CHECK(stored == (host && dec_slot_in_dst(d, dst)));
            }
            rows++; taken += host; failed += !host;
        };
        const u64 S = 300 * KiB;
        for (u32 m : { (u32)ZPK_METHOD_NONE, (u32)ZPK_METHOD_ZSTD, (u32)ZPK_METHOD_LZ4 }) {
            const bool dev = m != ZPK_METHOD_NONE;
            zpk_decode_desc d = good(m, S);
            row(d, ARCHIVE, DST, SPLIT, true, dev);
            d = good(m, S); d.comp_size = 0; row(d, ARCHIVE, DST, SPLIT, false, false);                                // :328
            d = good(m, S); d.comp_size = 1; row(d, ARCHIVE, DST, SPLIT, true, dev);
            d = good(m, S); d.src_offset = ARCHIVE; row(d, ARCHIVE, DST, SPLIT, false, false);                         // :331, the offset
            d = good(m, S); d.src_offset = ARCHIVE + 1; row(d, ARCHIVE, DST, SPLIT, false, false);
            d = good(m, S); d.src_offset = ~0ull - 5; row(d, ARCHIVE, DST, SPLIT, false, false);                       // (no wrap)
            d = good(m, S); d.src_offset = ARCHIVE - S; row(d, ARCHIVE, DST, SPLIT, false, false);                     // comp_size == archive_size - src_offset: strict
            CHECK(dec_src_in_image(d, ARCHIVE) && !dec_src_passes(d, ARCHIVE));                                        // ... its bytes can be staged all the same
            d = good(m, S); d.src_offset = ARCHIVE - S - 1; row(d, ARCHIVE, DST, SPLIT, true, dev);                    // ... one below
            CHECK(dec_src_in_image(d, ARCHIVE) && dec_src_passes(d, ARCHIVE));
            d = good(m, S); d.src_offset = ARCHIVE - S + 1; row(d, ARCHIVE, DST, SPLIT, false, false);
            CHECK(!dec_src_in_image(d, ARCHIVE) && !dec_src_passes(d, ARCHIVE));
            d = good(m, S); d.comp_size = ~0ull; row(d, ARCHIVE, DST, SPLIT, false, false);
            d = good(m, S); d.dst_capacity = S - 1; row(d, ARCHIVE, DST, SPLIT, false, false);                         // :329
            d = good(m, S); d.dst_capacity = S + 1; row(d, ARCHIVE, DST, SPLIT, true, dev);
            for (u64 s : { SPLIT - 1, SPLIT, (u64)ZPK_HOST_CHUNK_BYTES, (u64)ZPK_HOST_CHUNK_BYTES + 1 }) {                // the window
                const bool in = s >= SPLIT && s <= ZPK_HOST_CHUNK_BYTES;
                d = good(m, s); row(d, ARCHIVE, DST, SPLIT, in, in && dev);
            }
            d = good(m, S); row(d, ARCHIVE, DST, ~0ull, false, false);                                                 // the option is off
            d = good(m, ~0ull); d.comp_size = S; row(d, ~0ull, ~0ull, ~0ull, false, false);
            d = good(m, S); row(d, ARCHIVE, DST, S, true, dev); row(d, ARCHIVE, DST, S + 1, false, false);
            // the slot test: the device forms alone
            d = good(m, S); d.dst_offset = DST - S; row(d, ARCHIVE, DST, SPLIT, true, dev);
            d = good(m, S); d.dst_offset = DST - S + 1; row(d, ARCHIVE, DST, SPLIT, true, false);                      // one byte of overhang
            d = good(m, S); d.dst_offset = DST; row(d, ARCHIVE, DST, SPLIT, true, false);
            d = good(m, S); d.dst_offset = DST + 1; row(d, ARCHIVE, DST, SPLIT, true, false);
            d = good(m, S); d.dst_offset = ~0ull; row(d, ARCHIVE, DST, SPLIT, true, false);                            // (no wrap)
            d = good(m, S); d.flags = ZPK_DF_SKIP_HASH | ZPK_DF_GENERAL; row(d, ARCHIVE, DST, SPLIT, true, dev);       // the flags do not matter
        }
        for (u32 m : { 3u, 0x80000002u, ~0u }) { zpk_decode_desc d = good(m, S); row(d, ARCHIVE, DST, SPLIT, false, false); }   // an unknown method
        { zpk_decode_desc d = good(ZPK_METHOD_NONE, 0); CHECK(!dec_has_payload(d) && dec_capacity_holds(d) && !dec_guards_pass(d, ARCHIVE)); }
        CHECK(ZPK_DEC_SPLIT_MIN_DEFAULT == SPLIT && ZPK_HOST_CHUNK_BYTES == 4 * GiB);
        printf("rule: %llu rows, %llu candidates of the host form, %llu not: exactly by the rule, the device forms and stored_span_takes agree\n",
               (unsigned long long)rows, (unsigned long long)taken, (unsigned long long)failed);
    }

    // ---- the chooser ----
    {
        CHECK(batches.size() == sizeof(EXPECT) / sizeof(EXPECT[0]) && batches.size() >= 40);
        u64 cands = 0, kept = 0;
        for (size_t b = 0; b < batches.size(); b++) {
            const Batch& B = batches[b];
            const std::vector<u64> got = dec_choose(B.desc.data(), B.desc.size(), B.cand.data(), B.cand.size());
            if (join(got) != EXPECT[b]) { printf("FAILED batch %zu: chose [%s], recorded [%s]\n", b, join(got).c_str(), EXPECT[b]); exit(1); }
            std::vector<u8> seen(B.cand.size(), 0);
            for (u64 k : got) { CHECK(k < B.cand.size() && !seen[k]); seen[k] = 1; }
            cands += B.cand.size(); kept += got.size();
        }
        printf("choose: %zu batches, %llu candidates, %llu kept: every batch as recorded, order included\n", batches.size(),
               (unsigned long long)cands, (unsigned long long)kept);
    }

    // ---- the layout ----
    {
        std::vector<zpk_decode_desc> desc;
        std::vector<u64> cand;
        const u64 sizes[] = { 256 * KiB, 256 * KiB + 1, 65536 * 5 - 1, 3 * MiB + 17, 128 * MiB, 4 * GiB };
        for (u64 s : sizes) for (u32 m : { (u32)ZPK_METHOD_LZ4, (u32)ZPK_METHOD_ZSTD }) {
            desc.push_back(good(ZPK_METHOD_NONE, 1000));                                 // (entries between the candidates)
            zpk_decode_desc d = good(m, s); d.src_offset = 1000 + desc.size(); d.comp_size = s / 2 + 3;
            cand.push_back(desc.size()); desc.push_back(d);
        }
        for (u64 nc : { (u64)cand.size(), (u64)1, (u64)7 }) {
            std::vector<BigWalkItem> items(3);
            const BigWalkLayout L = dec_walk_layout(desc.data(), cand.data(), nc, items);
            CHECK(items.size() == nc && L.rec_off == ((nc * sizeof(BigWalkItem) + 255) & ~255ull) && L.rec_off >= nc * sizeof(BigWalkItem));
            u64 end = L.rec_off + nc * sizeof(BigWalkRec);
            for (u64 k = 0; k < nc; k++) {
                const zpk_decode_desc& d = desc[cand[k]];
                const BigWalkItem& it = items[k];
                CHECK(it.src_off == d.src_offset && it.comp == d.comp_size && it.uncomp == d.uncomp_size && it.method == d.method);
                CHECK(it.cap == (d.method == ZPK_METHOD_LZ4 ? walk_lz4_capacity(d.uncomp_size) : walk_zstd_capacity(d.uncomp_size)));
                CHECK(it.tab_off % 16 == 0 && it.tab_off >= end);                        // 16-aligned, ascending, behind the records, disjoint
                end = it.tab_off + (u64)it.cap * (d.method == ZPK_METHOD_LZ4 ? sizeof(PjBlock) : sizeof(ZpjBlock));
                CHECK(k + 1 < nc || (L.total >= end && L.total - end < 16));             // total = the end of the last table
            }
        }
        std::vector<BigWalkItem> none(2);
        const BigWalkLayout L0 = dec_walk_layout(desc.data(), cand.data(), 0, none);
        CHECK(none.empty() && L0.rec_off == 0 && L0.total == 0);                         // no candidate: no walk, nothing staged
        CHECK(sizeof(BigWalkItem) == 40 && sizeof(BigWalkRec) == 32);
        printf("layout: %zu candidates: tables 16-aligned, ascending and disjoint, capacities those of the walkers, total the end of the last table; none: no walk\n", cand.size());
    }

    // ---- the verdict ----
    {
        zpk_decode_desc d = good(ZPK_METHOD_LZ4, 300 * KiB); d.comp_size = 1000;
        zpk_decode_result r = dec_hash_verdict(d, d.expect_hash);
        CHECK(r.status == 0 && r.detail == 0 && r.produced == d.uncomp_size && r.hash == d.expect_hash);
        r = dec_hash_verdict(d, d.expect_hash ^ 1);
        CHECK(r.status == 15 && r.detail == 0 && r.produced == d.uncomp_size && r.hash == (d.expect_hash ^ 1));
        d.flags = ZPK_DF_SKIP_HASH;
        r = dec_hash_verdict(d, d.expect_hash ^ 1);
        CHECK(r.status == 0 && r.detail == 0 && r.produced == d.uncomp_size && r.hash == (d.expect_hash ^ 1));
        d.flags = ZPK_DF_GENERAL;
        r = dec_hash_verdict(d, d.expect_hash ^ 1);
        CHECK(r.status == 15 && r.produced == d.uncomp_size);
        r = stored_span_verdict(d, d.expect_hash ^ 1);
        CHECK(r.status == 15 && r.detail == 0 && r.produced == d.uncomp_size && r.hash == (d.expect_hash ^ 1));
        printf("verdict: OK, hash mismatch, hash mismatch skipped; detail 0, produced = uncomp_size, the hash as computed\n");
    }
    return 0;
}
