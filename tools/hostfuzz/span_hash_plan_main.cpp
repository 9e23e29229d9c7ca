// zpack_amd/csrc/span_hash_plan.h, the header the codec compiles, under ASan + UBSan: which spans one wave hashes and which the whole chip,
// the two tables, the partial-sum layout and the launches of k_span_hash and the chip-wide pair.  Every row and every group is walked the
// way the kernels walk it (span_hash.h, xxh3_span.h: 64 lanes x 16 bytes per 1 KiB block; the stripes and the last stripe of
// Xxh3Wave::finish) against a row of real bytes with guard bytes around it:
//   every byte of a row is covered once by the block and stripe loads, the last stripe closes the row as the hash defines it;
//   no load leaves the row;
//   the partial-sum slots of different rows do not overlap, and every launch split reaches every row and group once.
// `--pin` prints the plan's decisions at the sizes tests/test_span_hash_plan_cpu.py pins.  Built and run by tools/hostfuzz/run_span_hash_plan.sh
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "span_hash_plan.h"
using namespace zpk;

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static const u64 GUARD = 96;

// a 16-byte load at byte `at` of the row: inside it, and counted
static void load16(std::vector<u8>& seen, const std::vector<u8>& mem, u64 len, u64 at)
{
    CHECK(at + 16 <= len);                                                            // no load leaves the row
    volatile u8 sink = 0;
    for (u64 k = 0; k < 16; k++) { sink = sink ^ mem[GUARD + at + k]; seen[at + k]++; }   // (ASan sees the access)
}

// what Xxh3Wave::finish reads behind `done` bytes of blocks: the whole stripes, lane by lane, then the last stripe by the lanes of group 15
static void walk_finish(std::vector<u8>& seen, std::vector<u8>& last, const std::vector<u8>& mem, u64 len, const SpanHashLoads& L)
{
    const u64 done = L.blocks << 10;
    for (u32 lane = 0; lane < 64; lane++) {
        const u32 q = lane & 3, s = lane >> 2;
        if (s < L.stripes) load16(seen, mem, len, done + 16ull * lane);
        else if (s == 15) { CHECK(L.last_from + 16 * q + 16 <= len); for (u64 k = 0; k < 16; k++) last[L.last_from + 16 * q + k]++; }
    }
}

static void check_cover(const std::vector<u8>& seen, const std::vector<u8>& last, u64 len, const SpanHashLoads& L)
{
    CHECK(L.stripes < 16 && L.stripes_end < len && len - L.stripes_end <= 64 && L.last_from == len - 64);
    for (u64 i = 0; i < len; i++) {
        CHECK(seen[i] == (i < L.stripes_end ? 1 : 0));                                // blocks and stripes: every byte in front of stripes_end once, none behind
        CHECK(last[i] == (i >= L.last_from ? 1 : 0));                                 // the last stripe: [len - 64, len), so nothing between stripes_end and len is missed
    }
}

struct Counts { u64 rows = 0, wave = 0, wide = 0, groups = 0, launches = 0, bytes = 0; };

// One call's rows through the plan and the kernels' walk.  max_*: the launch limits (small ones force splits).
static void run_call(const std::vector<u64>& lens, u64 threshold, u64 max_wave_rows, u64 max_groups, u64 max_chains, Counts& C)
{
    const u64 n = lens.size();
    std::vector<std::vector<u8>> mem(n);
    for (u64 i = 0; i < n; i++) mem[i].assign(lens[i] + 2 * GUARD, (u8)(i * 37 + 11));
    std::vector<SpanHashRow> wave(n);
    std::vector<SpanHashWide> wide(n);
    std::vector<u64> kept(n);
    SpanHashPlan p = { 0, 0, 0, 0 };
    for (u64 i = 0; i < n; i++) {
        kept[i] = span_hash_emit(i, lens[i], threshold, wave.data(), wide.data(), p);                         // (addr: the row's number here)
        CHECK(kept[i] != ~0ull);
        CHECK(((kept[i] & ZPK_SPAN_HASH_WIDE_BIT) != 0) == span_hash_wide(lens[i], threshold));
    }
    CHECK(p.nwave + p.nwide == n && p.part_blocks == p.groups * ZPK_SPAN_GROUP);
    const SpanHashLayout L = span_hash_layout(p);
    CHECK(L.wide_rows == p.nwave * sizeof(SpanHashRow) && L.out == L.up_bytes && L.partial % 256 == 0 && L.partial >= L.out + n * 8 && L.bytes == L.partial + p.part_blocks * 64);
    std::vector<u8> out_written(n, 0);
    for (u64 i = 0; i < n; i++) { const u64 s = span_hash_out_slot(kept[i], p.nwave); CHECK(s < n && !out_written[s]); out_written[s] = 1; }   // one slot of `out` per row
    std::vector<std::vector<u8>> seen(n), last(n);
    for (u64 i = 0; i < n; i++) { seen[i].assign(lens[i], 0); last[i].assign(lens[i], 0); }
    // ---- k_span_hash: launch by launch, wave by wave ----
    std::vector<u8> wave_done(p.nwave, 0);
    for (u64 j = 0, nl = span_hash_launches(p.nwave, max_wave_rows); j < nl; j++, C.launches++) {
        const SpanHashLaunch W = span_hash_launch(p.nwave, j, max_wave_rows, 4);
        CHECK(W.count > 0 && W.count <= max_wave_rows && (u64)W.grid * 4 >= W.count && (u64)W.grid * 4 < W.count + 4);
        for (u64 w = W.first; w < W.first + (u64)W.grid * 4; w++) {
            if (w >= W.first + W.count) continue;                                     // (the kernel's `w >= end`)
            CHECK(w < p.nwave && !wave_done[w]);
            wave_done[w] = 1;
            const u64 i = wave[w].addr, len = wave[w].len;
            CHECK(len == lens[i] && !span_hash_wide(len, threshold));
            if (len <= 240) { for (u64 k = 0; k < len; k++) seen[i][k]++; continue; }                          // xxh3_short: inside [0, len), judged with the long rows' rule below
            const SpanHashLoads S = span_hash_loads(len);
            for (u64 b = 0; b < S.blocks; b++) for (u32 lane = 0; lane < 64; lane++) load16(seen[i], mem[i], len, (b << 10) + 16ull * lane);
            walk_finish(seen[i], last[i], mem[i], len, S);
        }
    }
    for (u64 w = 0; w < p.nwave; w++) CHECK(wave_done[w]);
    // ---- k_xxh3_partials: launch by launch, group by group; the slots each group writes ----
    std::vector<long long> slot_owner(p.part_blocks, -1);                             // partial-sum slot -> chip-wide row
    u64 groups_done = 0;
    for (u64 j = 0, nl = span_hash_launches(p.groups, max_groups); j < nl; j++, C.launches++) {
        const SpanHashLaunch G = span_hash_launch(p.groups, j, max_groups, 4);
        CHECK(G.count > 0 && G.count <= max_groups);
        const u64 end = G.first + G.count;
        for (u64 g = G.first; g < G.first + (u64)G.grid * 4; g++) {
            if (g >= end) continue;                                                   // (the kernel's `g >= ngroups`)
            const u64 k = span_hash_wide_of(wide.data(), p.nwide, g);
            const SpanHashWide& sp = wide[k];
            CHECK(sp.part_base % ZPK_SPAN_GROUP == 0 && sp.part_base / ZPK_SPAN_GROUP <= g && (k == 0 || wide[k - 1].part_base < sp.part_base));    // multiples of 64, ascending
            const u64 i = sp.off, len = sp.len;
            const SpanHashLoads S = span_hash_loads(len);
            const u64 b0 = (g - sp.part_base / ZPK_SPAN_GROUP) * ZPK_SPAN_GROUP;
            CHECK(b0 < S.blocks);                                                     // every group of the table has blocks
            const u64 nb = S.blocks - b0 < ZPK_SPAN_GROUP ? S.blocks - b0 : ZPK_SPAN_GROUP;
            for (u64 t = 0; t < nb; t++) {
                for (u32 lane = 0; lane < 64; lane++) load16(seen[i], mem[i], len, ((b0 + t) << 10) + 16ull * lane);
                const u64 slot = sp.part_base + b0 + t;
                CHECK(slot < p.part_blocks && slot_owner[slot] < 0);                  // a slot is written once, by one row
                slot_owner[slot] = (long long)k;
            }
            groups_done++;
        }
    }
    CHECK(groups_done == p.groups);
    // ---- k_xxh3_chain: one workgroup per chip-wide row; the slots it reads are its own, and all of them are there ----
    std::vector<u8> chain_done(p.nwide, 0);
    for (u64 j = 0, nl = span_hash_launches(p.nwide, max_chains); j < nl; j++, C.launches++) {
        const SpanHashLaunch K = span_hash_launch(p.nwide, j, max_chains, 1);
        CHECK(K.grid == K.count && K.count <= max_chains);
        for (u64 k = K.first; k < K.first + K.count; k++) {
            CHECK(k < p.nwide && !chain_done[k]);
            chain_done[k] = 1;
            const SpanHashWide& sp = wide[k];
            const u64 i = sp.off;
            const SpanHashLoads S = span_hash_loads(sp.len);
            CHECK(xxh3_span_blocks(sp.len) >= S.blocks && xxh3_span_blocks(sp.len) < S.blocks + ZPK_SPAN_GROUP);
            for (u64 b = 0; b < xxh3_span_blocks(sp.len); b++) CHECK(slot_owner[sp.part_base + b] == (b < S.blocks ? (long long)k : -1));
            walk_finish(seen[i], last[i], mem[i], sp.len, S);
        }
    }
    for (u64 k = 0; k < p.nwide; k++) CHECK(chain_done[k]);
    // ---- every row ----
    for (u64 i = 0; i < n; i++) {
        if (lens[i] <= 240) { for (u64 k = 0; k < lens[i]; k++) CHECK(seen[i][k] == 1); }
        else check_cover(seen[i], last[i], lens[i], span_hash_loads(lens[i]));
        C.bytes += lens[i];
    }
    C.rows += n; C.wave += p.nwave; C.wide += p.nwide; C.groups += p.groups;
}

static void pin(u64 threshold, u64 max_groups)
{
    // the split at the threshold
    for (u64 len : { threshold - 1, threshold, threshold + 1 }) printf("pin split: len %llu threshold %llu -> %s\n", (unsigned long long)len, (unsigned long long)threshold, span_hash_wide(len, threshold) ? "chip-wide" : "one wave");
    printf("pin split: len 1024 threshold 1 -> %s; len 1025 threshold 1 -> %s; len %llu threshold never -> %s\n", span_hash_wide(1024, 1) ? "chip-wide" : "one wave",
           span_hash_wide(1025, 1) ? "chip-wide" : "one wave", (unsigned long long)(1ull << 40), span_hash_wide(1ull << 40, ~0ull) ? "chip-wide" : "one wave");
    // the partial-sum bases of a mixed call
    const u64 lens[] = { threshold, 300, threshold + 65536, 0, threshold + 1025, 240, 65 * 65536 + 1 };
    std::vector<SpanHashRow> wave(7);
    std::vector<SpanHashWide> wide(7);
    SpanHashPlan p = { 0, 0, 0, 0 };
    printf("pin rows:");
    for (u64 i = 0; i < 7; i++) { const u64 k = span_hash_emit(0x1000 * (i + 1), lens[i], threshold, wave.data(), wide.data(), p); printf(" %s%llu", k & ZPK_SPAN_HASH_WIDE_BIT ? "W" : "w", (unsigned long long)(k & ~ZPK_SPAN_HASH_WIDE_BIT)); }
    printf("\npin part_base:");
    for (u64 k = 0; k < p.nwide; k++) printf(" %llu", (unsigned long long)wide[k].part_base);
    printf(" | part_blocks %llu groups %llu nwave %llu nwide %llu\n", (unsigned long long)p.part_blocks, (unsigned long long)p.groups, (unsigned long long)p.nwave, (unsigned long long)p.nwide);
    // the launches at a small group limit
    printf("pin launches of %llu groups at a limit of %llu:", (unsigned long long)p.groups, (unsigned long long)max_groups);
    for (u64 j = 0, nl = span_hash_launches(p.groups, max_groups); j < nl; j++) { const SpanHashLaunch G = span_hash_launch(p.groups, j, max_groups, 4); printf(" [%llu,+%llu) grid %u", (unsigned long long)G.first, (unsigned long long)G.count, G.grid); }
    printf("\n");
    const SpanHashLaunch whole = span_hash_launch(p.groups, 0, ZPK_SPAN_HASH_MAX_GROUPS, 4);
    printf("pin launches at the grid limit: %llu, [%llu,+%llu) grid %u\n", (unsigned long long)span_hash_launches(p.groups, ZPK_SPAN_HASH_MAX_GROUPS), (unsigned long long)whole.first, (unsigned long long)whole.count, whole.grid);
}

int main(int argc, char** argv)
{
    if (argc == 4 && strcmp(argv[1], "--pin") == 0) { pin(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10)); return 0; }
    Counts C;
    const u64 T = 4096;
    const std::vector<u64> edge = { 0, 1, 3, 4, 8, 9, 16, 17, 128, 129, 240, 241, 255, 256, 305, 1023, 1024, 1025, 1088, 1089, 2048, 2049, T - 1, T, T + 1, T + 1025,
                                    65535, 65536, 65537, 65536 + 1025, 131072, 131073, 133120 + 7, 3 * 65536 + 64 };
    // the lengths in ascending and descending order and shuffled; thresholds: a few KiB, the least, never; launch limits: whole and small
    std::vector<u64> desc(edge.rbegin(), edge.rend()), shuf = edge;
    u64 s = 12345;
    for (size_t i = shuf.size() - 1; i > 0; i--) { s = s * 6364136223846793005ull + 1442695040888963407ull; std::swap(shuf[i], shuf[(s >> 33) % (i + 1)]); }
    const std::vector<u64>* const orders[3] = { &edge, &desc, &shuf };
    const u64 thresholds[4] = { T, 1, ~0ull, 65536 };
    for (const std::vector<u64>* lens : orders)
        for (u64 thr : thresholds) {
            run_call(*lens, thr, ZPK_SPAN_HASH_MAX_WAVE_ROWS, ZPK_SPAN_HASH_MAX_GROUPS, ZPK_SPAN_HASH_MAX_CHAINS, C);
            run_call(*lens, thr, 8, 4, 3, C);                                         // small limits: several launches of each kernel
            run_call(*lens, thr, 4, 8, 1, C);
        }
    run_call(std::vector<u64>(3000, 300), T, ZPK_SPAN_HASH_MAX_WAVE_ROWS, ZPK_SPAN_HASH_MAX_GROUPS, ZPK_SPAN_HASH_MAX_CHAINS, C);      // many rows over few workgroups
    run_call(std::vector<u64>(1, 0), T, 4, 4, 1, C);
    // the tables are full at ZPK_SPAN_HASH_MAX_ROWS: nothing is written
    {
        SpanHashRow w1[1]; SpanHashWide W1[1]; memset(w1, 0xA5, sizeof(w1)); memset(W1, 0xA5, sizeof(W1));
        const SpanHashRow wb = w1[0]; const SpanHashWide Wb = W1[0];
        SpanHashPlan full = { ZPK_SPAN_HASH_MAX_ROWS - 5, 5, 64, 1 };
        CHECK(span_hash_emit(1, 2, T, w1, W1, full) == ~0ull && span_hash_emit(1, T, T, w1, W1, full) == ~0ull);
        CHECK(full.nwave == ZPK_SPAN_HASH_MAX_ROWS - 5 && full.nwide == 5 && full.part_blocks == 64 && memcmp(w1, &wb, sizeof(wb)) == 0 && memcmp(W1, &Wb, sizeof(Wb)) == 0);
    }
    printf("span hash plan: %llu rows in %llu bytes (%llu one wave, %llu chip-wide in %llu groups, %llu launches): every byte in front of the last stripe loaded once, "
           "the last stripe closes the row, no load leaves a row, one slot of partial sums per block and row, every split reaches each row and group once\n",
           (unsigned long long)C.rows, (unsigned long long)C.bytes, (unsigned long long)C.wave, (unsigned long long)C.wide, (unsigned long long)C.groups, (unsigned long long)C.launches);
    return 0;
}
