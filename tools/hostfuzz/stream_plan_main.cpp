// zpack_amd/csrc/stream_plan.h, the header the codec compiles, under ASan + UBSan: the intake rule and the go rule of the stream reader's
// bounded steps as tables (every refusal and every RESTART once next to the last value that passes), whole streams simulated without a
// GPU — synthetic LZ4 frames of block headers (lz4_stream_blocks reads nothing else) whose output sizes the harness assigns, fed in
// fixed and random windows, with the LZ4 constants and, for 128 KiB blocks and three history capacities, the Zstandard ones — and the
// two device layouts.  Built and run by tools/hostfuzz/run_stream_plan.sh
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "stream_plan.h"
using namespace zpk;

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)
static const u64 KiB = 1ull << 10, MiB = 1ull << 20;

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static u64 rnd_in(u64 lo, u64 hi) { return lo + rnd() % (hi - lo + 1); }

// ---- (a) the tables -------------------------------------------------------------------------------------------------------------------------
static void tables()
{
    const u64 MAX = ZPK_STREAM_MAX_BYTES;
    const struct { u64 comp, in_total, in_size; int rc; u64 take; } intake[] = {
        { 100, 0, 40, 0, 40 }, { 100, 60, 40, 0, 40 }, { 100, 60, 41, 0, 40 }, { 100, 99, 5, 0, 1 },      // never more than the entry still has
        { 100, 100, 40, 0, 0 }, { 100, 101, 40, 21, 0 },                                                 // comp_size below what was taken: 21, next to the last that passes
        { MAX, 0, 5, 0, 5 }, { MAX + 1, 0, 5, 10, 0 },                                                   // a size no device holds: 10, likewise
        { MAX + 1, MAX + 2, 5, 21, 0 },                                                                  // (21 is looked at first)
        { 0, 0, 5, 0, 0 }, { 100, 0, 0, 0, 0 },
    };
    u32 n_intake = 0, refused = 0;
    for (const auto& r : intake) {
        const StreamIntake it = stream_intake(r.comp, r.in_total, r.in_size);
        CHECK(it.rc == r.rc && it.take == r.take);
        n_intake++; refused += r.rc != 0;
    }
    // the pending buffer: unchanged while the bytes fit, else what is needed + 1 MiB
    CHECK(stream_pend_cap(0, 0, 0) == 0 && stream_pend_cap(0, 0, 1) == 1 + MiB && stream_pend_cap(10, 20, 10) == 20 && stream_pend_cap(10, 20, 11) == 21 + MiB);
    printf("intake: %u rows, %u refused (21 below what was taken, 10 above 2^46), never more than the entry has; the pending buffer grows by need + 1 MiB\n", n_intake, refused);

    const StreamGo W = STREAM_WAIT, R = STREAM_RUN, X = STREAM_RESTART;
    const struct { bool end; u32 nb, table, first_min; u64 f_T; bool all_in, q_is_all; StreamGo want; } go[] = {
        // the end mark: a step — unless something follows it, or the entry's bytes are not all here
        { true, 5, 64, 4, 0, true, true, R }, { true, 0, 64, 4, 700, true, true, R }, { true, 5, 64, 4, 0, true, false, X }, { true, 5, 64, 4, 0, false, true, X },
        { true, 0, 64, 2, 700, true, true, R }, { true, 1, 64, 2, 0, true, false, X }, { true, 1, 64, 2, 0, false, true, X },
        // a full table
        { false, 64, 64, 4, 700, false, false, R }, { false, 63, 64, 4, 700, false, false, W }, { false, 64, 64, 4, 700, true, true, R }, { false, 63, 64, 4, 700, true, true, X },
        { false, 64, 64, 2, 700, false, false, R }, { false, 63, 64, 2, 700, false, false, W }, { false, 63, 64, 2, 700, true, false, X },
        // the first step: from 4 (LZ4) / 2 (Zstandard) blocks on; later steps wait for the table
        { false, 4, 64, 4, 0, false, false, R }, { false, 3, 64, 4, 0, false, false, W }, { false, 3, 64, 4, 0, true, true, X }, { false, 4, 64, 4, 1, false, false, W },
        { false, 2, 64, 2, 0, false, false, R }, { false, 1, 64, 2, 0, false, false, W }, { false, 1, 64, 2, 0, true, true, X }, { false, 2, 64, 2, 1, false, false, W },
        { false, 0, 64, 4, 0, false, true, W }, { false, 0, 64, 4, 0, true, true, X },
    };
    u32 n_go = 0, cnt[3] = { 0, 0, 0 };
    for (const auto& r : go) { CHECK(stream_go(r.end, r.nb, r.table, r.first_min, r.f_T, r.all_in, r.q_is_all) == r.want); n_go++; cnt[r.want]++; }
    CHECK(F_BLOCKS == 64 && F_FIRST_MIN == 4 && FZ_BLOCKS == 64 && FZ_FIRST_MIN == 2 && F_LOOK == 12 && FZ_LOOK == 14);
    CHECK(stream_verdict(5, 5) == 0 && stream_verdict(5, 5 ^ 4) == 15);
    printf("go: %u rows, %u run, %u wait, %u RESTART: exactly by the rule; LZ4 64 / 4, Zstandard 64 / 2; verdict 0 or 15\n", n_go, cnt[R], cnt[W], cnt[X]);
}

// ---- (b) streams ---------------------------------------------------------------------------------------------------------------------------
struct Frame { std::vector<u8> bytes; std::vector<u32> word, out; u64 total, min_block; };     // per block: its header word, its output size
// blocks of block_out bytes of output (`shorts`: some in the middle are shorter), the rest in a last short one; bodies of `body_lo ..
// body_hi` bytes, every `stored_every`-th block stored
static Frame make_frame(u64 total, u32 block_out, bool shorts, u32 body_lo, u32 body_hi, u32 stored_every)
{
    Frame f; f.total = total; f.min_block = ~0ull;
    u64 left = total;
    while (left) {
        u32 out = (u32)std::min<u64>(left, block_out);
        if (shorts && out == block_out && rnd() % 5 == 0) out = (u32)rnd_in(1, block_out - 1);
        const bool stored = stored_every && f.out.size() % stored_every == stored_every - 1;
        const u32 n = stored ? std::min<u32>(out, PJ_BLOCK) : (u32)rnd_in(body_lo, body_hi);
        const u32 w = n | (stored ? 0x80000000u : 0u);
        u8 h[4]; memcpy(h, &w, 4);
        f.bytes.insert(f.bytes.end(), h, h + 4);
        f.bytes.resize(f.bytes.size() + n, (u8)0xAB);
        f.word.push_back(w); f.out.push_back(out);
        f.min_block = std::min<u64>(f.min_block, 4 + n);
        left -= out;
    }
    f.bytes.resize(f.bytes.size() + 4, 0);                          // the EndMark
    return f;
}

struct Params { u32 block_out, table, first_min; u64 cap, part_bytes; };
struct Totals { u64 streams, calls, steps, one_shot, carries, stated_bound; };

// window: bytes per call; 0: a random size in [1, 9 MiB] for every call
static void simulate(const Frame& f, const Params& P, u64 window, Totals& tot)
{
    const u64 comp = f.bytes.size(), step_max = (u64)P.table * P.block_out;
    std::vector<u8> pend; u64 pend_cap = 0;
    u64 in_total = 0, T = 0, hist = 0, ghashed = 0, next_block = 0, steps = 0;
    std::vector<u32> partial_done, chain_done;
    bool final_seen = false, one_shot_seen = false, ended = false;
    // Pending bytes: a call takes the caller's whole window and a step at most `table` blocks away, so "a step's worth + the window" bounds
    // them where a full step takes at least a window's bytes away (`stated`); in general a call that waits holds less than a step's worth
    // and no call holds more than what the last one left + its window
    const bool stated = window != 0 && window <= (u64)P.table * f.min_block;
    std::vector<PjBlock> tab(P.table);
    for (u64 call = 0; !ended; call++) {
        CHECK(call < 40000000);
        const u64 w = window ? window : (rnd() % 4 == 0 ? rnd_in(1, 9 * MiB) : rnd_in(1, 1ull << rnd_in(1, 23)));
        const u64 have = std::min<u64>(w, comp - in_total);                  // a caller never passes more than it has
        const StreamIntake it = stream_intake(comp, in_total, have);
        CHECK(it.rc == 0 && it.take == have);
        const u64 cap = stream_pend_cap(pend.size(), pend_cap, it.take);
        CHECK(cap >= pend.size() + it.take && cap >= pend_cap);
        pend_cap = cap;
        pend.insert(pend.end(), f.bytes.begin() + (long)in_total, f.bytes.begin() + (long)(in_total + it.take));
        in_total += it.take;
        const bool all_in = in_total == comp;
        if (stated) CHECK(pend.size() <= F_IN + window);
        u64 q = 0; bool end = false;
        const int found = lz4_stream_blocks(pend.data(), pend.size(), tab.data(), P.table, &q, &end);
        CHECK(found >= 0);
        const u32 nb = (u32)found;
        const StreamGo go = stream_go(end, nb, P.table, P.first_min, T, all_in, q == pend.size());
        CHECK(go != STREAM_RESTART);
        tot.calls++;
        if (go == STREAM_WAIT) { CHECK(!all_in && pend.size() <= F_IN); continue; }
        // ---- one step: its blocks are the next ones, in order ----
        u64 step_out = 0;
        for (u32 i = 0; i < nb; i++) { CHECK(next_block + i < f.word.size() && tab[i].comp_size == f.word[next_block + i]); step_out += f.out[next_block + i]; }
        if (end) CHECK(next_block + nb == f.word.size());                  // (a full table leaves the EndMark for a step of its own)
        CHECK(step_out <= step_max && hist <= P.cap && hist <= T);
        const bool first_step = steps == 0;
        if (!end) CHECK(nb == P.table || (first_step && nb >= P.first_min));
        const u64 T_new = T + step_out, win_lo = T - hist;                   // the device window holds positions [win_lo, T_new)
        const StreamHash h = stream_hash_plan(T, hist, T_new, ghashed, end);
        CHECK(h.virt_back == win_lo);
        CHECK(h.one_shot == (end && first_step));                            // exactly when the entry ends in its first step
        if (h.one_shot) { CHECK(win_lo == 0 && !h.chain && !h.partials && !h.span_up && !final_seen); one_shot_seen = true; tot.one_shot++; }
        else if (h.chain) {
            CHECK(h.span_up && !final_seen && h.g_from == ghashed && h.g_to >= h.g_from);
            const u64 nblk = T_new ? (T_new - 1) >> 10 : 0;
            if (partial_done.size() < h.g_to) { partial_done.resize(h.g_to, 0); chain_done.resize(h.g_to, 0); }
            CHECK(h.partials == (h.g_to > h.g_from));
            CHECK((h.g_to - h.g_from) * 4096 <= P.part_bytes && h.part_back == h.g_from * (XS_GROUP * 8));     // the step's sums fit the partials region, from its start
            for (u64 g = h.g_from; g < h.g_to; g++) {
                const u64 lo = g * XS_GROUP * 1024, hi = std::min<u64>((g + 1) * XS_GROUP, nblk) * 1024;        // what the group's sums read
                CHECK(lo < hi && lo >= win_lo && hi <= T_new);
                partial_done[g]++; chain_done[g]++;
            }
            CHECK(h.b_from == h.g_from * XS_GROUP && h.b_to == h.g_to * XS_GROUP && h.last == (end ? 1 : 0));
            if (h.last) {                                                    // the finish: the block with the last byte, the last stripe reaches 64 bytes back
                const u64 lo = T_new <= 240 ? 0 : std::min<u64>(nblk * 1024, T_new - 64);
                CHECK(lo >= win_lo && h.g_to * XS_GROUP >= nblk);
                final_seen = true;
            } else CHECK(h.b_to <= nblk);                                    // whole groups only, never the block with the last byte
            CHECK(h.ghashed_new == (end ? ghashed : h.g_to));
        } else CHECK(!end && !h.span_up && !h.partials && h.ghashed_new == ghashed);
        // ---- the carry: the last min(have, cap) bytes stay ----
        const StreamCarry k = stream_carry(hist, step_out, P.cap, end);
        if (end || !step_out) CHECK(!k.move && k.hist_new == hist);
        else {
            const u64 have_out = hist + step_out, keep = std::min<u64>(have_out, P.cap);
            CHECK(have_out <= P.cap + step_max);                             // [history | step] fits the window's region
            CHECK(k.keep == keep && k.hist_new == keep && k.move == (have_out > keep));
            const u64 new_lo = k.move ? win_lo + k.from : win_lo;            // the position that lies at the window's start afterwards
            CHECK(new_lo == T_new - keep && (!k.move || k.from + k.keep == have_out));
            tot.carries += k.move;
        }
        T = T_new; hist = k.hist_new; ghashed = h.ghashed_new; next_block += nb; steps++; tot.steps++;
        pend.erase(pend.begin(), pend.begin() + (long)q);
        ended = end;
        if (end) CHECK(all_in && pend.empty());
    }
    // every block in exactly one step; every 64 KiB group summed once and chained once; the finish once and last
    CHECK(next_block == f.word.size() && T == f.total);
    if (one_shot_seen) CHECK(steps == 1 && !final_seen && partial_done.empty());
    else {
        const u64 nblk = T ? (T - 1) >> 10 : 0, groups = (nblk + XS_GROUP - 1) / XS_GROUP;
        CHECK(final_seen && partial_done.size() == groups);
        for (u64 g = 0; g < groups; g++) CHECK(partial_done[g] == 1 && chain_done[g] == 1);
    }
    tot.streams++; tot.stated_bound += stated;
}

static void streams(const char* name, const Params& P, bool heavy)
{
    Totals tot = {};
    const u64 B = P.block_out;
    std::vector<u64> totals = { 0, 1, 240, 241, 65535, 65536, 64 * KiB * 64 - 1, 64 * KiB * 64, 64 * KiB * 64 + 1,
                                B * P.table - 1, B * P.table, B * P.table + 1, B * (P.first_min + 2 * P.table + 5) + 777 };
    if (heavy) totals.push_back(B * 300 + 12345);                            // a history carried over many steps
    for (u64 total : totals)
        for (int kind = 0; kind < 4; kind++) {
            // 0: small bodies, full blocks; 1: short blocks in the middle, every 7th stored; 2: bodies up to 64 KiB; 3: tiny bodies, all but the stored ones
            const Frame f = kind == 0 ? make_frame(total, P.block_out, false, 100, 400, 0) : kind == 1 ? make_frame(total, P.block_out, true, 50, 3000, 7)
                          : kind == 2 ? make_frame(total, P.block_out, true, 30000, 65536, 5) : make_frame(total, P.block_out, false, 1, 12, 3);
            std::vector<u64> windows = { 4096, 65536, 100000, 128 * KiB, 1 * MiB, 9 * MiB, 0, 0 };
            if (f.bytes.size() <= 64 * KiB) { windows.push_back(1); windows.push_back(7); }
            for (u64 w : windows) simulate(f, P, w, tot);
        }
    printf("%s: %llu streams, %llu calls, %llu steps, %llu ended in the first step, %llu carries: every block in one step, every group summed and chained once, "
           "the finish once and last, every read inside the window; pending <= a step + the window in %llu streams\n", name,
           (unsigned long long)tot.streams, (unsigned long long)tot.calls, (unsigned long long)tot.steps, (unsigned long long)tot.one_shot,
           (unsigned long long)tot.carries, (unsigned long long)tot.stated_bound);
}

// ---- (c) layouts ---------------------------------------------------------------------------------------------------------------------------
struct Region { u64 at, need; };
static void regions_ok(const std::vector<Region>& r, u64 size, u64 align)
{
    for (size_t i = 0; i < r.size(); i++) {
        CHECK(r[i].at % align == 0);
        CHECK(r[i].at + r[i].need <= (i + 1 < r.size() ? r[i + 1].at : size));          // ascending, disjoint, the total behind the last one
    }
}
static void layouts()
{
    const FastLayout L = dstream_fast_layout();
    const u64 win = (u64)F_HIST + F_OUT;
    regions_ok({ { L.in, F_IN + FS_SRC_SLACK }, { L.out, win + 64 }, { L.tmp, F_HIST }, { L.S, win * 4 + 64 }, { L.recs, (u64)F_BLOCKS * (PJ_BLOCK / 3 + 2 + 8) * 8 },
                 { L.masks, (u64)F_BLOCKS * (PJ_BLOCK / 8) }, { L.blocks, F_BLOCKS * sizeof(PjBlock) }, { L.flags, 256 }, { L.part, fs_part_bytes(win) },
                 { L.span, FS_SMALL }, { L.hash, 64 }, { L.state, 64 }, { L.rec, FS_SMALL } }, L.size, 256);
    CHECK(L.size == 37957120ull);                                            // recorded from dstream_fast_layout() as it stood in zpk_stream.inc
    CHECK(L.size - L.rec == 256 && F_IN >= F_BLOCKS * (PJ_BLOCK + 4ull) + 4 && fs_part_bytes(win) >= (win / 65536 + 2) * 4096);
    u32 n = 0;
    for (u64 window : { 1 * KiB, 128 * KiB, 1 * MiB, (8 * MiB) + 7 * MiB })
        for (u64 nt : { 1ull, 2ull, 64ull, 65ull })
            for (u64 slots : { 0ull, 1000ull, 65ull * 43691 })
                for (u64 src_total : { 1000ull, 9ull * MiB + 5 }) {
                    CHECK(fz_window_ok(window));
                    const u64 HC = fz_hist_cap(window);
                    CHECK(HC % 256 == 0 && HC >= window && HC >= F_HIST);
                    const FzLayout Z = dstream_fz_layout(nt, slots, src_total, HC);
                    regions_ok({ { Z.in, src_total + FS_SRC_SLACK }, { Z.zb, nt * sizeof(ZpjBlock) }, { Z.pb, nt * sizeof(PjBlock) }, { Z.desc, nt * FZ_DESC_BYTES }, { Z.list, nt * 4 },
                                 { Z.state, nt * 4 }, { Z.rep, nt * 12 }, { Z.recs, (slots + 64) * 8 }, { Z.pos, (slots + 64) * 8 }, { Z.masks, nt * (ZPJ_BLOCK / 8) },
                                 { Z.S, (u64)FZ_CHUNK * ZPJ_BLOCK * 4 + 64 }, { Z.part, fs_part_bytes(HC + FZ_OUT) } }, Z.size, 256);
                    // what persists: the window and the carry's temporary, then the small block (64-byte steps behind the window's 64 bytes of slack)
                    regions_ok({ { Z.out, HC + FZ_OUT + 64 }, { Z.tmp, HC }, { Z.p_state, 64 }, { Z.p_hash, 64 }, { Z.p_span, 128 }, { Z.p_rec, FS_SMALL }, { Z.p_flags, 512 } }, Z.fo_need, 64);
                    CHECK(Z.fo_need == 2 * HC + FZ_OUT + 64 + 1024 && fz_scratch_alloc(Z.size) == Z.size + Z.size / 4);
                    n++;
                }
    CHECK(!fz_window_ok((8 * MiB) + 7 * MiB + 1));
    printf("layout: LZ4 13 regions, %llu bytes as recorded; Zstandard %u shapes: 12 scratch regions 256-aligned, 7 persistent ones 64-aligned, all ascending and disjoint, totals the end of the last region\n",
           (unsigned long long)L.size, n);
}

int main()
{
    tables();
    const u64 lz4_win = (u64)F_HIST + F_OUT;
    streams("streams lz4", Params{ PJ_BLOCK, F_BLOCKS, F_FIRST_MIN, F_HIST, fs_part_bytes(lz4_win) }, true);
    for (u64 window : { 128 * KiB, 1 * MiB, 8 * MiB + 7 * MiB }) {
        const u64 HC = fz_hist_cap(window);
        char name[64]; snprintf(name, sizeof(name), "streams zstd window %llu KiB", (unsigned long long)(window / KiB));
        streams(name, Params{ ZPJ_BLOCK, FZ_BLOCKS, FZ_FIRST_MIN, HC, fs_part_bytes(HC + FZ_OUT) }, window == 128 * KiB);
    }
    layouts();
    return 0;
}
