// The fixed-capacity walkers of zpack_amd/csrc/host_walk.h (walk_lz4_single_into, walk_zstd_single_into: what k_big_walk runs on the device,
// compiled here for the CPU) against the vector walkers, on mutated single frames under ASan + UBSan: built and run by
// tools/hostfuzz/run_big_walk.sh.  Every table is a heap allocation of exactly `capacity` elements: ASan sees a block written behind it.
#include <stdio.h>
#include <stdlib.h>
#include "host_walk.h"
using namespace zpk;

static u64 rng_s = 0x9E3779B97F4A7C15ull;
static u64 rnd() { rng_s ^= rng_s << 13; rng_s ^= rng_s >> 7; rng_s ^= rng_s << 17; return rng_s; }
#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); exit(1); } while (0)

static void put32(std::vector<u8>& e, u32 w) { u8 t[4]; memcpy(t, &w, 4); e.insert(e.end(), t, t + 4); }
static void put24(std::vector<u8>& e, u32 w) { e.push_back((u8)w); e.push_back((u8)(w >> 8)); e.push_back((u8)(w >> 16)); }

// An LZ4 frame as the block-parallel reader takes it: `nb` blocks of 1 .. max_n arbitrary bytes (the walk never looks inside);
// hdrs = where its frame header and block headers start
static std::vector<u8> lz4_frame(int nb, u32 max_n, bool all_stored, std::vector<size_t>& hdrs)
{
    std::vector<u8> e;
    u8 h[7] = {0x04, 0x22, 0x4D, 0x18, (u8)(0x40 | ((rnd() & 1) ? 0x20 : 0)), 0x40, 0};
    h[6] = (u8)(host_xxh32_small(h + 4, 2) >> 8);
    hdrs.clear(); hdrs.push_back(4);
    e.insert(e.end(), h, h + 7);
    for (int b = 0; b < nb; b++) {
        const u32 n = 1 + (u32)(rnd() % max_n);
        hdrs.push_back(e.size());
        put32(e, n | ((all_stored || (rnd() & 3) == 0) ? 0x80000000u : 0));
        for (u32 i = 0; i < n; i++) e.push_back((u8)rnd());
    }
    hdrs.push_back(e.size());
    put32(e, 0);
    return e;
}

// A Zstandard frame of raw, RLE and compressed blocks whose literals and sequences headers are well-formed (the walk reads those and the
// table descriptions, nothing behind them)
static std::vector<u8> zstd_frame(int nb, bool all_raw1, std::vector<size_t>& hdrs)
{
    std::vector<u8> e;
    const u8 h[6] = {0x28, 0xB5, 0x2F, 0xFD, 0x00, 0x58};
    hdrs.clear(); hdrs.push_back(4);
    e.insert(e.end(), h, h + 6);
    bool have_tree = false, have_tabs = false;
    for (int b = 0; b < nb; b++) {
        const u32 type = all_raw1 ? 0 : (u32)(rnd() % 3);
        std::vector<u8> body;
        if (type == 2) {
            u32 lt = (u32)(rnd() % 4); const u32 regen = (u32)(rnd() % 600);
            if (lt == 3 && !have_tree && (rnd() & 7)) lt = 2;                    // (a Treeless block in front of any tree: declined, now and then)
            if (lt < 2) { body.push_back((u8)(lt | (1 << 2) | ((regen & 15) << 4))); body.push_back((u8)(regen >> 4)); const u32 n = lt == 0 ? regen : 1; for (u32 i = 0; i < n; i++) body.push_back((u8)rnd()); }
            else { const u32 cs = 1 + (u32)(rnd() % 300); const u32 v = lt | (1 << 2) | (regen << 4) | (cs << 14); put24(body, v); for (u32 i = 0; i < cs; i++) body.push_back((u8)rnd()); }
            if (lt == 2) have_tree = true;
            const u32 nseq = rnd() % 3 == 0 ? 0 : 1 + (u32)(rnd() % 300);
            if (nseq == 0) body.push_back(0);
            else {
                if (nseq < 128) body.push_back((u8)nseq); else { body.push_back((u8)(128 + (nseq >> 8))); body.push_back((u8)nseq); }
                // predefined, RLE and (once tables exist) Repeat_Mode kinds; an FSE description of random bytes is usually malformed: rarely
                const u8 modes[6] = {0x00, 0x54, 0x10, 0x44, (u8)(have_tabs ? 0xFC : 0x00), (u8)(have_tabs ? 0xCC : 0x54)};
                u8 m = modes[rnd() % 6];
                if ((rnd() & 31) == 0) m = 0xA8;
                body.push_back(m); have_tabs = true;
                const u32 rest = 4 + (u32)(rnd() % 100); for (u32 i = 0; i < rest; i++) body.push_back((u8)rnd());
            }
        }
        const u32 n = type == 2 ? (u32)body.size() : (all_raw1 ? 1 : 1 + (u32)(rnd() % 300));
        hdrs.push_back(e.size());
        put24(e, (b + 1 == nb ? 1u : 0u) | (type << 1) | (n << 3));
        if (type == 2) e.insert(e.end(), body.begin(), body.end()); else for (u32 i = 0; i < (type == 1 ? 1 : n); i++) e.push_back((u8)rnd());
    }
    return e;
}

struct Tally { u64 inputs = 0, accepted = 0, by_capacity = 0, calls = 0; };

// One input through both forms, at the given capacities: the same verdict and the same table wherever the table holds the frame, a decline
// wherever it does not.  -> the vector walker's block count (0: declined)
static u64 check_lz4(const std::vector<u8>& e, u64 uncomp, const std::vector<i64>& caps_rel, Tally& t)
{
    u8* p = (u8*)malloc(e.size() ? e.size() : 1); memcpy(p, e.data(), e.size());          // exact-size heap copy: ASan sees any read past the end
    std::vector<PjBlock> v; int iv = 0;
    const bool okv = walk_lz4_single(p, e.size(), uncomp, v, iv);
    const u64 nbv = okv ? v.size() : 0;
    t.inputs++; if (okv) t.accepted++;
    std::vector<u64> caps;
    for (i64 r : caps_rel) { const i64 c = (i64)nbv + r; if (c >= 0) caps.push_back((u64)c); }
    caps.push_back(walk_lz4_capacity(uncomp)); caps.push_back(rnd() % 24);
    for (u64 cap : caps) {
        PjBlock* tab = (PjBlock*)malloc(cap ? cap * sizeof(PjBlock) : 1);
        u32 n = 77; int ii = -5;
        const bool oki = walk_lz4_single_into(p, e.size(), uncomp, cap ? tab : (PjBlock*)nullptr, (u32)cap, &n, &ii);
        t.calls++;
        if (!okv && oki) FAIL("lz4: the table form accepts what the vector form declines (capacity %llu)", (unsigned long long)cap);
        if (okv && nbv > cap) { if (oki) FAIL("lz4: %llu blocks accepted into a table of %llu", (unsigned long long)nbv, (unsigned long long)cap); t.by_capacity++; }
        if (okv && nbv <= cap) {
            if (!oki || n != nbv || ii != iv) FAIL("lz4: verdict / block count / independent differ (capacity %llu: %d %u/%llu %d/%d)", (unsigned long long)cap, (int)oki, n, (unsigned long long)nbv, ii, iv);
            if (memcmp(tab, v.data(), nbv * sizeof(PjBlock))) FAIL("lz4: the tables differ");
        }
        if (!oki && n != 0) FAIL("lz4: declined with a block count");
        free(tab);
    }
    free(p);
    return nbv;
}

static u64 check_zstd(const std::vector<u8>& e, u64 uncomp, const std::vector<i64>& caps_rel, Tally& t)
{
    u8* p = (u8*)malloc(e.size() ? e.size() : 1); memcpy(p, e.data(), e.size());
    std::vector<ZpjBlock> v; u64 sv = 0, lv = 0;
    const bool okv = walk_zstd_single(p, e.size(), uncomp, v, sv, lv);
    const u64 nbv = okv ? v.size() : 0;
    t.inputs++; if (okv) t.accepted++;
    std::vector<u64> caps;
    for (i64 r : caps_rel) { const i64 c = (i64)nbv + r; if (c >= 0) caps.push_back((u64)c); }
    caps.push_back(walk_zstd_capacity(uncomp)); caps.push_back(rnd() % 24);
    for (u64 cap : caps) {
        ZpjBlock* tab = (ZpjBlock*)malloc(cap ? cap * sizeof(ZpjBlock) : 1);
        u32 n = 77; u64 si = 5, li = 5;
        const bool oki = walk_zstd_single_into(p, e.size(), uncomp, cap ? tab : (ZpjBlock*)nullptr, (u32)cap, &n, &si, &li);
        t.calls++;
        if (!okv && oki) FAIL("zstd: the table form accepts what the vector form declines (capacity %llu)", (unsigned long long)cap);
        if (okv && nbv > cap) { if (oki) FAIL("zstd: %llu blocks accepted into a table of %llu", (unsigned long long)nbv, (unsigned long long)cap); t.by_capacity++; }
        if (okv && nbv <= cap) {
            if (!oki || n != nbv || si != sv || li != lv) FAIL("zstd: verdict / block count / slots / lit_total differ (capacity %llu)", (unsigned long long)cap);
            if (memcmp(tab, v.data(), nbv * sizeof(ZpjBlock))) FAIL("zstd: the tables differ");
        }
        if (!oki && n != 0) FAIL("zstd: declined with a block count");
        free(tab);
    }
    free(p);
    return nbv;
}

// byte flips in the frame header and in block headers, truncation, trailing bytes, a block size made longer
static void mutate(std::vector<u8>& e, const std::vector<size_t>& hdrs, int hdr_bytes)
{
    const int muts = (int)(rnd() % 3);
    for (int m = 0; m < muts && !e.empty(); m++) {
        const int kind = (int)(rnd() % 6);
        const size_t h0 = hdrs[rnd() % hdrs.size()], at = h0 + rnd() % (size_t)hdr_bytes;
        const size_t size_byte = h0 + (hdr_bytes == 3 ? 1 : 0);                         // (LZ4: the low byte of the size; Zstandard: bits 5 .. 12 of it)
        if (kind == 0 && at < e.size()) e[at] ^= (u8)(1u << (rnd() % 8));
        else if (kind == 1 && at < e.size()) e[at] = (u8)rnd();
        else if (kind == 2) e.resize(rnd() % (e.size() + 1));
        else if (kind == 3) { const size_t n = 1 + rnd() % 40; for (size_t i = 0; i < n; i++) e.push_back((u8)rnd()); }
        else if (kind == 4 && size_byte < e.size()) e[size_byte] += (u8)(1 + rnd() % 16);       // a block that says it is longer
        else e[rnd() % e.size()] ^= (u8)(1u << (rnd() % 8));
    }
}

int main(int argc, char** argv)
{
    const u64 iters = argc > 1 ? strtoull(argv[1], 0, 10) : 1000000;
    const std::vector<i64> around = { -1, 0, 1 };
    std::vector<size_t> hdrs;
    Tally fixed;
    // ---- intact frames at the capacities nb - 1, nb, nb + 1: accepted exactly when the table holds them ----
    for (int nb = 4; nb <= 40; nb++) {
        const std::vector<u8> a = lz4_frame(nb, 200, false, hdrs);
        if (check_lz4(a, (u64)nb * PJ_BLOCK, around, fixed) != (u64)nb) FAIL("an intact LZ4 frame of %d blocks is declined", nb);
        const std::vector<u8> z = zstd_frame(nb, true, hdrs);
        if (check_zstd(z, (u64)nb, around, fixed) != (u64)nb) FAIL("an intact Zstandard frame of %d raw blocks is declined", nb);
    }
    // ---- several thousand one-byte stored blocks: far more than the capacity a descriptor of that size gives ----
    for (int nb : { 3000, 5000 }) {
        const std::vector<u8> a = lz4_frame(nb, 1, true, hdrs);
        if (walk_lz4_capacity((u64)nb) >= (u64)nb) FAIL("capacity rule");
        if (check_lz4(a, (u64)nb, around, fixed) != (u64)nb) FAIL("the LZ4 frame of %d one-byte blocks is declined by the vector form", nb);
        const std::vector<u8> z = zstd_frame(nb, true, hdrs);
        if (check_zstd(z, (u64)nb, around, fixed) != (u64)nb) FAIL("the Zstandard frame of %d one-byte blocks is declined by the vector form", nb);
    }
    if (fixed.by_capacity < 2 * (37 + 2) + 4) FAIL("too few declines by capacity among the intact frames: %llu", (unsigned long long)fixed.by_capacity);
    // ---- mutated frames ----
    Tally l, z;
    for (u64 it = 0; it < iters; it++) {
        const int nb = 2 + (int)(rnd() % 14);
        if (rnd() & 1) {
            std::vector<u8> e = lz4_frame(nb, 200, false, hdrs);
            mutate(e, hdrs, 4);
            check_lz4(e, (rnd() & 3) ? (u64)nb * PJ_BLOCK - rnd() % PJ_BLOCK : rnd() % (1u << 22), around, l);
        } else {
            std::vector<u8> e = zstd_frame(nb, false, hdrs);
            mutate(e, hdrs, 3);
            check_zstd(e, rnd() % (1u << 22), around, z);
        }
    }
    printf("%llu intact frames at the capacities nb - 1, nb, nb + 1, among them frames of 3000 and 5000 one-byte blocks: %llu declines by capacity, every other table identical\n",
           (unsigned long long)fixed.inputs, (unsigned long long)fixed.by_capacity);
    printf("%llu mutated LZ4 frames (%llu accepted) and %llu mutated Zstandard frames (%llu accepted) through both forms at %llu capacities: the table form agrees with the vector form, declines by capacity %llu\n",
           (unsigned long long)l.inputs, (unsigned long long)l.accepted, (unsigned long long)z.inputs, (unsigned long long)z.accepted,
           (unsigned long long)(l.calls + z.calls), (unsigned long long)(l.by_capacity + z.by_capacity));
    if (iters >= 1000 && (l.accepted == 0 || z.accepted == 0)) FAIL("no mutated frame was accepted: the harness checks nothing");
    return 0;
}
