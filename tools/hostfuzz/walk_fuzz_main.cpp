// zpack_amd/csrc/host_walk.h, the header the codec compiles, on mutated frames under ASan + UBSan: built and run by tools/hostfuzz/run.sh
#include <stdio.h>
#include <stdlib.h>
#include "host_walk.h"
using namespace zpk;

static u64 rng_s = 88172645463325252ull;
static u64 rnd() { rng_s ^= rng_s << 13; rng_s ^= rng_s >> 7; rng_s ^= rng_s << 17; return rng_s; }
int main(int argc, char** argv) {
    // seeds: well-formed sequences of frames built by hand (block payloads are arbitrary bytes: the walkers never look inside)
    std::vector<std::vector<u8>> seeds;
    for (int method = 1; method <= 2; method++) for (int nf = 1; nf <= 4; nf++) {
        std::vector<u8> e;
        for (int f = 0; f < nf; f++) {
            const u64 csz = 256 * (1 + rnd() % 8);
            if (method == 2) {
                u8 h[15] = {0x04,0x22,0x4D,0x18, (u8)(0x48 | ((rnd()&1)?0x10:0) | ((rnd()&1)?0x04:0)), 0x40}; memcpy(h + 6, &csz, 8); h[14] = 0x5A;
                e.insert(e.end(), h, h + 15);
                const int nb = 1 + rnd() % 3;
                for (int b = 0; b < nb; b++) { u32 n = 1 + rnd() % 300; u32 w = n | ((rnd()&1) ? 0x80000000u : 0); u8 t[4]; memcpy(t, &w, 4); e.insert(e.end(), t, t + 4); for (u32 i = 0; i < n + ((h[4] & 0x10) ? 4 : 0); i++) e.push_back((u8)rnd()); }
                u8 z[4] = {0,0,0,0}; e.insert(e.end(), z, z + 4); if (h[4] & 0x04) e.insert(e.end(), z, z + 4);
            } else {
                u8 h[4] = {0x28,0xB5,0x2F,0xFD}; e.insert(e.end(), h, h + 4);
                const int ss = rnd() & 1, ck = rnd() & 1; const int flag = 1 + rnd() % 3;
                e.push_back((u8)((flag << 6) | (ss << 5) | (ck << 2)));
                if (!ss) e.push_back(0x30);
                const u64 v = flag == 1 ? csz - 256 : csz; const int nbytes = flag == 1 ? 2 : flag == 2 ? 4 : 8;
                for (int i = 0; i < nbytes; i++) e.push_back((u8)(v >> (8 * i)));
                const int nb = 1 + rnd() % 3;
                for (int b = 0; b < nb; b++) { const u32 type = rnd() % 3; const u32 n = 1 + rnd() % 300; const u32 w = (b + 1 == nb ? 1u : 0u) | (type << 1) | (n << 3); e.push_back((u8)w); e.push_back((u8)(w >> 8)); e.push_back((u8)(w >> 16)); for (u32 i = 0; i < (type == 1 ? 1 : n); i++) e.push_back((u8)rnd()); }
                if (ck) for (int i = 0; i < 4; i++) e.push_back((u8)rnd());
            }
        }
        seeds.push_back(e);
    }
    u64 iters = argc > 1 ? strtoull(argv[1], 0, 10) : 2000000, accepted = 0, intact_ok = 0;
    std::vector<BigSub> subs;
    for (size_t k = 0; k < seeds.size(); k++) {            // intact seeds with the right total must be accepted when they hold >= 2 frames
        const int method = k < 4 ? 1 : 2; const int nf = (int)(k % 4) + 1;
        u64 total = 0; { std::vector<BigSub> t; /* total from a permissive first walk */ for (u64 u = 256; u <= 256 * 8 * 4; u += 256) { t.clear(); if ((method == 2 ? walk_lz4_frames : walk_zstd_frames)(seeds[k].data(), seeds[k].size(), u, t)) { total = u; break; } } }
        if (nf >= 2 && total) intact_ok++;
        if (nf >= 2 && !total) { printf("seed %zu (method %d, %d frames) not accepted\n", k, method, nf); return 1; }
    }
    for (u64 it = 0; it < iters; it++) {
        const size_t k = rnd() % seeds.size();
        std::vector<u8> e = seeds[k];
        const int muts = rnd() % 4;
        for (int m = 0; m < muts; m++) { const int kind = rnd() % 4; if (e.empty()) break;
            if (kind == 0) e[rnd() % e.size()] ^= (u8)(1u << (rnd() % 8));
            else if (kind == 1) e[rnd() % e.size()] = (u8)rnd();
            else if (kind == 2) e.resize(rnd() % (e.size() + 1));
            else { const size_t n = rnd() % 40; for (size_t i = 0; i < n; i++) e.push_back((u8)rnd()); } }
        // exact-size heap copy: ASan sees any read past the end
        u8* p = (u8*)malloc(e.size() ? e.size() : 1); memcpy(p, e.data(), e.size());
        const u64 uncomp = (rnd() & 3) ? 256 * (1 + rnd() % 40) : rnd();
        subs.clear();
        const bool ok = (k < 4 ? walk_zstd_frames : walk_lz4_frames)(p, e.size(), uncomp, subs);
        if (ok) { accepted++; u64 out = 0, ip = 0;
            if (subs.size() < 2) { printf("accepted with < 2 frames\n"); return 1; }
            for (auto& S : subs) { if (S.src_off != ip || S.out_off != out || S.size == 0 || (S.out_off & 255) || S.comp > e.size() - S.src_off) { printf("inconsistent plan\n"); return 1; } ip += S.comp; out += S.size; }
            if (ip != e.size() || out != uncomp) { printf("plan does not tile the entry\n"); return 1; } }
        else if (!subs.empty()) { printf("refused but left frames behind\n"); return 1; }
        free(p);
    }
    // ---- ONE frame (block-parallel readers): hand-built single frames of >= 8 blocks, mutated; whatever the walkers accept must lie inside the entry
    u64 acc1 = 0, acc2 = 0;
    for (u64 it = 0; it < iters; it++) {
        std::vector<u8> e;
        const int method = 1 + (int)(rnd() & 1);
        const int nb = 8 + rnd() % 6;
        u64 uncomp = 0;
        if (method == 2) {
            u8 h[7] = {0x04,0x22,0x4D,0x18, (u8)(0x40 | ((rnd() & 1) ? 0x20 : 0)), 0x40, 0};
            h[6] = (u8)(host_xxh32_small(h + 4, 2) >> 8);
            e.insert(e.end(), h, h + 7);
            for (int b = 0; b < nb; b++) { u32 n = 1 + rnd() % 200; u32 w = n | ((rnd() & 3) == 0 ? 0x80000000u : 0); u8 t[4]; memcpy(t, &w, 4); e.insert(e.end(), t, t + 4); for (u32 i = 0; i < n; i++) e.push_back((u8)rnd()); uncomp += 65536; }
            u8 z[4] = {0,0,0,0}; e.insert(e.end(), z, z + 4);
        } else {
            u8 h[6] = {0x28,0xB5,0x2F,0xFD, 0x00, 0x58}; e.insert(e.end(), h, h + 6);
            for (int b = 0; b < nb; b++) {
                const u32 type = rnd() % 3;
                std::vector<u8> body;
                if (type == 2) {                          // literals header (raw / RLE / "compressed" / treeless) + sequences header
                    const u32 lt = rnd() % 4; const u32 regen = rnd() % 600;
                    if (lt < 2) { body.push_back((u8)(lt | (1 << 2) | ((regen & 15) << 4))); body.push_back((u8)(regen >> 4)); const u32 n = lt == 0 ? regen : 1; for (u32 i = 0; i < n; i++) body.push_back((u8)rnd()); }
                    else { const u32 cs = 1 + rnd() % 300; const u32 v = lt | (1 << 2) | (regen << 4) | (cs << 14); body.push_back((u8)v); body.push_back((u8)(v >> 8)); body.push_back((u8)(v >> 16)); for (u32 i = 0; i < cs; i++) body.push_back((u8)rnd()); }
                    const u32 nseq = rnd() % 3 == 0 ? 0 : 1 + rnd() % 300;
                    if (nseq == 0) body.push_back(0);
                    else { if (nseq < 128) body.push_back((u8)nseq); else { body.push_back((u8)(128 + (nseq >> 8))); body.push_back((u8)nseq); }
                           const u8 modes[8] = {0x00, 0xA8, 0x54, 0x20, 0xFC, 0x30, 0x0C, 0xC0}; body.push_back(modes[rnd() % 8]); /* (incl. Repeat_Mode kinds) */ const u32 rest = 4 + rnd() % 100; for (u32 i = 0; i < rest; i++) body.push_back((u8)rnd()); }
                }
                const u32 n = type == 2 ? (u32)body.size() : 1 + rnd() % 300;
                const u32 w = (b + 1 == nb ? 1u : 0u) | (type << 1) | (n << 3); e.push_back((u8)w); e.push_back((u8)(w >> 8)); e.push_back((u8)(w >> 16));
                if (type == 2) e.insert(e.end(), body.begin(), body.end()); else for (u32 i = 0; i < (type == 1 ? 1 : n); i++) e.push_back((u8)rnd());
            }
            uncomp = rnd() % (1u << 22);
        }
        const int muts = rnd() % 4;
        for (int m = 0; m < muts; m++) { const int kind = rnd() % 4; if (e.empty()) break;
            if (kind == 0) e[rnd() % e.size()] ^= (u8)(1u << (rnd() % 8));
            else if (kind == 1) e[rnd() % e.size()] = (u8)rnd();
            else if (kind == 2) e.resize(rnd() % (e.size() + 1));
            else { const size_t n = rnd() % 40; for (size_t i = 0; i < n; i++) e.push_back((u8)rnd()); } }
        u8* p = (u8*)malloc(e.size() ? e.size() : 1); memcpy(p, e.data(), e.size());
        if (method == 2) {
            std::vector<PjBlock> blocks; int indep = 0;
            if (walk_lz4_single(p, e.size(), uncomp, blocks, indep)) {
                acc1++;
                if (blocks.size() < ZPK_PJ_MIN_BLOCKS) { printf("lz4 single: too few blocks accepted\n"); return 1; }
                u64 at = 7;
                for (auto& B : blocks) { const u32 n = B.comp_size & 0x7FFFFFFFu; if (B.comp_off != at + 4 || n == 0 || n > PJ_BLOCK || (u64)B.comp_off + n > e.size()) { printf("lz4 single: block outside the entry\n"); return 1; } at = (u64)B.comp_off + n; }
                if (at + 4 != e.size()) { printf("lz4 single: the frame does not end the entry\n"); return 1; }
            }
        } else {
            std::vector<ZpjBlock> zb; u64 slots = 0, lit = 0;
            if (walk_zstd_single(p, e.size(), uncomp, zb, slots, lit)) {
                acc2++;
                u64 sl = 0;
                for (auto& B : zb) {
                    const u64 body = B.type == 1 ? 1 : B.size;
                    if ((u64)B.hdr_off + 3 + body > e.size() || B.type > 2) { printf("zstd single: block outside the entry\n"); return 1; }
                    if (B.type == 2) { if (B.lit_used > B.size || B.lit_size > ZPJ_BLOCK || B.seq_base != sl || (B.lit_type == 3 && B.tree_src >= zb.size())) { printf("zstd single: inconsistent block\n"); return 1; } sl += (u64)B.nseq + 1; }
                }
                if (sl != slots) { printf("zstd single: slots\n"); return 1; }
            }
            // the block parser alone, at every offset of the mutated entry (what the streaming steps do with bytes as they arrive)
            ZpjTabs tb; for (int k = 0; k < 3; k++) { tb.mode[k] = rnd() % 4; tb.off[k] = (u32)rnd(); }
            for (u64 q = 0; q < e.size(); q += 1 + rnd() % 7) { ZpjBlock B; u32 last = 0; u64 total = 0; const int r = zpj_parse_block(p + q, e.size() - q, q, B, &last, &total, (rnd() & 1) ? &tb : nullptr); if (r == 1 && q + total > e.size()) { printf("zpj_parse_block: a block beyond its bytes\n"); return 1; } }
            for (u64 q = 0; q < e.size(); q += 1 + rnd() % 11) (void)zpj_ncount_len(p + q, e.size() - q, 52, 9);
            u64 win = 0, fcs = 0; (void)zpj_parse_frame_header(p, e.size(), 23, &win, &fcs);
        }
        free(p);
    }
    // ---- the LZ4 stream step's parsers: the shared frame header and the scan for complete blocks, on mutated single frames cut off at several
    // lengths (bytes as they arrive); every block reported must lie inside the bytes that were given
    u64 hdr_ok = 0, blocks_seen = 0, ends = 0;
    for (u64 it = 0; it < iters; it++) {
        std::vector<u8> e;
        u8 h[15] = {0x04,0x22,0x4D,0x18, (u8)(0x40 | ((rnd() & 1) ? 0x20 : 0) | ((rnd() & 1) ? 0x08 : 0)), 0x40};
        const u32 hl = (h[4] & 0x08) ? 15 : 7;
        for (u32 i = 6; i + 1 < hl; i++) h[i] = (u8)rnd();
        h[hl - 1] = (u8)(host_xxh32_small(h + 4, hl - 5) >> 8);
        e.insert(e.end(), h, h + hl);
        const int nb = 1 + rnd() % 70;                        // (more than the 64 blocks of a step, now and then)
        for (int b = 0; b < nb; b++) { u32 n = rnd() % 120; u32 w = n | ((rnd() & 3) == 0 ? 0x80000000u : 0); u8 t[4]; memcpy(t, &w, 4); e.insert(e.end(), t, t + 4); for (u32 i = 0; i < n; i++) e.push_back((u8)rnd()); }
        u8 z[4] = {0,0,0,0}; e.insert(e.end(), z, z + 4);
        const int muts = rnd() % 4;
        for (int m = 0; m < muts; m++) { const int kind = rnd() % 4; if (e.empty()) break;
            if (kind == 0) e[rnd() % e.size()] ^= (u8)(1u << (rnd() % 8));
            else if (kind == 1) e[rnd() % e.size()] = (u8)rnd();
            else if (kind == 2) e.resize(rnd() % (e.size() + 1));
            else { const size_t n = rnd() % 40; for (size_t i = 0; i < n; i++) e.push_back((u8)rnd()); } }
        for (int cut = 0; cut < 4; cut++) {
            const u64 len = cut == 0 ? e.size() : cut == 1 ? rnd() % 20 : rnd() % (e.size() + 1);
            u8* p = (u8*)malloc(len ? len : 1); memcpy(p, e.data(), len);      // exact-size heap copy of what has "arrived"
            int indep = -1, has_cs = -1; u64 content = 0;
            const int hdr = lz4_single_header(p, len, &indep, &has_cs, &content);
            if (hdr > 0) {
                hdr_ok++;
                if ((hdr != 7 && hdr != 15) || (u64)hdr > len || (indep | 1) != 1 || has_cs != (hdr == 15)) { printf("lz4 header: inconsistent answer\n"); return 1; }
                const u64 avail = len - (u64)hdr; const u32 maxb = 1 + rnd() % 64;
                u8* r = (u8*)malloc(avail ? avail : 1); memcpy(r, p + hdr, avail);                  // (the stream step drops the header from its pending bytes)
                PjBlock* tab = (PjBlock*)malloc(maxb * sizeof(PjBlock));                            // exactly max_blocks entries: ASan sees one too many
                u64 used = 0; bool end = false;
                const int n = lz4_stream_blocks(r, avail, tab, maxb, &used, &end);
                if (n >= 0) {
                    if ((u32)n > maxb || used > avail) { printf("lz4 stream scan: more blocks or bytes than it was given\n"); return 1; }
                    u64 at = 0;
                    for (int b = 0; b < n; b++) { const u32 sz = tab[b].comp_size & 0x7FFFFFFFu; if (tab[b].comp_off != at + 4 || sz > PJ_BLOCK || (u64)tab[b].comp_off + sz > avail) { printf("lz4 stream scan: block outside its bytes\n"); return 1; } at = (u64)tab[b].comp_off + sz; }
                    if (at + (end ? 4 : 0) != used) { printf("lz4 stream scan: consumed bytes disagree with the blocks\n"); return 1; }
                    blocks_seen += (u64)n; ends += end ? 1 : 0;
                }
                free(tab); free(r);
            } else if (hdr != 0 && hdr != -1) { printf("lz4 header: unknown answer\n"); return 1; }
            free(p);
        }
    }
    printf("%llu mutated single frames walked: %llu LZ4 / %llu Zstandard accepted for the block-parallel readers, every accepted block inside its entry\n", (unsigned long long)iters, (unsigned long long)acc1, (unsigned long long)acc2);
    printf("%llu mutated entries walked, %llu accepted as frame sequences (every accepted plan tiles its entry exactly), %llu intact seeds accepted\n", (unsigned long long)iters, (unsigned long long)accepted, (unsigned long long)intact_ok);
    printf("%llu mutated LZ4 frames at 4 lengths each through the stream step's header and block scan: %llu headers taken, %llu blocks and %llu EndMarks found, every block inside the bytes given, consumed <= available\n",
           (unsigned long long)iters, (unsigned long long)hdr_ok, (unsigned long long)blocks_seen, (unsigned long long)ends);
    return 0;
}
