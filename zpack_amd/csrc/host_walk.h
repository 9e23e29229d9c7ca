// host_walk.h — the host code that parses UNTRUSTED archive bytes for the frame-parallel and block-parallel readers (zpk_codec.hip) and
// for the bounded stream steps (zpk_stream.inc): frame headers, block headers, block tables.
// Plain C++17, standard headers only: tools/hostfuzz builds this file with g++ under ASan + UBSan (g++ knows no HIP), which keeps it so.
// The walk over ONE large frame is also device code (k_big_walk, big_walk.h): ZPK_HD is empty on a CPU build, so the rules exist once.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "pj_types.h"

#ifndef ZPK_HD
#ifdef __HIPCC__
#define ZPK_HD __host__ __device__
#else
#define ZPK_HD
#endif
#endif

namespace zpk {

// ---- entries that are SEQUENCES OF FRAMES, decoded frame-parallel (host path) -----------------------------------------------------
// One wave decodes one frame; an entry of hundreds of MiB in ONE frame is therefore one wave's work (~0.1 GB/s).  Entries written by
// this library's own writer above 2 MiB (zpk_encode.inc, zpk_stream.inc) are sequences of 512 KiB frames that each state their
// content size: the host walks the frames' block headers (4 / 3 bytes per block, in the caller's archive image), and when the frames
// tile the entry exactly — >= 2 of them, every one with its content size, the sizes summing to uncomp_size — they go to the device
// as a batch of their own, every frame a sub-entry with its own output range; the entry's XXH3 is computed over the assembled
// output by the whole chip (xxh3_span.h).  Large stored entries are cut into 512 KiB slices the same way.  Anything else — a single
// frame, a frame without content size, skippable frames, trailing bytes, a guard of lib/zpack_read.c:328-348 that would fire — stays
// with the one-wave decoders, and so does every entry one of whose frames fails here: verdicts come from one place only.
struct BigSub { u64 src_off, comp, out_off, size; };                  // a frame: byte ranges relative to its entry
ZPK_HD static inline u32 hrd32(const u8* p) { u32 v; memcpy(&v, p, 4); return v; }
ZPK_HD static inline u64 hrd64(const u8* p) { u64 v; memcpy(&v, p, 8); return v; }

static bool walk_lz4_frames(const u8* p, u64 comp, u64 uncomp, std::vector<BigSub>& subs)
{
    const size_t start = subs.size();
    u64 ip = 0, out = 0;
    while (ip < comp) {
        if (comp - ip < 15 + 4 || hrd32(p + ip) != 0x184D2204u) goto other;
        {
            const u8 flg = p[ip + 4];
            if ((flg >> 6) != 1 || (flg & 0x03) || !(flg & 0x08)) goto other;        // version 01, no reserved bit, no dictionary, content size present
            const u64 csz = hrd64(p + ip + 6);
            u64 q = ip + 15;
            for (;;) {
                if (comp - q < 4) goto other;
                const u32 w = hrd32(p + q); q += 4;
                if (w == 0) break;
                const u64 nb = (u64)(w & 0x7FFFFFFFu) + ((flg & 0x10) ? 4 : 0);
                if (nb > comp - q) goto other;
                q += nb;
            }
            if (flg & 0x04) { if (comp - q < 4) goto other; q += 4; }
            if (csz == 0 || csz > uncomp - out || (out & 255)) goto other;           // (output ranges start on 256-byte boundaries, like the slots of any batch)
            subs.push_back(BigSub{ ip, q - ip, out, csz });
            out += csz; ip = q;
        }
    }
    if (out == uncomp && subs.size() - start >= 2) return true;
other:
    subs.resize(start);
    return false;
}

static bool walk_zstd_frames(const u8* p, u64 comp, u64 uncomp, std::vector<BigSub>& subs)
{
    const size_t start = subs.size();
    u64 ip = 0, out = 0;
    while (ip < comp) {
        if (comp - ip < 4 + 1 + 1 + 3 || hrd32(p + ip) != 0xFD2FB528u) goto other;
        {
            const u8 fhd = p[ip + 4];
            const u32 fcs_flag = fhd >> 6, ss = (fhd >> 5) & 1, did = fhd & 3;
            if (fhd & 0x08) goto other;                                               // reserved bit
            const u32 fcs_bytes = fcs_flag == 0 ? ss : (fcs_flag == 1 ? 2u : (fcs_flag == 2 ? 4u : 8u));
            if (!fcs_bytes) goto other;                                               // no content size: its output cannot be placed
            u64 q = ip + 5 + (ss ? 0 : 1) + (did == 3 ? 4 : did);
            if (q > comp || comp - q < fcs_bytes) goto other;
            u64 fcs = 0;
            for (u32 i = 0; i < fcs_bytes; i++) fcs |= (u64)p[q + i] << (8 * i);
            if (fcs_bytes == 2) fcs += 256;
            q += fcs_bytes;
            for (;;) {
                if (comp - q < 3) goto other;
                const u32 w = (u32)p[q] | ((u32)p[q + 1] << 8) | ((u32)p[q + 2] << 16); q += 3;
                const u32 type = (w >> 1) & 3;
                if (type == 3) goto other;
                const u64 nb = type == 1 ? 1 : (w >> 3);
                if (nb > comp - q) goto other;
                q += nb;
                if (w & 1) break;
            }
            if (fhd & 0x04) { if (comp - q < 4) goto other; q += 4; }
            if (fcs == 0 || fcs > uncomp - out || (out & 255)) goto other;
            subs.push_back(BigSub{ ip, q - ip, out, fcs });
            out += fcs; ip = q;
        }
    }
    if (out == uncomp && subs.size() - start >= 2) return true;
other:
    subs.resize(start);
    return false;
}

// ---- ONE LARGE LZ4 FRAME (what the reference writer produces for any large entry: lib/zpack_write.c:204-210), block-parallel: lz4_pj.h ----
// XXH32 of a frame descriptor (2 .. 14 bytes; xxHash specification, inputs shorter than 16 bytes): the header checksum byte is (h >> 8) & 0xFF
ZPK_HD static u32 host_xxh32_small(const u8* p, u32 len)
{
    const u32 P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
    (void)P1; (void)P2;
    u32 h = P5 + len;
    u32 i = 0;
    for (; i + 4 <= len; i += 4) { h += hrd32(p + i) * P3; h = ((h << 17) | (h >> 15)) * P4; }
    for (; i < len; i++) { h += (u32)p[i] * P5; h = ((h << 11) | (h >> 21)) * P1; }
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}
#ifndef ZPK_PJ_MIN_BLOCKS
#define ZPK_PJ_MIN_BLOCKS 4u                          // LZ4: 256 KiB (fewer blocks: the fixed ~0.6 ms is not earned back)
#define ZPK_ZPJ_MIN_BLOCKS 2u                         // Zstandard: 2 blocks (the serial FSE chain of ONE block, ~3.5 ms, is the fixed cost either way)
#endif
// The header of ONE LZ4 frame as the block-parallel readers take it: version 01; no reserved bit, block / content checksum or dictionary;
// 64 KiB blocks; a header checksum byte that is right.  -> its size, 7 or 15 (0: the bytes end inside it, -1: not this path's);
// *independent = the blocks do not reach into each other, *has_content_size / *content_size = what the frame says about its output.
ZPK_HD static int lz4_single_header(const u8* p, u64 avail, int* independent, int* has_content_size, u64* content_size)
{
    if (avail < 7) return 0;
    if (hrd32(p) != 0x184D2204u) return -1;
    const u32 flg = p[4], bd = p[5];
    if ((flg >> 6) != 1 || (flg & 0x17) || bd != 0x40) return -1;
    const u32 hdr = 7 + ((flg & 0x08) ? 8u : 0u);
    if (avail < hdr) return 0;
    if (((host_xxh32_small(p + 4, hdr - 5) >> 8) & 0xFF) != p[hdr - 1]) return -1;
    *independent = (flg >> 5) & 1; *has_content_size = (flg >> 3) & 1; *content_size = (flg & 0x08) ? hrd64(p + 6) : 0;
    return (int)hdr;
}

// The complete blocks among the `avail` bytes at p, which follow the header of such a frame (the LZ4 stream step: bytes as they arrive):
// -> how many, at most max_blocks, in tab (offsets relative to p), or -1: a block larger than 64 KiB.  *consumed = the bytes they and
// the EndMark take, *end = the EndMark was seen.  An incomplete block is where the scan stops, not an error, and a stored block of
// length 0 is taken: not the scan of walk_lz4_single, which refuses both — their stop conditions differ on purpose.
static int lz4_stream_blocks(const u8* p, u64 avail, PjBlock* tab, u32 max_blocks, u64* consumed, bool* end)
{
    u32 nb = 0; u64 q = 0, recs = 0;
    *end = false;
    while (nb < max_blocks) {
        if (avail - q < 4) break;
        const u32 w = hrd32(p + q);
        if (w == 0) { *end = true; q += 4; break; }
        const u32 n = w & 0x7FFFFFFFu;
        if (n > PJ_BLOCK) return -1;
        if (avail - q - 4 < n) break;
        PjBlock& B = tab[nb]; B.comp_off = (u32)(q + 4); B.comp_size = w; B.rec_base = (u32)recs; B.out_size = 0; B.out_off = 0; B.nrec = 0;
        if (!(w >> 31)) recs += n / 3 + 2;
        nb++; q += 4 + n;
    }
    *consumed = q;
    return (int)nb;
}

// ---- where a walk over ONE frame puts its block table ------------------------------------------------------------------------------------
// The host readers grow a std::vector; the walk on the device (k_big_walk) and its CPU harness fill a table of FIXED capacity that the
// caller sized from descriptor fields alone.  A frame with more blocks than the table holds is declined, like any other irregular frame:
// push() refuses the block behind the last slot and nothing is written there, so a walk makes at most capacity + 1 turns of its loop
// (every turn takes at least 3 bytes of the entry).
template <class T> struct WalkVec {                                   // host only
    std::vector<T>& v;
    bool push(const T& b) { v.push_back(b); return true; }
    u64 size() const { return v.size(); }
};
template <class T> struct WalkTab {
    T* tab; u32 cap, n;
    ZPK_HD bool push(const T& b) { if (n >= cap) return false; tab[n++] = b; return true; }
    ZPK_HD u64 size() const { return n; }
};
// Table capacities of the fixed form: twice the blocks a frame of full blocks has, + 8 (a writer may close blocks early)
ZPK_HD static inline u64 walk_lz4_capacity(u64 uncomp) { return 2 * ((uncomp + PJ_BLOCK - 1) / PJ_BLOCK) + 8; }
ZPK_HD static inline u64 walk_zstd_capacity(u64 uncomp) { return 2 * ((uncomp + ZPJ_BLOCK - 1) / ZPJ_BLOCK) + 8; }

// The entry is ONE frame of 64 KiB blocks, nothing optional but a content size that agrees with the entry, nothing behind its EndMark:
// its block table (offsets relative to the entry).  Anything else: false (the one-wave decoder's).
template <class Sink> ZPK_HD static bool walk_lz4_single_to(const u8* p, u64 comp, u64 uncomp, Sink& blocks, int& independent)
{
    if (comp >= 0x7FFF0000ull || uncomp >= 0x7FFF0000ull) return false;
    int has_cs = 0; u64 content = 0;
    const int hdr = lz4_single_header(p, comp, &independent, &has_cs, &content);
    if (hdr <= 0 || comp < (u64)hdr + 4 || (has_cs && content != uncomp)) return false;
    u64 q = (u64)hdr, recs = 0;
    for (;;) {
        if (comp - q < 4) return false;
        const u32 w = hrd32(p + q); q += 4;
        if (w == 0) break;
        const u32 n = w & 0x7FFFFFFFu;
        if (n == 0 || n > PJ_BLOCK || n > comp - q) return false;
        PjBlock B; B.comp_off = (u32)q; B.comp_size = w; B.rec_base = (u32)recs; B.out_size = 0; B.out_off = 0; B.nrec = 0;
        if (!(w >> 31)) recs += n / 3 + 2;
        if (recs > 0xFFFFFF00ull) return false;
        if (!blocks.push(B)) return false;
        q += n;
    }
    return q == comp && blocks.size() >= ZPK_PJ_MIN_BLOCKS;
}
static bool walk_lz4_single(const u8* p, u64 comp, u64 uncomp, std::vector<PjBlock>& blocks, int& independent)
{
    blocks.clear();
    WalkVec<PjBlock> sink{ blocks };
    return walk_lz4_single_to(p, comp, uncomp, sink, independent);
}
// ... into tab[0, capacity): *nblocks = the blocks it holds (0 when the frame is declined; slots behind *nblocks may have been written)
ZPK_HD static bool walk_lz4_single_into(const u8* p, u64 comp, u64 uncomp, PjBlock* tab, u32 capacity, u32* nblocks, int* independent)
{
    WalkTab<PjBlock> sink{ tab, capacity, 0 };
    int indep = 0;
    const bool ok = walk_lz4_single_to(p, comp, uncomp, sink, indep);
    *nblocks = ok ? sink.n : 0; *independent = indep;
    return ok;
}

// Bytes an FSE table description (RFC 8878 4.1.1) takes, or -1 (malformed / beyond `avail` / more symbols or accuracy than its kind allows)
ZPK_HD static int zpj_ncount_len(const u8* p, u64 avail, int max_sym, int max_al)
{
    u64 bit = 0;
    auto rd = [&](u32 n) -> i64 {                                   // n <= 16 bits from the LSB-first stream; -1 beyond the bytes
        if (((bit + n + 7) >> 3) > avail) return -1;
        u32 v = 0;
        for (u32 i = 0; i < 4 && (bit >> 3) + i < avail; i++) v |= (u32)p[(bit >> 3) + i] << (8 * i);
        v = (v >> (bit & 7)) & ((1u << n) - 1u);
        bit += n;
        return (i64)v;
    };
    i64 x = rd(4);
    if (x < 0) return -1;
    const int al = 5 + (int)x;
    if (al > max_al) return -1;
    int remaining = 1 << al, s = 0;
    while (remaining > 0 && s <= max_sym) {
        int nb = 0; for (u32 t = (u32)remaining + 1; t; t >>= 1) nb++;      // highbit(remaining + 1) + 1
        x = rd((u32)nb);
        if (x < 0) return -1;
        u32 val = (u32)x;
        const u32 lower_mask = (1u << (nb - 1)) - 1, threshold = (1u << nb) - 1 - ((u32)remaining + 1);
        if ((val & lower_mask) < threshold) { bit -= 1; val &= lower_mask; }
        else if (val > lower_mask) val -= threshold;
        const int proba = (int)val - 1;
        remaining -= proba < 0 ? 1 : proba;
        s++;
        if (proba == 0) {
            for (;;) {
                x = rd(2);
                if (x < 0) return -1;
                s += (int)x;
                if (s > max_sym + 1) return -1;
                if (x != 3) break;
            }
        }
    }
    if (remaining != 0) return -1;
    return (int)((bit + 7) >> 3);
}
// what governs the three sequence tables at some point of a frame: mode (0 predefined, 1 RLE, 2 FSE description, 3 nothing yet) and
// where the description starts (offset in the compressed entry)
struct ZpjTabs { u32 mode[3], off[3]; };

// One block of a Zstandard frame at p (avail bytes follow): 1 = parsed into B (hdr_off = at; sizes, literals and sequence headers; nothing
// about trees or slots), 0 = the bytes end inside it, -1 = not a block this path takes (reserved type, Repeat_Mode table, sizes that
// disagree).  *last = its Last_Block bit, *total = 3 + the bytes of its body.
// tabs != nullptr: Repeat_Mode tables are taken — resolved against *tabs, which is updated with what this block defines.
ZPK_HD static int zpj_parse_block(const u8* p, u64 avail, u64 at, ZpjBlock& B, u32* last, u64* total, ZpjTabs* tabs = nullptr)
{
    if (avail < 3) return 0;
    const u32 bh = (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16);
    const u32 bt = (bh >> 1) & 3, bs = bh >> 3;
    *last = bh & 1;
    memset(&B, 0, sizeof(B));
    B.hdr_off = (u32)at; B.type = bt; B.size = bs; B.tree_src = ZPJ_NONE;
    if (bt == 3 || bs > ZPJ_BLOCK || at > 0x7FFFFF00ull) return -1;
    const u64 body = bt == 1 ? 1 : bs;
    *total = 3 + body;
    if (avail - 3 < body) return 0;
    if (bt != 2) return 1;
    const u8* const b = p + 3;
    if (bs < 3) return -1;
    const u32 b0 = b[0], lt = b0 & 3, fmt = (b0 >> 2) & 3;
    u32 hl, regen, csize;
    if (lt < 2) {
        if ((fmt & 1) == 0) { hl = 1; regen = b0 >> 3; }
        else if (fmt == 1) { hl = 2; regen = (b0 >> 4) | ((u32)b[1] << 4); }
        else { hl = 3; regen = (b0 >> 4) | ((u32)b[1] << 4) | ((u32)b[2] << 12); }
        csize = lt == 0 ? regen : 1u;
    } else {
        if (bs < 5) return -1;
        const u64 v = hrd32(b);
        if (fmt < 2) { hl = 3; regen = (u32)(v >> 4) & 0x3FF; csize = (u32)(v >> 14) & 0x3FF; }
        else if (fmt == 2) { hl = 4; regen = (u32)(v >> 4) & 0x3FFF; csize = (u32)(v >> 18); }
        else { hl = 5; regen = (u32)(v >> 4) & 0x3FFFF; csize = (u32)(v >> 22) | ((u32)b[4] << 10); }
    }
    if (regen > ZPJ_BLOCK || (u64)hl + csize > bs) return -1;
    B.lit_type = lt; B.lit_size = regen; B.lit_used = hl + csize;
    if (lt < 2) B.lit_ref = (u32)(at + 3 + hl);
    u64 o = B.lit_used;
    if (bs - o < 1) return -1;
    u64 nseq = b[o];
    if (nseq == 0) { if (bs - o != 1) return -1; }
    else {
        if (nseq < 128) o += 1;
        else if (nseq < 255) { if (bs - o < 2) return -1; nseq = ((nseq - 128) << 8) + b[o + 1]; o += 2; if (nseq == 0) return -1; /* tables without sequences */ }
        else { if (bs - o < 3) return -1; nseq = (u64)b[o + 1] + ((u64)b[o + 2] << 8) + 0x7F00; o += 3; }
        if (bs - o < 1) return -1;
        const u32 modes = b[o];
        const bool any_repeat = ((modes >> 6) & 3) == 3 || ((modes >> 4) & 3) == 3 || ((modes >> 2) & 3) == 3;
        if ((modes & 3) || (any_repeat && !tabs)) return -1;
        B.tab_modes = 0x3F;
        if (tabs) {
            // the three descriptions follow the modes byte in the order LL, OF, ML; each is measured so that the next one's start — and
            // what a later Repeat_Mode block inherits — is known
            u64 q = o + 1;
            for (int kind = 0; kind < 3; kind++) {                     // (T_LL, T_OF, T_ML of zstd_wg.h)
                const u32 mode = (modes >> (6 - 2 * kind)) & 3;
                if (mode == 3) {
                    if (tabs->mode[kind] == 3) return -1;              // nothing to repeat
                } else {
                    tabs->mode[kind] = mode; tabs->off[kind] = (u32)(at + 3 + q);
                    if (mode == 1) { if (bs - q < 1) return -1; q += 1; }
                    else if (mode == 2) { const int n = zpj_ncount_len(b + q, bs - q, kind == 0 ? 35 : (kind == 1 ? 31 : 52), kind == 1 ? 8 : 9); if (n < 0) return -1; q += (u64)n; }
                }
                B.tab_off[kind] = tabs->off[kind];
                B.tab_modes = (B.tab_modes & ~(3u << (2 * kind))) | (tabs->mode[kind] << (2 * kind));
            }
        }
    }
    B.nseq = (u32)nseq;
    return 1;
}

// The header of a Zstandard frame as ZSTD_compressCCtx writes it (lib/zpack_write.c:179): no dictionary, no checksum, a window of at
// most 2^max_wlog bytes.  -> its size (0: the bytes end inside it, -1: not this path's); *window = Window_Size, *fcs = content size or ~0.
ZPK_HD static int zpj_parse_frame_header(const u8* p, u64 avail, u32 max_wlog, u64* window, u64* fcs)
{
    if (avail < 6) return 0;
    if (hrd32(p) != 0xFD2FB528u) return -1;
    u64 q = 4;
    const u32 fhd = p[q++];
    const u32 fcs_flag = fhd >> 6, single = (fhd >> 5) & 1;
    if (fhd & 0x0F) return -1;                                      // reserved bit, content checksum, dictionary: the one-wave decoder's
    *window = 0;
    if (!single) {
        const u32 wdesc = p[q++], wlog = 10 + (wdesc >> 3);
        if (wlog > max_wlog) return -1;
        *window = (1ull << wlog) + ((1ull << wlog) >> 3) * (wdesc & 7);
    }
    const u32 fn = fcs_flag == 0 ? (single ? 1u : 0u) : (fcs_flag == 1 ? 2u : (fcs_flag == 2 ? 4u : 8u));
    if (avail - q < fn) return 0;
    *fcs = ~0ull;
    if (fn) { u64 v = 0; for (u32 i = 0; i < fn; i++) v |= (u64)p[q + i] << (8 * i); if (fn == 2) v += 256; *fcs = v; q += fn; }
    if (single) *window = *fcs;
    return (int)q;
}

// The place of a parsed block in its block table, where it becomes entry `index`: a compressed block gets its sequence slots (nseq + 1
// from `slots` on), its room in the literal arena (`lit_total`) and, Treeless, the block whose tree it uses.  tree = the last table entry
// whose literals carry a Huffman tree so far (ZPJ_NONE: none), kept up to date here.  false: a Treeless block with no tree in front of it.
ZPK_HD static inline bool zpj_place_block(ZpjBlock& B, u32 index, u32& tree, u64& slots, u64& lit_total)
{
    if (B.type != 2) return true;
    if (B.lit_type == 2) tree = index;
    if (B.lit_type == 3) { if (tree == ZPJ_NONE) return false; B.tree_src = tree; }
    if (B.lit_type >= 2) { B.lit_base = (u32)lit_total; lit_total += ((u64)B.lit_size + 15) / 16 * 16 + 64; }
    B.seq_base = (u32)slots;
    slots += (u64)B.nseq + 1;
    return true;
}

// ONE Zstandard frame as ZSTD_compressCCtx writes it (lib/zpack_write.c:179): no dictionary, no checksum, its content size (if stated) the
// entry's, a window of at most 128 MiB, no Repeat_Mode table, every Treeless block behind a block with a tree, >= ZPK_PJ_MIN_BLOCKS
// blocks, nothing behind the last block -> the block table of zstd_pj.h.  slots = sequence slots (a block owns nseq + 1), lit_total =
// bytes of the literal arena.
template <class Sink> ZPK_HD static bool walk_zstd_single_to(const u8* p, u64 comp, u64 uncomp, Sink& blocks, u64& slots, u64& lit_total)
{
    slots = 0; lit_total = 0;
    u64 window = 0, fcs = ~0ull;
    const int hdr = zpj_parse_frame_header(p, comp, 27, &window, &fcs);
    if (hdr <= 0 || (fcs != ~0ull && fcs != uncomp)) return false;
    u64 q = (u64)hdr;
    u32 tree = ZPJ_NONE;
    ZpjTabs tabs; for (int k = 0; k < 3; k++) { tabs.mode[k] = 3; tabs.off[k] = 0; }
    for (;;) {
        ZpjBlock B; u32 last = 0; u64 total = 0;
        if (zpj_parse_block(p + q, comp - q, q, B, &last, &total, &tabs) != 1) return false;
        if (!zpj_place_block(B, (u32)blocks.size(), tree, slots, lit_total)) return false;
        if (!blocks.push(B)) return false;
        q += total;
        if (last) break;
        if (slots > 0x7FFFFF00ull || lit_total > 0x70000000ull) return false;
    }
    if (q != comp || blocks.size() < ZPK_ZPJ_MIN_BLOCKS) return false;
    return comp + lit_total + 1024 < 0x7FFFFF00ull;
}
static bool walk_zstd_single(const u8* p, u64 comp, u64 uncomp, std::vector<ZpjBlock>& blocks, u64& slots, u64& lit_total)
{
    blocks.clear();
    WalkVec<ZpjBlock> sink{ blocks };
    return walk_zstd_single_to(p, comp, uncomp, sink, slots, lit_total);
}
// ... into tab[0, capacity), like walk_lz4_single_into
ZPK_HD static bool walk_zstd_single_into(const u8* p, u64 comp, u64 uncomp, ZpjBlock* tab, u32 capacity, u32* nblocks, u64* slots, u64* lit_total)
{
    WalkTab<ZpjBlock> sink{ tab, capacity, 0 };
    u64 sl = 0, lt = 0;
    const bool ok = walk_zstd_single_to(p, comp, uncomp, sink, sl, lt);
    *nblocks = ok ? sink.n : 0; *slots = sl; *lit_total = lt;
    return ok;
}

}  // namespace zpk
