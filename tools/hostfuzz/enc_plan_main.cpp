// zpack_amd/csrc/enc_plan.h, the header the codec compiles, under ASan + UBSan: the piece plan over the sizes and options at which it can
// go wrong, the frame envelope against bytes written out here from the two format specifications (and through the header parsers of
// host_walk.h), the verdict as a table.  Built and run by tools/hostfuzz/run_enc_plan.sh
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "enc_plan.h"
#include "host_walk.h"
using namespace zpk;

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static const u64 PIECE = 512u << 10;

// the pieces of one entry appended behind a layout that already holds something: every property of the plan
static u64 check_entry(u64 split_min, u32 method, u64 size, u64 base, u64& out_total, u64& max_cap_io)
{
    zpk_encode_desc d; memset(&d, 0, sizeof(d));
    d.src_offset = 0x1234; d.size = size; d.dst_offset = 0x777; d.dst_capacity = 99 + size / 3; d.method = method; d.level = 3;
    const bool want_split = size >= split_min && size > PIECE && method <= 2;                // the rule, stated once more
    CHECK(enc_is_split(split_min, d) == want_split);
    const u64 pieces = enc_piece_count(split_min, d);
    CHECK(pieces == (want_split ? (size + PIECE - 1) / PIECE : 1));
    std::vector<zpk_encode_desc> out(pieces + 1);
    memset(&out[pieces], 0xA5, sizeof(zpk_encode_desc));                                      // the element behind the last stays as it is
    const zpk_encode_desc guard = out[pieces];
    const u64 out_before = out_total, cap_before = max_cap_io;
    const EncSpan sp = enc_emit_entry(split_min, d, base, out.data(), out_total, max_cap_io);
    CHECK(memcmp(&out[pieces], &guard, sizeof(guard)) == 0);
    CHECK(sp.off == base && sp.len == size);
    u64 at = base, slot = out_before, max_cap = cap_before;
    for (u64 j = 0; j < pieces; j++) {
        const zpk_encode_desc& p = out[j];
        CHECK(p.src_offset == at && p.level == d.level);                                       // in order, no gap, no overlap
        if (want_split) {
            CHECK(p.size == (j + 1 < pieces ? PIECE : size - j * PIECE) && p.size >= 1 && p.size <= PIECE);
            CHECK(p.dst_capacity == enc_compress_bound(method, p.size));
            CHECK(p.method == (method | ZPK_EF_PIECE));
        } else {
            CHECK(p.size == size && p.dst_capacity == d.dst_capacity && p.method == method);
        }
        CHECK(p.dst_offset == slot && (p.dst_offset & 255) == 0);                              // 256-aligned, ascending, disjoint
        slot = p.dst_offset + ((p.dst_capacity + 255) & ~255ull);
        CHECK(slot >= p.dst_offset + p.dst_capacity);
        if (p.dst_capacity > max_cap) max_cap = p.dst_capacity;
        at += p.size;
    }
    CHECK(at == base + size);                                                                   // the pieces tile [base, base + size)
    CHECK(out_total == slot && max_cap_io == max_cap);
    return pieces;
}

static void check_envelope(u32 method, u64 content, const u8* hdr, u32 hl, const u8* trl, u32 tl)
{
    const EncEnvelope e = enc_envelope(method, content);
    CHECK(e.hl == hl && e.tl == tl);
    CHECK(memcmp(e.hdr, hdr, hl) == 0 && memcmp(e.trl, trl, tl) == 0);
    for (u32 i = hl; i < sizeof(e.hdr); i++) CHECK(e.hdr[i] == 0);
    for (u32 i = tl; i < sizeof(e.trl); i++) CHECK(e.trl[i] == 0);
    if (method == ZPK_METHOD_LZ4) {
        int independent = -1, has_cs = -1; u64 cs = 1;
        CHECK(lz4_single_header(e.hdr, e.hl, &independent, &has_cs, &cs) == (int)hl);
        CHECK(independent == 0 && has_cs == 0 && cs == 0);
    } else if (method == ZPK_METHOD_ZSTD) {
        u64 window = 0, fcs = 0;
        CHECK(zpj_parse_frame_header(e.hdr, e.hl, 27, &window, &fcs) == (int)hl);
        CHECK(window == 65536 && fcs == content);                                               // (not known: ~0 on both sides)
        u8 blk[3]; memcpy(blk, e.trl, 3);
        ZpjBlock B; u32 last = 0; u64 total = 0;
        CHECK(zpj_parse_block(blk, 3, 0, B, &last, &total) == 1 && last == 1 && total == 3 && B.type == 0 && B.size == 0);
    }
}

int main()
{
    // ---- the plan ----
    const u64 sizes[] = { 0, 1, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE, 3 * PIECE + 17, 2ull << 20, 0xFFFFFFFFull, 1ull << 32, (1ull << 32) + PIECE + 1 };
    const u64 split_mins[] = { 1, 2ull << 20, ~0ull };
    u64 entries = 0, pieces = 0, split = 0;
    for (u64 split_min : split_mins) {
        u64 out_total = 0, max_cap = 0;                                                          // one layout across all entries of an option: slots of different entries stay disjoint too
        u64 base = 13;
        for (u32 method = 0; method <= 2; method++) for (u64 size : sizes) {
            const u64 np = check_entry(split_min, method, size, base, out_total, max_cap);
            entries++; pieces += np; split += np > 1;
            base += size + 16;
        }
    }
    { zpk_encode_desc d; memset(&d, 0, sizeof(d)); d.size = 4 * PIECE; d.method = 3; CHECK(!enc_is_split(1, d) && enc_piece_count(1, d) == 1); }   // an unknown method is never split
    printf("plan: %llu entries, %llu split, %llu pieces: split exactly by the rule, pieces tile their entry, slots aligned and disjoint\n",
           (unsigned long long)entries, (unsigned long long)split, (unsigned long long)pieces);

    // ---- the bound's values at the sizes the plan uses (tests/test_abi_cpu.py pins the exported function) ----
    CHECK(enc_compress_bound(ZPK_METHOD_NONE, PIECE) == PIECE && enc_compress_bound(3, 100) == 0);
    CHECK(enc_compress_bound(ZPK_METHOD_LZ4, PIECE) == 8 * 8 + PIECE + 8 && enc_compress_bound(ZPK_METHOD_LZ4, 0) == 8 + 65535 + 8);
    CHECK(enc_compress_bound(ZPK_METHOD_ZSTD, PIECE) == PIECE + (PIECE >> 8) && enc_compress_bound(ZPK_METHOD_ZSTD, 0) == 64);

    // ---- the envelope ----
    const u8 l4_hdr[] = { 0x04, 0x22, 0x4D, 0x18, 0x40, 0x40, 0xC0 }, l4_end[] = { 0x00, 0x00, 0x00, 0x00 };
    const u8 zs_small[] = { 0x28, 0xB5, 0x2F, 0xFD, 0x80, 0x30, 0x01, 0x00, 0x08, 0x00 };
    const u8 zs_4g[] = { 0x28, 0xB5, 0x2F, 0xFD, 0xC0, 0x30, 0x00, 0x00, 0x00, 0x00, 0x01, 0x00, 0x00, 0x00 };
    const u8 zs_unknown[] = { 0x28, 0xB5, 0x2F, 0xFD, 0x00, 0x30 }, zs_end[] = { 0x01, 0x00, 0x00 };
    check_envelope(ZPK_METHOD_LZ4, 0x80001, l4_hdr, 7, l4_end, 4);
    check_envelope(ZPK_METHOD_LZ4, 1ull << 32, l4_hdr, 7, l4_end, 4);
    check_envelope(ZPK_METHOD_LZ4, ZPK_ENC_SIZE_UNKNOWN, l4_hdr, 7, l4_end, 4);
    check_envelope(ZPK_METHOD_ZSTD, 0x80001, zs_small, 10, zs_end, 3);
    check_envelope(ZPK_METHOD_ZSTD, 1ull << 32, zs_4g, 14, zs_end, 3);
    check_envelope(ZPK_METHOD_ZSTD, ZPK_ENC_SIZE_UNKNOWN, zs_unknown, 6, zs_end, 3);
    { const u8 top[] = { 0x28, 0xB5, 0x2F, 0xFD, 0x80, 0x30, 0xFF, 0xFF, 0xFF, 0xFF }; check_envelope(ZPK_METHOD_ZSTD, 0xFFFFFFFFull, top, 10, zs_end, 3); }   // the last size of four bytes
    check_envelope(ZPK_METHOD_NONE, 0x80001, zs_end, 0, zs_end, 0);                             // (no byte of either is looked at)
    check_envelope(ZPK_METHOD_NONE, ZPK_ENC_SIZE_UNKNOWN, zs_end, 0, zs_end, 0);
    printf("envelope: LZ4, Zstandard with 4 and 8 bytes of content size and with none, stored: the bytes of the specifications, accepted by the header parsers\n");

    // ---- the verdict ----
    const u64 H = 0x1122334455667788ull;
    for (u32 method = 0; method <= 2; method++) {
        const EncEnvelope e = enc_envelope(method, 3 * PIECE + 17);
        const u64 blocks = 1000003, frame = e.hl + blocks + e.tl;
        zpk_encode_result r = enc_verdict(nullptr, blocks, e.hl, e.tl, frame, method, H);           // fits exactly
        CHECK(r.status == 0 && r.detail == 0 && r.comp_size == frame && r.hash == H);
        r = enc_verdict(nullptr, blocks, e.hl, e.tl, frame + 1, method, H);
        CHECK(r.status == 0 && r.detail == 0 && r.comp_size == frame && r.hash == H);
        r = enc_verdict(nullptr, blocks, e.hl, e.tl, frame - 1, method, H);                         // one byte less
        CHECK(r.status == (method == ZPK_METHOD_NONE ? 12 : 14) && r.detail == 0 && r.comp_size == 0 && r.hash == 0);
        r = enc_verdict(nullptr, blocks, e.hl, e.tl, 0, method, H);
        CHECK(r.status == (method == ZPK_METHOD_NONE ? 12 : 14) && r.detail == 0 && r.comp_size == 0 && r.hash == 0);
        zpk_encode_result f; f.status = 14; f.detail = 0xBEEF; f.comp_size = 777; f.hash = 5;   // a failing piece: its status and detail, whatever fits
        r = enc_verdict(&f, blocks, e.hl, e.tl, frame, method, H);
        CHECK(r.status == 14 && r.detail == 0xBEEF && r.comp_size == 0 && r.hash == 0);
        f.status = 12; f.detail = 0;
        r = enc_verdict(&f, blocks, e.hl, e.tl, frame - 1, method, H);
        CHECK(r.status == 12 && r.detail == 0 && r.comp_size == 0 && r.hash == 0);
    }
    printf("verdict: a frame that fits exactly, one byte less, a failing piece; every failure with comp_size = hash = 0\n");
    return 0;
}
