// enc_plan.h — an entry written IN PIECES, decided in one place for the three writers: zpk_codec_encode_batch_host and
// zpk_codec_encode_big_device (zpk_encode.inc) and the stream writer (zpk_stream.inc).  Which entries are split, a piece's descriptor and
// slot, the frame's header and end, the entry's verdict.
// Plain C++17, the public header and standard headers only: tools/hostfuzz builds this file with g++ under ASan + UBSan (g++ knows no HIP),
// which keeps it so.  The verdict is also device code (k_big_close): ZPK_HD is empty on a CPU build.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/zpack_codec.h"

#ifdef __HIPCC__
#define ZPK_HD __host__ __device__
#else
#define ZPK_HD
#endif

namespace zpk {

typedef uint8_t  u8;                             // (the typedefs of zpk_device.h)
typedef uint32_t u32;
typedef uint64_t u64;

// Entries of at least `split_min` bytes (zpk_codec::enc_split_min) go to the device as 512 KiB pieces, one wave each.  Round 4 made every
// piece a frame of its own; since round 5 a piece is a run of BLOCKS and the entry is ONE frame — what the reference writer produces
// (lib/zpack_write.c:179, :204-210): the frame header goes in front of the first piece's blocks and the frame is closed behind the last
// one (LZ4: the EndMark; Zstandard: an empty last block), the pieces stay in order.  A piece's first block has no match into the piece
// before it (its table starts empty): 0.1 % of ratio.  The entry's hash is that of the whole plaintext.
#define ZPK_ENC_PIECE (512u << 10)               // a piece: what one wave compresses, a run of blocks of the entry's frame

// zpk_codec_compress_bound (the exported function calls this; tests/test_abi_cpu.py pins its values)
static inline size_t enc_compress_bound(u32 method, size_t n)
{
    switch (method) {
    case ZPK_METHOD_NONE: return n;
    case ZPK_METHOD_ZSTD: {                                                        // >= ZSTD_COMPRESSBOUND(n), room for raw blocks
        size_t zb = n + (n >> 8) + (n < (128u << 10) ? (((128u << 10) - n) >> 11) : 0);
        size_t raw = n + 13 + 3 * (n / (128u << 10) + 1);
        return zb > raw ? zb : raw;
    }
    case ZPK_METHOD_LZ4: {                                                          // LZ4F_compressBound(n, NULL) of lz4 1.9.x
        size_t max_src = n + 65535, full = max_src / 65536, part = max_src & 65535;
        size_t last = n == 0 ? part : 0;
        return 8 * (full + (last > 0)) + 65536 * full + last + 8;
    }
    default: return 0;
    }
}

// ---- the split rule ----------------------------------------------------------------------------------------------------------------
static inline bool enc_is_split(u64 split_min, const zpk_encode_desc& d) { return d.size >= split_min && d.size > ZPK_ENC_PIECE && d.method <= ZPK_METHOD_LZ4; }
static inline u64 enc_piece_count(u64 split_min, const zpk_encode_desc& d) { return enc_is_split(split_min, d) ? (d.size + ZPK_ENC_PIECE - 1) / ZPK_ENC_PIECE : 1; }

// ---- the pieces of one entry -------------------------------------------------------------------------------------------------------
struct EncSpan { u64 off, len; };                // the plaintext of an entry: what its XXH3 is taken over

// Appends the enc_piece_count descriptors of entry d, whose plaintext lies at src_base of the source the pieces are encoded from, to
// `out`: piece j is bytes [j * ZPK_ENC_PIECE, ...) of it with a slot of its own bound and ZPK_EF_PIECE; an entry that is not split is one
// "piece", d itself (its capacity, no flag).  The slots lie back to back, 256-aligned: out_total = the bytes they take so far, max_cap =
// the largest capacity so far.  -> the entry's plaintext.
static inline EncSpan enc_emit_entry(u64 split_min, const zpk_encode_desc& d, u64 src_base, zpk_encode_desc* out, u64& out_total, u64& max_cap)
{
    const bool split = enc_is_split(split_min, d);
    const u64 pieces = enc_piece_count(split_min, d);
    for (u64 j = 0; j < pieces; j++) {
        zpk_encode_desc& p = out[j];
        p = d;
        p.src_offset = src_base + j * ZPK_ENC_PIECE;
        if (split) {
            p.size = j + 1 == pieces ? d.size - j * ZPK_ENC_PIECE : (u64)ZPK_ENC_PIECE;
            p.dst_capacity = enc_compress_bound(d.method, p.size);
            p.method |= ZPK_EF_PIECE;
        }
        p.dst_offset = out_total; out_total += (p.dst_capacity + 255) & ~255ull;
        if (p.dst_capacity > max_cap) max_cap = p.dst_capacity;
    }
    return EncSpan{ src_base, d.size };
}

// ---- the frame around an entry's pieces ---------------------------------------------------------------------------------------------
struct EncEnvelope {
    u32 hl, tl;                                  // bytes of frame header / end of frame (stored entries: 0, 0)
    u8  hdr[16], trl[8];
};
#define ZPK_ENC_SIZE_UNKNOWN (~0ull)             // the stream writer's header: the content size is not known when it goes out

static inline EncEnvelope enc_envelope(u32 method, u64 content_size)
{
    EncEnvelope e;
    memset(&e, 0, sizeof(e));
    if (method == ZPK_METHOD_LZ4) {
        const u8 b[7] = {0x04, 0x22, 0x4D, 0x18, 0x40, 0x40, 0xC0};
        memcpy(e.hdr, b, 7); e.hl = 7;
        e.tl = 4;                                                                  // EndMark: four zero bytes
    } else if (method == ZPK_METHOD_ZSTD) {
        // magic, Frame_Header_Descriptor (content size of 4 or 8 bytes or none, not single-segment), Window_Descriptor 64 KiB (no match of
        // this encoder reaches further, and its blocks are <= 64 KiB), Frame_Content_Size
        const u32 fcs = content_size == ZPK_ENC_SIZE_UNKNOWN ? 0u : (content_size <= 0xFFFFFFFFull ? 4u : 8u);
        const u8 b[6] = {0x28, 0xB5, 0x2F, 0xFD, (u8)((fcs == 0 ? 0u : (fcs == 4 ? 2u : 3u)) << 6), 0x30};
        memcpy(e.hdr, b, 6);
        for (u32 i = 0; i < fcs; i++) e.hdr[6 + i] = (u8)(content_size >> (8 * i));
        e.hl = 6 + fcs;
        e.trl[0] = 0x01; e.tl = 3;                                                 // Last_Block, Raw_Block, Block_Size 0
    }
    return e;
}

// ---- the entry's verdict ------------------------------------------------------------------------------------------------------------
// That of its first failing piece (`failed`; nullptr: none failed), else the frame's length — header + the pieces' blocks + end of frame —
// against what the caller gave.  Every failure leaves comp_size = hash = 0.  (The values are zpack_result's, R_* of zpk_device.h.)
enum : int { ENC_R_OK = 0, ENC_R_BUFFER_TOO_SMALL = 12, ENC_R_COMPRESS_FAILED = 14 };
ZPK_HD static inline zpk_encode_result enc_verdict(const zpk_encode_result* failed, u64 blocks, u32 hl, u32 tl, u64 dst_capacity, u32 method, u64 hash)
{
    zpk_encode_result r; r.status = ENC_R_OK; r.detail = 0; r.comp_size = 0; r.hash = 0;
    if (failed) { r.status = failed->status; r.detail = failed->detail; }
    else if (hl + blocks + tl > dst_capacity) r.status = method == ZPK_METHOD_NONE ? ENC_R_BUFFER_TOO_SMALL : ENC_R_COMPRESS_FAILED;
    else { r.comp_size = hl + blocks + tl; r.hash = hash; }
    return r;
}

}  // namespace zpk
