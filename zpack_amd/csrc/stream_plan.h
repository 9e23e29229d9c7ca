// stream_plan.h — the bounded steps of the stream reader (zpk_stream.inc: dstream_fast_lz4, dstream_fast_zstd), every rule of a step
// that is not a kernel launch, stated once: how many of the caller's bytes a call takes, when a step runs, the sections the XXH3 of
// the output so far is computed in, the history that stays on the device, the two device layouts, the constants, the verdict.
// Plain C++17, host_walk.h / pj_types.h and standard headers only: tools/hostfuzz builds this file with g++ under ASan + UBSan
// (g++ knows no HIP), which keeps it so.  ZPK_HD is empty on a CPU build.
#pragma once
#include <stdint.h>
#include "host_walk.h"                           // pj_types.h: PjBlock, ZpjBlock, PJ_BLOCK, ZPJ_BLOCK, XS_GROUP; ZPK_HD

namespace zpk {

// ---- the constants -----------------------------------------------------------------------------------------------------------------------
#define ZPK_STREAM_MAX_BYTES (1ull << 46)        // sizes derive from what the caller says about the entry: nothing may wrap
#define ZPK_DS_GATHER (256u << 10)               // the windowless step: small chunks are gathered on the host up to this
#define ZPK_DS_FAST_MIN (1ull << 20)             // compressed bytes from which an entry goes in bounded steps
#ifndef ZPK_DS_RESTART
#define ZPK_DS_RESTART 1001
#endif
#define FS_SRC_SLACK 192u                        // = ZPK_SRC_SLACK: what the kernels may read behind a staged image
#define FS_SMALL 256u                            // the region of a zpk_span / a zpk_stream_rec in the layouts (zpk_stream.inc asserts they fit)
// LZ4: steps of up to 64 blocks of 64 KiB behind 128 KiB of history
#define F_BLOCKS 64u
#define F_FIRST_MIN 4u                           // the first step runs from this many blocks on (ZPK_PJ_MIN_BLOCKS: fewer do not earn the fixed cost)
#define F_HIST (128u << 10)
#define F_OUT (F_BLOCKS * PJ_BLOCK)
#define F_IN (F_BLOCKS * (PJ_BLOCK + 4u) + 256u)
#define F_HOST_OUT (8ull << 20)                  // the pinned buffer a step's output comes home in (the larger of the two step sizes)
#define F_LOOK 12u                               // pointer-doubling rounds between two looks at the flags
// Zstandard: steps of up to 64 blocks of 128 KiB behind the frame's window
#define FZ_BLOCKS 64u
#define FZ_FIRST_MIN 2u                          // (ZPK_ZPJ_MIN_BLOCKS)
#define FZ_CHUNK 16u
#define FZ_OUT ((u64)FZ_BLOCKS * ZPJ_BLOCK)
#define FZ_MAX_WLOG 23u
#define FZ_TABDESC 192u                          // bytes kept of an FSE table description (53 symbols at accuracy 9 take < 100)
#define FZ_DESC_BYTES 56u                        // = sizeof(zpk_decode_desc) (zpk_stream.inc asserts it)
#define FZ_LOOK 14u
static_assert(FZ_OUT <= F_HOST_OUT && F_OUT <= F_HOST_OUT, "a step's output fits the pinned buffer");

// ---- intake: the caller's bytes (never more than the entry still has) ---------------------------------------------------------------------
// rc 21 (STREAM_INVALID): comp_size lies below what was already taken; 10 (MALLOC_FAILED): a size no device holds, as the windowless
// path answers it
struct StreamIntake { int rc; u64 take; };
ZPK_HD static inline StreamIntake stream_intake(u64 comp_size, u64 in_total, u64 in_size)
{
    if (comp_size < in_total) return StreamIntake{ 21, 0 };
    if (comp_size > ZPK_STREAM_MAX_BYTES) return StreamIntake{ 10, 0 };
    const u64 want = comp_size - in_total;
    return StreamIntake{ 0, in_size < want ? in_size : want };
}
// the capacity the pending buffer needs for `take` more bytes (unchanged while they fit; else what is needed + 1 MiB)
ZPK_HD static inline u64 stream_pend_cap(u64 pend_len, u64 pend_cap, u64 take) { return pend_len + take > pend_cap ? pend_len + take + (1u << 20) : pend_cap; }

// ---- go: a step runs at the end mark, at a full table, or — the first step — from first_min blocks on -----------------------------------------
// end: the scan saw the frame's end; nb: complete blocks among the pending bytes; all_in: every byte of the entry has arrived;
// q_is_all: the blocks (and the end) take every pending byte.  RESTART: the verdict is not the steps' to give.
enum StreamGo { STREAM_WAIT = 0, STREAM_RUN = 1, STREAM_RESTART = 2 };
ZPK_HD static inline StreamGo stream_go(bool end, u32 nb, u32 table, u32 first_min, u64 f_T, bool all_in, bool q_is_all)
{
    if (end && !(all_in && q_is_all)) return STREAM_RESTART;                             // something follows the end: not one frame
    if (end || nb == table || (f_T == 0 && nb >= first_min)) return STREAM_RUN;
    return all_in ? STREAM_RESTART : STREAM_WAIT;                                        // the entry ends inside a frame / more input
}

// ---- the XXH3 of everything produced so far, in sections of whole 64 KiB groups ----------------------------------------------------------------
// The device window holds positions [f_T - f_hist, T_new) of the output at d_out: position p lies at virt + p, virt = d_out - virt_back.
// The partial sums of groups [g_from, g_to) lie at the partials region's start: group g at part_v + g * XS_GROUP * 8 (u64s),
// part_v = d_part - part_back.  The chain takes blocks [b_from, b_to) of 1 KiB; the launch with last != 0 finishes the hash (the block
// with the last byte, the tail) and reads up to 64 bytes in front of the last stripe.
// one_shot: the entry ends in its first step — k_stream_hash over d_out, nothing else.
struct StreamHash {
    bool one_shot, span_up, partials, chain;     // span_up: the span record goes up (always with the chain)
    u64 g_from, g_to, b_from, b_to; int last;
    u64 virt_back, part_back;                    // bytes / u64s
    u64 ghashed_new;
};
ZPK_HD static inline StreamHash stream_hash_plan(u64 f_T, u64 f_hist, u64 T_new, u64 f_ghashed, bool end)
{
    StreamHash h = {};
    h.virt_back = f_T - f_hist; h.ghashed_new = f_ghashed; h.g_from = h.g_to = f_ghashed;
    if (end && f_ghashed == 0 && f_T == 0) { h.one_shot = true; return h; }
    const u64 nblk = T_new ? (T_new - 1) >> 10 : 0;                                      // the block with the last byte belongs to the chain's finish
    h.g_to = end ? (nblk + XS_GROUP - 1) / XS_GROUP : nblk / XS_GROUP;
    if (!(h.g_to > f_ghashed || end)) { h.g_to = f_ghashed; return h; }
    h.span_up = h.chain = true;
    h.partials = h.g_to > f_ghashed;
    h.part_back = f_ghashed * (XS_GROUP * 8);
    h.b_from = f_ghashed * XS_GROUP; h.b_to = h.g_to * XS_GROUP; h.last = end ? 1 : 0;
    if (!end) h.ghashed_new = h.g_to;
    return h;
}

// ---- the history carry: the last min(have, cap) bytes of [history | step] stay at the window's start ------------------------------------------
struct StreamCarry { bool move; u64 from, keep, hist_new; };     // move: `keep` bytes from d_out + from to d_out (through the temporary)
ZPK_HD static inline StreamCarry stream_carry(u64 f_hist, u64 step_out, u64 cap, bool end)
{
    if (end || !step_out) return StreamCarry{ false, 0, f_hist, f_hist };
    const u64 have = f_hist + step_out, keep = have < cap ? have : cap;
    return StreamCarry{ have > keep, have - keep, keep, keep };
}

// ---- the verdict: lib/zpack_read.c:631-637, with the last byte; the bytes stay --------------------------------------------------------------
ZPK_HD static inline int stream_verdict(u64 got, u64 expect) { return got == expect ? 0 : 15; /* ZPACK_ERROR_FILE_HASH_MISMATCH */ }

// ---- the device block of an LZ4 step: fixed, ~40 MiB whatever the entry's size --------------------------------------------------------------
struct FastLayout { u64 in, out, tmp, S, recs, masks, blocks, flags, part, span, hash, state, rec, size; };
ZPK_HD static inline u64 fs_take(u64& o, u64 n) { const u64 at = o; o += (n + 255) & ~255ull; return at; }
ZPK_HD static inline u64 fs_part_bytes(u64 window) { return (window / 65536 + 4) * 4096; }     // partial sums of a window's groups: 4 KiB per group
ZPK_HD static inline FastLayout dstream_fast_layout()
{
    FastLayout L; u64 o = 0;
    L.in = fs_take(o, F_IN + FS_SRC_SLACK); L.out = fs_take(o, F_HIST + F_OUT + 64); L.tmp = fs_take(o, F_HIST); L.S = fs_take(o, ((u64)F_HIST + F_OUT) * 4 + 64);
    L.recs = fs_take(o, (u64)F_BLOCKS * (PJ_BLOCK / 3 + 2 + 8) * 8); L.masks = fs_take(o, (u64)F_BLOCKS * (PJ_BLOCK / 8)); L.blocks = fs_take(o, F_BLOCKS * sizeof(PjBlock));
    L.flags = fs_take(o, 256); L.part = fs_take(o, fs_part_bytes((u64)F_HIST + F_OUT)); L.span = fs_take(o, FS_SMALL); L.hash = fs_take(o, 64); L.state = fs_take(o, 64);
    L.rec = fs_take(o, FS_SMALL); L.size = o;
    return L;
}

// ---- the device blocks of a Zstandard step ---------------------------------------------------------------------------------------------------
// The scratch (d_f, sized by the step): nt table entries, `slots` sequence slots, src_total bytes of [descriptions | tree block | blocks |
// literal arena].  What persists (d_fo, sized by the frame's window HC): [history | a step's output | 64] [temporary of the carry: HC]
// [state 64 | hash 64 | span 128 | rec 256 | flags 512].
ZPK_HD static inline u64 fz_hist_cap(u64 window) { return (window < F_HIST ? (u64)F_HIST : window + 255) & ~255ull; }
ZPK_HD static inline bool fz_window_ok(u64 window) { return window <= (1ull << FZ_MAX_WLOG) + (1ull << (FZ_MAX_WLOG - 3)) * 7; }     // (a single-segment frame: its window is its content size)
struct FzLayout {
    u64 in, zb, pb, desc, list, state, rep, recs, pos, masks, S, part, size;             // offsets in d_f; size: what the scratch takes
    u64 out, tmp, p_state, p_hash, p_span, p_rec, p_flags, fo_need;                      // offsets in d_fo
};
ZPK_HD static inline FzLayout dstream_fz_layout(u64 nt, u64 slots, u64 src_total, u64 HC)
{
    FzLayout L; u64 o = 0;
    L.in = fs_take(o, src_total + FS_SRC_SLACK); L.zb = fs_take(o, nt * sizeof(ZpjBlock)); L.pb = fs_take(o, nt * sizeof(PjBlock));
    L.desc = fs_take(o, nt * FZ_DESC_BYTES); L.list = fs_take(o, nt * 4); L.state = fs_take(o, nt * 4); L.rep = fs_take(o, nt * 12);
    L.recs = fs_take(o, (slots + 64) * 8); L.pos = fs_take(o, (slots + 64) * 8); L.masks = fs_take(o, nt * (ZPJ_BLOCK / 8));
    L.S = fs_take(o, (u64)FZ_CHUNK * ZPJ_BLOCK * 4 + 64); L.part = fs_take(o, fs_part_bytes(HC + FZ_OUT)); L.size = o;
    L.out = 0; L.tmp = HC + FZ_OUT + 64;
    L.p_state = L.tmp + HC; L.p_hash = L.p_state + 64; L.p_span = L.p_state + 128; L.p_rec = L.p_state + 256; L.p_flags = L.p_state + 512;
    L.fo_need = L.p_state + 1024;
    return L;
}
ZPK_HD static inline u64 fz_scratch_alloc(u64 size) { return size + size / 4; }          // a larger step to come does not allocate again

}  // namespace zpk
