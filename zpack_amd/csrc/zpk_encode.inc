// zpk_encode.inc — batch encode + hash entry points and kernels (included by zpk_codec.hip).
//
// Replaces zpack_compress_file + the XXH3 of zpack_add_written_file_entry (lib/zpack_write.c:161-260):
//   NONE  copy
//   LZ4   LZ4 frame with the reference writer's layout (`04 22 4D 18 40 40 C0`, 64 KiB blocks, EndMark;
//         lib/zpack_write.c:199-211): one wave per entry, blocks in sequence.  Per 64-position chunk every
//         lane hashes its 4-byte window into a per-wave LDS table (candidates are read before the chunk's
//         own positions are inserted, so a candidate always precedes its position), verifies and extends
//         its match 8 bytes at a time; the greedy parse over the chunk is then a short wave-uniform loop
//         over the ballot of usable matches, and each chosen sequence is emitted cooperatively.  Blocks
//         that do not shrink are stored (bit 31), exactly like LZ4F_makeBlock.
//   ZSTD  a single-segment frame (`28 B5 2F FD`, Frame_Content_Size, no checksum — the header flavour of
//         ZSTD_compressCCtx, lib/zpack_write.c:179) of 64 KiB blocks.  Each block is parsed by the same
//         lane-parallel match finder as LZ4 into a sequence list (matches may reach into the previous blocks of the
//         entry), then written as a Compressed_Block: literals Huffman-coded in four streams (direct or FSE-compressed
//         weight description) or Raw, sequences FSE-coded over per-block tables (RLE_Mode / FSE_Compressed_Mode with
//         the table description) or the predefined distributions, whichever is estimated smaller; RLE block when the
//         block is one byte, Raw when nothing shrinks.  Repeat-offset codes (offset value 1 only) on blocks of binary data, where the match
//         finder also tries the previous match's offset (round 3); a forward pass that only re-codes the offsets a plain hash finder
//         happened to repeat gained nothing (measured twice).  Compressed bytes are unpinned by the reference (tests/write_archive.c
//         checks return codes only); every frame is checked against stock libzstd and this codec's own decoder.

#define ZPK_ENC_GRID_MAX 7168u          // 28 workgroups per CU
#ifndef ZE_WAVES_PER_SIMD
#define ZE_WAVES_PER_SIMD 5               // k_encode<12>: register budget (96 VGPRs); 8 KiB of LDS = 7 allocation units: 18 workgroups per CU
#endif
#define LZ4E_HASH_LOG 12                // levels <= 2: 8 KiB of LDS per workgroup (k_encode<12>)
#define LZ4E_HASH_LOG_MID 13            // levels 3..5: 16 KiB, 9 workgroups per CU (k_encode<13>) — the CLI's default level 3 lives here
#define LZ4E_HASH_LOG_HC 14             // levels >= 6: 32 KiB — four times the match candidates of <12>, 4 workgroups per CU (k_encode<14>)
// (round 4, 2000 x 1 MiB at level 3, 2^14 -> 2^13 slots: text zstd 33.0 -> 59.7 GiB/s at ratio 0.336 -> 0.347, text LZ4 46.4 -> 80.3 at
// 0.462 -> 0.486, records zstd 23.7 -> 40.4 at 0.503 -> 0.507 (profiles/r04/r04_enc_level3_table_ab.txt): twice the workgroups per CU
// are worth more to the default level than the last 3 % of ratio; levels >= 6 keep the large table and the two-candidate parse.)
#ifndef ZE_MINMATCH
#define ZE_MINMATCH 6u
#endif
#define LZ4E_MFLIMIT 12u
#define LZ4E_LASTLIT 5u

// seqring: the Zstandard sequence list of a block is staged here and written out in bursts (round 3).  A store per chunk made every
// chunk's first load wait for a STORE round trip — loads and stores share the wave's vmcnt and the compiler waits for both (measured,
// 6000 x 1 MiB text: the chunk loop alone 18.8 ms, with its sequence stores 65.0).  768 bytes: the table's 8 KiB took seven LDS
// allocation units of 1280 bytes anyway.
#define LZ4E_SEQRING 96u
#ifndef LZ4E_CHUNKS
#define LZ4E_CHUNKS 4                   // chunks of 64 positions per trip of the match finder in k_encode<12> (96 VGPRs).  Measured on C5: 1 / 2 / 3 / 4 / 6 / 8 chunks = 79.0 / 87.6 / 89.8 / 91-92 / 85.2 / 67.0 GiB/s
#endif
#ifndef LZ4E_CHUNKS_HC
#define LZ4E_CHUNKS_HC 4                // chunks of 64 positions per trip of the match finder in k_encode<14> (k_encode<12>: 2)
#endif
template <int HLOG> struct alignas(16) Lz4EncSharedT { u16 table[1 << HLOG]; u64 seqring[LZ4E_SEQRING]; };
typedef Lz4EncSharedT<LZ4E_HASH_LOG> Lz4EncShared;

// The match finder of both formats: lists the sequences of src[0, n) (n <= 65536) in `seqs` (workgroup scratch, ZE_MAXSEQ entries) as
// packed u64 (literal length | match length << 20 | offset << 40; the trailing literals are not listed), their number in nseq_out.
// dst == nullptr (Zstandard): returns where the trailing literals start.  dst != nullptr (LZ4, capacity >= n + 4): the list is
// written as an LZ4 block (lz4e_write_block) and the block's size comes back, or 0 when it does not shrink (the caller stores it).
// effort follows the caller's compression level (lib/zpack_write.c:179 passes it to ZSTD_compressCCtx, :199-201 to LZ4F): 0 = greedy, one
// candidate per position (levels <= 2: "fast"); 1 = the same candidates, LAZY parse — a position whose right neighbour has a match
// that is longer by more than one byte becomes a literal (levels 3-5); 2 = lazy + TWO candidates per hash bucket, the longer match
// wins (levels >= 6).  More effort = a smaller or equal output on the same input (asserted in the tests), never another format.
__device__ __forceinline__ int lz4e_effort(int level) { return level >= 6 ? 2 : (level >= 3 ? 1 : 0); }

// literal runs beyond their first 32 bytes: a lane copies its own run 16 bytes per round trip up to ZE_LANE_LIT bytes; a longer run is
// copied by the whole wave, 1 KiB per round trip (a block with two 30 KiB runs kept two lanes busy for 2 000 dependent round trips each)
#define ZE_LANE_LIT 256u
__device__ __forceinline__ void ze_copy_long_literals(u8* d, const u8* s, u32 ll, bool valid, int lane)
{
    const bool mine = valid && ll > 32u && ll <= ZE_LANE_LIT;
    if (mine) for (u32 c = 32; c < ll; c += 16) gcopy_upto16(d + c, s + c, ll - c);
    u64 lm = __ballot(valid && ll > ZE_LANE_LIT);
    while (lm) {
        const int k = __ffsll((long long)lm) - 1;
        lm &= lm - 1;
        const u32 nk = (u32)__builtin_amdgcn_readlane((int)ll, k);
        u8* const dk = (u8*)readlane_ptr(d, k);
        const u8* const sk = readlane_ptr(s, k);
        for (u32 c = 32u + (u32)lane * 16u; c < nk; c += WAVE * 16u) gcopy_upto16(dk + c, sk + c, nk - c);
    }
}

// LZ4 block out of a sequence list (round 3): lz4e_block lists the block's sequences — the same list the Zstandard writer takes — and
// this writes them 64 at a time: a prefix sum of the encoded sizes places every sequence, each lane writes its own token, length
// bytes, literals and offset.  (The block used to be written sequence by sequence, token and offset by lane 0 and the literals by the
// whole wave: three store round trips and a scalar loop per sequence — LZ4 encode ran at less than half the Zstandard rate.)
// Returns the block's size, or 0 when it would not be smaller than n (the caller stores the block).
__device__ inline u32 lz4e_write_block(const u8* src, u32 n, u8* dst, const u64* seqs, u32 nseq, u32 tail, int lane)
{
    const u32 limit = n - 1;                                               // the block must end strictly below n bytes
    u32 opos = 0, spos = 0;                                                // bytes written / source bytes consumed (uniform)
    for (u32 b0 = 0; b0 < nseq; b0 += WAVE) {
        const u32 k = b0 + (u32)lane;
        const bool valid = k < nseq;
        const u64 q = valid ? ((const ZPK_GLOBAL u64*)seqs)[k] : 0ull;
        const u32 ll = (u32)(q & 0xFFFFFu), ml = (u32)((q >> 20) & 0xFFFFFu), off = (u32)(q >> 40) & 0x7FFFFFu;
        const u32 mlc = valid ? ml - 4u : 0u;
        const u32 lle = ll >= 15u ? (ll - 15u) / 255u + 1u : 0u, mle = mlc >= 15u ? (mlc - 15u) / 255u + 1u : 0u;
        const u32 sz = valid ? 1u + lle + ll + 2u + mle : 0u;
        const u32 xo = wave_scan_add(sz), xs = wave_scan_add(ll + ml);
        const u32 tot = (u32)__builtin_amdgcn_readlane((int)xo, 63);
        if (opos + tot > limit) return 0;
        const u8* const s = src + spos + (xs - (ll + ml));
        u8* o = dst + opos + (xo - sz);
        const u32 nl = ll < 32u ? ll : 32u;
        Copy32 c; c.lo.lo = c.lo.hi = c.hi.lo = c.hi.hi = 0;
        if (valid) c = gload_wide32(s, nl, s + 16 <= src + n);             // (the literal loads of all lanes before the first store)
        u8* lit_o = o;
        if (valid) {
            st8(o, (u8)(((ll >= 15u ? 15u : ll) << 4) | (mlc >= 15u ? 15u : mlc)));
            o += 1;
            if (ll >= 15u) { u32 r = ll - 15u; while (r >= 255u) { st8(o++, 255); r -= 255u; } st8(o++, (u8)r); }
            gstore_wide32(o, c, nl);
            lit_o = o;
            o += ll;
            st8(o, (u8)off); st8(o + 1, (u8)(off >> 8));
            o += 2;
            if (mlc >= 15u) { u32 r = mlc - 15u; while (r >= 255u) { st8(o++, 255); r -= 255u; } st8(o, (u8)r); }
        }
        ze_copy_long_literals(lit_o, s, ll, valid, lane);
        opos += tot;
        spos += (u32)__builtin_amdgcn_readlane((int)xs, 63);
    }
    // the last sequence: literals only
    const u32 ll = n - tail;
    const u32 lle = ll >= 15u ? (ll - 15u) / 255u + 1u : 0u;
    if (opos + 1u + lle + ll > limit) return 0;
    u8* o = dst + opos;
    if (lane == 0) {
        st8(o, (u8)((ll >= 15u ? 15u : ll) << 4));
        if (ll >= 15u) { u32 r = ll - 15u; u8* p = o + 1; while (r >= 255u) { st8(p++, 255); r -= 255u; } st8(p, (u8)r); }
    }
    o += 1u + lle;
    for (u32 i = (u32)lane * 16; i < ll; i += WAVE * 16) gcopy_upto16(o + i, src + tail + i, ll - i);
    return opos + 1u + lle + ll;
}

template <bool B> struct ZeBool { static constexpr bool value = B; };
template <int HLOG>
__device__ inline u32 lz4e_block(Lz4EncSharedT<HLOG>& sh, const u8* src, u32 n, u8* dst, int lane, u64* seqs = nullptr, u32* nseq_out = nullptr,
                                 u32 minmatch = 4u, int effort = 0, u64 abs_base = 0, u32* rep_io = nullptr)
{
    // rep_io != nullptr (Zstandard, blocks of binary data): the REPEAT-OFFSET search.  *rep_io = the offset of the last sequence the frame
    // has emitted so far (Zstandard's repeat offset 1).  Every position also tries the offset of the last match emitted before its trip — one
    // more load per chunk, coalesced, since all lanes look back by the same distance — and a sequence whose offset equals its predecessor's
    // (and that has literals) is flagged in bit 63 of its list word: the block writer codes it as offset value 1 (no extra bits).  Record-
    // like data, where nearly every match sits at the previous match's offset, is what this is for (tools/zstd_param_probe.py).
    const bool use_rep = rep_io != nullptr;
    u32 rep_cur = use_rep ? (u32)__builtin_amdgcn_readfirstlane((int)*rep_io) : 0u;      // offset of the last emitted match (uniform: kept in a scalar register)
    // abs_base = position of the block inside its entry.  The hash table lives on from block to block of an entry: it holds the low
    // 16 bits of (absolute position + 1), a candidate is the nearest earlier position with those bits, so a match may reach up to
    // 65 535 bytes back INTO THE PREVIOUS BLOCKS (LZ4 frames of the reference writer have linked blocks; Zstandard offsets may reach
    // anywhere in the frame).  A stale or aliased slot is just a candidate that fails the byte comparison.
    u32 nseq = 0;
    if (nseq_out) *nseq_out = 0;
    if (HLOG == LZ4E_HASH_LOG) effort = 0;               // (the small table serves levels <= 2 only: the lazy / two-way code is not instantiated there)
    if (n < LZ4E_MFLIMIT + 1) return 0;
    const u32 hist = abs_base > 65536ull ? 65536u : (u32)abs_base;        // bytes of the entry before this block a match may use
    const u32 tag0 = (u32)abs_base & 0xFFFFu;
    if (hist == 0) for (u32 i = lane; i < (1u << HLOG); i += WAVE) sh.table[i] = 0;     // first block of an entry.  0 = empty
    wave_mem_fence();                                      // one wave per workgroup: LDS is in order, no s_waitcnt (a workgroup fence also waits for the global stores)
    const u32 mflimit = n - LZ4E_MFLIMIT;         // last position a match may start at
    const u32 mend = n - LZ4E_LASTLIT;            // matches end at or before this
    u32 anchor = 0, skip_until = 0;
    u32 rn = 0;                                                                 // sequences waiting in sh.seqring (uniform)
    // ---- the stages of one chunk of 64 positions (lane k: position base + k) ----
    // (round 3) every lane reads 16 bytes at its position, not 4: a candidate is then compared over 16 bytes with ONE scattered load, so
    // that a match of up to 16 bytes — nearly all of them on text — is measured in the round trip that used to verify its first 4 bytes only.
    struct Pos { u32 p; bool in, wide; u128 v16; u32 v, h, cand, cand2; };
    struct Cand { u32 d; bool ok; u128 c16; u32 l2; bool diff; };
    // FAST (a uniform property of a trip: every position of both chunks may start a match and has 16 readable bytes — all trips of a
    // block but its last one or two): the loads are UNCONDITIONAL.  A load inside a divergent branch gets its s_waitcnt right there (the
    // value is merged with the other path's), i.e. the second chunk's load would be issued after the first one's has come back.
    auto load_own = [&](Pos& P, u32 pp, auto fast) {
        P.p = pp; P.h = 0; P.cand = 0; P.cand2 = 0;
        if constexpr (decltype(fast)::value) { P.in = true; P.wide = true; P.v16 = ld128(src + pp); P.v = (u32)P.v16.lo; }
        else {
            P.in = pp <= mflimit; P.wide = pp + 16u <= n;                       // (the last positions of a block: 4 bytes)
            P.v16.lo = 0; P.v16.hi = 0; P.v = 0;
            if (P.in) { if (P.wide) { P.v16 = ld128(src + pp); P.v = (u32)P.v16.lo; } else P.v = ld32(src + pp); }
        }
    };
    auto lookup_insert = [&](Pos& P) {                                          // candidates are read before the chunk's own inserts
        if (P.in) {
            P.h = (P.v * 2654435761u) >> (32 - HLOG);
            if (effort >= 2) { P.h &= ~1u; P.cand2 = sh.table[P.h + 1]; }       // bucket = two slots: [newest, the one before]
            P.cand = sh.table[P.h];
        }
        wave_mem_fence();                                      // one wave per workgroup: LDS is in order, no s_waitcnt (a workgroup fence also waits for the global stores)
        if (P.in) {
            if (effort >= 2) sh.table[P.h + 1] = (u16)P.cand;  // (two lanes of a chunk in one bucket: one of them wins each slot — any winner is a valid older position)
            sh.table[P.h] = (u16)(tag0 + P.p + 1u);
        }
        wave_mem_fence();
    };
    auto probe = [&](const Pos& P, u32 cd, Cand& C, auto fast) {                // issue the candidate's load
        C.d = (tag0 + P.p + 1u - cd) & 0xFFFFu;                                 // distance to the nearest earlier position with these low bits
        C.ok = P.in && cd != 0 && C.d != 0 && C.d <= P.p + hist && P.p >= skip_until;
        C.l2 = 0; C.diff = true;
        if constexpr (decltype(fast)::value) C.c16 = ld128(C.ok ? src + P.p - C.d : src);     // (a lane without a candidate reads the block's first bytes: one line for all of them)
        else {
            C.c16.lo = 0; C.c16.hi = 0;
            if (C.ok) { const u8* const cp = src + P.p - C.d; if (P.wide) C.c16 = ld128(cp); else C.c16.lo = (u64)ld32(cp); }
        }
    };
    auto probe_at = [&](const Pos& P, u32 d, Cand& C, auto fast) {              // the candidate at a given distance (the repeat offset: the same for all lanes)
        C.d = d;
        C.ok = P.in && d != 0 && d <= P.p + hist && P.p >= skip_until;
        C.l2 = 0; C.diff = true;
        if constexpr (decltype(fast)::value) C.c16 = ld128(C.ok ? src + P.p - d : src);
        else {
            C.c16.lo = 0; C.c16.hi = 0;
            if (C.ok) { const u8* const cp = src + P.p - d; if (P.wide) C.c16 = ld128(cp); else C.c16.lo = (u64)ld32(cp); }
        }
    };
    auto measure16 = [&](const Pos& P, Cand& C) {                               // the first 16 bytes: registers only
        C.ok = C.ok && (u32)C.c16.lo == P.v;
        C.l2 = 4; C.diff = false;
        if (C.ok && P.wide) {                                                   // first mismatch inside the 16 bytes, or all 16 equal
            const u64 y0 = C.c16.lo ^ P.v16.lo, y1 = C.c16.hi ^ P.v16.hi;
            C.l2 = y0 ? (u32)(__ffsll((long long)y0) - 1) >> 3 : (y1 ? 8u + ((u32)(__ffsll((long long)y1) - 1) >> 3) : 16u);
            C.diff = C.l2 < 16u;
            if (C.l2 > mend - P.p) { C.l2 = mend - P.p; C.diff = true; }        // matches end at or before mend
        }
    };
    auto extend_len = [&](const Pos& P, const Cand& C) -> u32 {                 // longer matches: more round trips, rare.  0 = no match
        if (!C.ok) return 0u;
        u32 l2 = C.l2; bool diff = C.diff;
        const u8* const cp = src + P.p - C.d;
        const u32 pp = P.p;
        // 32 bytes per memory round trip first (the wave waits for its longest match: eight bytes per trip made a 40-byte match
        // five dependent round trips for all 64 lanes), then 8, then single bytes up to the block's match limit
        while (!diff && pp + l2 + 32 <= mend) {
            const u128 a0 = ld128(cp + l2), a1 = ld128(cp + l2 + 16), b0 = ld128(src + pp + l2), b1 = ld128(src + pp + l2 + 16);
            const u64 x0 = a0.lo ^ b0.lo, x1 = a0.hi ^ b0.hi, x2 = a1.lo ^ b1.lo, x3 = a1.hi ^ b1.hi;
            if (x0) { l2 += (u32)(__ffsll((long long)x0) - 1) >> 3; diff = true; }
            else if (x1) { l2 += 8u + ((u32)(__ffsll((long long)x1) - 1) >> 3); diff = true; }
            else if (x2) { l2 += 16u + ((u32)(__ffsll((long long)x2) - 1) >> 3); diff = true; }
            else if (x3) { l2 += 24u + ((u32)(__ffsll((long long)x3) - 1) >> 3); diff = true; }
            else l2 += 32;
        }
        if (!diff)
        while (pp + l2 + 8 <= mend) {
            const u64 x = ld64(cp + l2) ^ ld64(src + pp + l2);
            if (x) { l2 += (u32)(__ffsll((long long)x) - 1) >> 3; break; }
            l2 += 8;
        }
        if (!diff && pp + l2 + 8 > mend) while (pp + l2 < mend && ld8(cp + l2) == ld8(src + pp + l2)) l2++;
        return l2;
    };
    auto extend = [&](const Pos& P, const Cand& C, u32& len, u32& off) { const u32 l2 = extend_len(P, C); if (l2 > len) { len = l2; off = C.d; } };
    // ---- blocks of binary data (the repeat-offset variant of the trip): long matches, by the whole wave --------------------------------
    // There every position of a chunk often sits in one long match (a run of equal bytes, a repeated record), and the per-lane loop above
    // took all 64 lanes through it 32 bytes per memory round trip — a run of 1 500 bytes = 47 dependent round trips per chunk, all but the
    // first position's for nothing, since the greedy chain picks the first and skips what it covers.  So in that variant a candidate gets ONE
    // per-lane step of 32 bytes (step32); what is still going stays OPEN and is measured to its end only if and when the chain picks it
    // (extend_picked): the wave compares 1 KiB per round trip (16 bytes per lane, contiguous), the last bytes before the block's match
    // limit one byte per lane.  (Tried for every block: text lost 3 % to the extra code in the chain loop — it has few long matches.)
    auto step32 = [&](const Pos& P, Cand& C) {
        const bool more = C.ok && !C.diff && P.p + C.l2 + 32u <= mend;
        if (__ballot(more) == 0) return;
        if (more) {
            const u8* const cp = src + P.p - C.d + C.l2; const u8* const op_ = src + P.p + C.l2;
            const u128 a0 = ld128(cp), a1 = ld128(cp + 16), b0 = ld128(op_), b1 = ld128(op_ + 16);
            const u64 x0 = a0.lo ^ b0.lo, x1 = a0.hi ^ b0.hi, x2 = a1.lo ^ b1.lo, x3 = a1.hi ^ b1.hi;
            if (x0) { C.l2 += (u32)(__ffsll((long long)x0) - 1) >> 3; C.diff = true; }
            else if (x1) { C.l2 += 8u + ((u32)(__ffsll((long long)x1) - 1) >> 3); C.diff = true; }
            else if (x2) { C.l2 += 16u + ((u32)(__ffsll((long long)x2) - 1) >> 3); C.diff = true; }
            else if (x3) { C.l2 += 24u + ((u32)(__ffsll((long long)x3) - 1) >> 3); C.diff = true; }
            else C.l2 += 32;
        }
    };
    // the better of two candidates by what is known of them (an OPEN one is at least as long as its known part)
    auto take = [&](const Cand& C, u32& len, u32& off, bool& open) { if (C.ok && C.l2 > len) { len = C.l2; off = C.d; open = !C.diff; } };
    // the repeat-offset candidate wins unless the table's match is longer by two bytes or more (its sequence is about a byte cheaper)
    auto take_rep = [&](const Cand& C, u32& len, u32& off, bool& open) { if (C.ok && C.l2 >= 4u && C.l2 + 1u >= len) { len = C.l2; off = C.d; open = !C.diff; } };
    auto extend_picked = [&](u32 dL, u32 q) -> u32 {                            // the match at distance dL holds up to q: its end (uniform)
        for (;;) {
            const u32 at = q + 16u * (u32)lane;
            const bool valid = at + 16u <= mend;
            const u128 a = ld128(valid ? src + at - dL : src), b = ld128(valid ? src + at : src);
            const u64 x0 = a.lo ^ b.lo, x1 = a.hi ^ b.hi;
            const bool stop = !valid || (x0 | x1) != 0;
            const u32 nb = x0 ? (u32)(__ffsll((long long)x0) - 1) >> 3 : 8u + ((u32)(__ffsll((long long)(x1 | (1ull << 63))) - 1) >> 3);   // first differing byte of this lane's 16
            const u64 sm = __ballot(stop);
            if (sm == 0) { q += 16u * WAVE; continue; }
            const int f = __ffsll((long long)sm) - 1;
            q += 16u * (u32)f;
            if ((__ballot(valid) >> f) & 1) return q + (u32)__builtin_amdgcn_readlane((int)nb, f);      // a difference
            break;                                                              // fewer than 16 bytes from q to the match limit
        }
        const u32 r = mend - q;                                                 // < 16
        const bool ne = (u32)lane < r && ld8(src + q + (u32)lane - dL) != ld8(src + q + (u32)lane);
        const u64 nm = __ballot(ne);
        return nm ? q + (u32)(__ffsll((long long)nm) - 1) : mend;
    };
    // the parse of one chunk whose lanes hold (len, off) of their best candidate
    auto parse_chunk = [&](u32 base, u32 pp, u32 len, u32 off, bool open, auto rep) {
        constexpr bool REP = decltype(rep)::value;               // (compile time: the repeat-offset search costs registers the other path has no use for)
        u64 openm = REP ? __ballot(open && len != 0u) : 0ull;     // (binary blocks) matches known only up to `len` so far
        u64 mask = __ballot(len >= minmatch) | openm;             // (an open match below the minimum length is tested when it is picked)
        {
            // The sequence list (both formats).  The greedy chain through the chunk (first usable match at or after the cursor wins, the
            // cursor jumps behind it) is the only serial part: a scalar loop of a dozen instructions per emitted match that
            // only collects WHICH positions emit.  Everything else — the lazy rule (a local test on neighbouring lanes), literal
            // lengths, list slots, the stores — is done by all lanes at once.  (The loop used to read, pack and store every
            // sequence through lane 0: ~66 scalar instructions per sequence, 44 % of the kernel's time.)
            u64 usable = mask;
            if (effort >= 1) {                                                  // lazy: the next position has a clearly longer match
                const u32 ln = (u32)__shfl_down((int)len, 1, 64);
                usable &= ~__ballot(lane < 63 && ((mask >> (lane + 1)) & 1) && ln > len + 1);
            }
            u64 emit = 0;
            u32 cur = skip_until > base ? skip_until - base : 0u;               // chunk-relative cursor
            u32 prev_end = 0;                                                   // per emitting lane: where the literals before its match start
            u32 prev_off = 0;                                                   // ... and (repeat-offset search) the offset of the sequence before it
            u32 pe = anchor, po = (u32)__builtin_amdgcn_readfirstlane((int)rep_cur);
            while (cur < 64u) {
                const u64 m = usable & (~0ull << cur);
                if (m == 0) break;
                const int l = __ffsll((long long)m) - 1;
                if (REP && ((openm >> l) & 1)) {                                // picked, and still open: to its end now, by the whole wave
                    const u32 pL = base + (u32)l;
                    const u32 e = extend_picked((u32)__builtin_amdgcn_readlane((int)off, l), pL + (u32)__builtin_amdgcn_readlane((int)len, l));
                    if (lane == l) len = e - pL;
                    openm &= ~(1ull << l);
                    if (e - pL < minmatch) { usable &= ~(1ull << l); continue; }   // (only next to the block's end: a match of fewer than 16 known bytes)
                }
                emit |= 1ull << l;
                if (REP) {
                    u32 m0_keep2;
                    asm volatile("s_mov_b32 %1, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tv_writelane_b32 %0, %2, m0\n\ts_mov_b32 m0, %1" : "+v"(prev_off), "=&s"(m0_keep2) : "s"(po), "s"(l));
                    po = (u32)__builtin_amdgcn_readlane((int)off, l);
                }
                // (the chain knows where the literals before this match start: no search over the lanes afterwards)
                { u32 m0_keep;                                             // (two SGPR operands are one too many for the constant bus: the lane select goes through M0, which is put back)
                  asm volatile("s_mov_b32 %1, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tv_writelane_b32 %0, %2, m0\n\ts_mov_b32 m0, %1" : "+v"(prev_end), "=&s"(m0_keep) : "s"(pe), "s"(l)); }
                cur = (u32)l + (u32)__builtin_amdgcn_readlane((int)len, l);
                pe = base + cur;
            }
            if (emit) {
                const u32 slot = __builtin_amdgcn_mbcnt_hi((u32)(emit >> 32), __builtin_amdgcn_mbcnt_lo((u32)emit, 0u));     // emitted matches before this lane's
                if ((emit >> lane) & 1) {
                    const u32 ll = pp - prev_end;
                    const u64 repflag = (REP && off == prev_off && ll != 0u) ? 1ull << 63 : 0ull;
                    sh.seqring[rn + slot] = (u64)ll | ((u64)len << 20) | ((u64)off << 40) | repflag;
                }
                if (REP) rep_cur = po;
                const u32 ne = (u32)__popcll(emit);                             // <= 16: a match is at least 4 positions long
                nseq += ne; rn += ne;
                anchor = skip_until = base + cur;                               // behind the last emitted match
                if (rn > LZ4E_SEQRING - 16u) {                                  // no room for another chunk's worth: one burst to the list
                    wave_mem_fence();
                    for (u32 i = (u32)lane; i < rn; i += WAVE) ((ZPK_GLOBAL u64*)seqs)[nseq - rn + i] = sh.seqring[i];
                    wave_mem_fence();
                    rn = 0;
                }
            }
        }
    };
    // SEVERAL chunks per trip (round 3, second half; described for two): the chunk loop is bound by its dependent memory round trips — the chunk's own
    // bytes, then the candidates — with one of each in flight per wave.  Both chunks' own bytes are loaded together, both go through
    // the table (look-ups of the second chunk after the inserts of the first: the same order as one chunk at a time), and both
    // sets of candidates are loaded together: one round trip of each kind per 128 positions.  The parses stay in order; a position of
    // the second chunk that the first chunk's last match covers drops its candidate after the fact, so the output is what it was.
    // NCH chunks per trip: 4 in both instantiations (measured; k_encode<12> has 96 VGPRs at five waves per SIMD, k_encode<14>'s 32 KiB table
    // leaves ONE wave per SIMD — nothing hides that wave's round trips but the wave itself)
    constexpr int NCH = HLOG == LZ4E_HASH_LOG ? LZ4E_CHUNKS : LZ4E_CHUNKS_HC;
    auto trip = [&](u32 base, auto fast, auto rep) {
        constexpr bool REP = decltype(rep)::value;
        Pos P[NCH]; Cand C[NCH][2]; Cand R[REP ? NCH : 1];
        const bool do_rep = REP && rep_cur != 0u;                                // (uniform) nothing to try before the frame's first match: incompressible data pays nothing
        #pragma unroll
        for (int i = 0; i < NCH; i++) load_own(P[i], base + (u32)i * WAVE <= mflimit ? base + (u32)i * WAVE + (u32)lane : mflimit + 1u, fast);
        #pragma unroll
        for (int i = 0; i < NCH; i++) if (base + (u32)i * WAVE <= mflimit) lookup_insert(P[i]);      // (uniform) the chunk has a position
        #pragma unroll
        for (int i = 0; i < NCH; i++) {
            probe(P[i], P[i].cand, C[i][0], fast);
            if (effort >= 2) probe(P[i], P[i].cand2, C[i][1], fast); else C[i][1].ok = false;
            if constexpr (REP) { if (do_rep) probe_at(P[i], rep_cur, R[i], fast); else R[i].ok = false; }
        }
        #pragma unroll
        for (int i = 0; i < NCH; i++) { measure16(P[i], C[i][0]); if (effort >= 2) measure16(P[i], C[i][1]); if constexpr (REP) { if (do_rep) measure16(P[i], R[i]); } }
        #pragma unroll
        for (int i = 0; i < NCH; i++) {
            if (base + (u32)i * WAVE > mflimit) return;
            // positions the previous chunks' last match covers drop their candidates (the first chunk's were tested when they were probed)
            C[i][0].ok = C[i][0].ok && P[i].p >= skip_until; C[i][1].ok = C[i][1].ok && P[i].p >= skip_until;
            if constexpr (REP) R[i].ok = R[i].ok && P[i].p >= skip_until;
            u32 len = 0, off = 0; bool open = false;
            if constexpr (REP) {
                step32(P[i], C[i][0]); if (effort >= 2) step32(P[i], C[i][1]);
                if (do_rep) step32(P[i], R[i]);
                take(C[i][0], len, off, open); if (effort >= 2) take(C[i][1], len, off, open);
                if (do_rep) take_rep(R[i], len, off, open);
            } else { extend(P[i], C[i][0], len, off); if (effort >= 2) extend(P[i], C[i][1], len, off); }
            parse_chunk(base + (u32)i * WAVE, P[i].p, len, off, open, rep);
        }
    };
    for (u32 base = 0; base <= mflimit; base += NCH * WAVE) {
        const bool fast = base + NCH * WAVE + 15u <= n && base + NCH * WAVE - 1u <= mflimit;
        if (use_rep) { if (fast) trip(base, ZeBool<true>(), ZeBool<true>()); else trip(base, ZeBool<false>(), ZeBool<true>()); }
        else { if (fast) trip(base, ZeBool<true>(), ZeBool<false>()); else trip(base, ZeBool<false>(), ZeBool<false>()); }
    }
    wave_mem_fence();
    for (u32 i = (u32)lane; i < rn; i += WAVE) ((ZPK_GLOBAL u64*)seqs)[nseq - rn + i] = sh.seqring[i];      // what is left in the ring
    wave_mem_fence();
    if (nseq_out) *nseq_out = nseq;
    if (use_rep) *rep_io = rep_cur;
    if (!dst) return anchor;                                  // Zstandard: anchor = where the trailing literals start
    return lz4e_write_block(src, n, dst, seqs, nseq, anchor, lane);
}

// ---- Zstandard compressed blocks: Raw literals + predefined-distribution FSE sequences -------------------
#define ZE_BLOCK 65536u
#define ZE_MAXSEQ (ZE_BLOCK / 4u + 8u)
#define ZE_SCRATCH_LDS 5760u                                // bytes of the hash table the per-block scratch (ZeHuf, ZeFseCustom) overlays
#define ZE_SHZ_OFF ZE_SCRATCH_LDS                           // ... followed by the predefined tables (ZstdEncShared), reloaded for every block
#define ZE_SHZ_BYTES 2016u
#define ZE_TABLE_SAVE (ZE_SHZ_OFF + ZE_SHZ_BYTES)           // bytes of the hash table that go to HBM while a block is written
// u64 per workgroup: sequence list + literal staging + saved table part + the image of the predefined tables
#define ZE_WG_SCRATCH (ZE_MAXSEQ + ZE_BLOCK / 8u + 8u + ZE_TABLE_SAVE / 8u + ZE_SHZ_BYTES / 8u)

struct alignas(16) ZstdEncShared {
    u16 st[3][64];            // FSE encoder state tables, [T_LL], [T_OF] (32 used), [T_ML]
    u32 dnb[124];             // per symbol: deltaNbBits — LL codes at [0, 36), OF at [36, 68), ML at [68, 121) (ze_sym_base)
    i32 dfs[124];             // per symbol: deltaFindState, same layout
    u32 symtab[2][56];        // [0] literal-length, [1] match-length codes: baseline | extra bits << 24
    u8  tsym[64]; u16 cumul[57];
};
// (packed per kind: with [3][56] arrays the workgroup took 10 560 bytes of LDS = 9 allocation units of 1280 bytes, 14 workgroups per
// CU; 10 208 bytes are 8 units, 16 workgroups)
__device__ __forceinline__ int ze_sym_base(int kind) { return kind == T_LL ? 0 : (kind == T_OF ? 36 : 68); }

// FSE compression table of one predefined distribution (the construction of RFC 8878 4.1 / libzstd
// FSE_buildCTable, restated): by one lane.
__device__ inline void ze_build_ctable_at(u16* st, u32* dnb, i32* dfs, u8* tsym, u16* cumul, const i16* norm, int nsym, int log)
{
    const int size = 1 << log, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
    int high = size - 1;
    cumul[0] = 0;
    for (int s = 0; s < nsym; s++) {
        const int c = norm[s];
        cumul[s + 1] = (u16)(cumul[s] + (c == -1 ? 1 : c));
        if (c == -1) tsym[high--] = (u8)s;
    }
    int pos = 0;
    for (int s = 0; s < nsym; s++) {
        const int c = norm[s];
        for (int i = 0; i < c; i++) { tsym[pos] = (u8)s; do { pos = (pos + step) & mask; } while (pos > high); }
    }
    for (int u = 0; u < size; u++) { const int s = tsym[u]; st[cumul[s]++] = (u16)(size + u); }
    int total = 0;
    for (int s = 0; s < nsym; s++) {
        const int c = norm[s];
        if (c == 0) { dnb[s] = ((u32)(log + 1) << 16) - (u32)size; dfs[s] = 0; }
        else if (c == -1 || c == 1) { dnb[s] = ((u32)log << 16) - (u32)size; dfs[s] = total - 1; total++; }
        else {
            const u32 maxbits = (u32)log - (u32)highbit32((u32)c - 1);
            dnb[s] = (maxbits << 16) - ((u32)c << maxbits);
            dfs[s] = total - c; total += c;
        }
    }
}
__device__ inline void ze_build_ctable(ZstdEncShared& sh, int kind, const i16* norm, int nsym, int log)
{
    ze_build_ctable_at(sh.st[kind], sh.dnb + ze_sym_base(kind), sh.dfs + ze_sym_base(kind), sh.tsym, sh.cumul, norm, nsym, log);
}

__device__ __forceinline__ u32 ze_ll_code(u32 ll)
{
    if (ll < 16) return ll;
    if (ll < 24) return 16 + (ll - 16) / 2;
    if (ll < 32) return 20 + (ll - 24) / 4;
    if (ll < 48) return 22 + (ll - 32) / 8;
    if (ll < 64) return 24;
    return (u32)highbit32(ll) + 19;
}
__device__ __forceinline__ u32 ze_ml_code(u32 ml)          // ml >= 3
{
    const u32 mb = ml - 3;
    if (mb < 32) return mb;
    if (mb < 40) return 32 + (mb - 32) / 2;
    if (mb < 48) return 36 + (mb - 40) / 4;
    if (mb < 64) return 38 + (mb - 48) / 8;
    if (mb < 96) return 40 + (mb - 64) / 16;
    if (mb < 128) return 42;
    return (u32)highbit32(mb) + 36;
}

// LSB-first bit writer of the sequences section (one lane)
struct ZeBits {
    u8* ptr; u64 c; u32 n;
    __device__ __forceinline__ void add(u32 v, u32 nb) { c |= (u64)(v & ((1u << nb) - 1u)) << n; n += nb; }      // nb <= 31
    __device__ __forceinline__ void flush() { st64(ptr, c); ptr += n >> 3; c = (n & ~7u) ? c >> (n & ~7u) : c; n &= 7u; }
    // flush() stores eight bytes whatever it holds: fine where more of the block follows, but behind the END of a block's bitstream the
    // spare bytes of the frame's last block landed behind comp_size (inside the slot, yet not the entry's).  This one stores the bytes it holds.
    __device__ __forceinline__ void flush_exact() { for (u32 i = 0; i < ((n + 7u) >> 3); i++) st8(ptr + i, (u8)(c >> (8u * i))); ptr += n >> 3; c = (n & ~7u) ? c >> (n & ~7u) : c; n &= 7u; }
};
struct ZeState { u32 v; };
// the encoder table of one of the three code kinds for the current block: the predefined one (mode 0), none (mode 1, RLE: the
// kind has a single code in this block and takes no bits), or the block's own (mode 2, FSE_Compressed)
struct ZeTab { const u16* st; const u32* dnb; const i32* dfs; u32 log, mode; };
__device__ __forceinline__ void ze_init_state(const ZeTab& t, ZeState& st, u32 sym)
{
    if (t.mode == 1) { st.v = 0; return; }
    const u32 dnb = t.dnb[sym];
    const u32 nb = (dnb + (1u << 15)) >> 16;
    const u32 val = (nb << 16) - dnb;
    st.v = t.st[(i32)(val >> nb) + t.dfs[sym]];
}
__device__ __forceinline__ void ze_encode(const ZeTab& t, ZeState& st, ZeBits& b, u32 sym)
{
    if (t.mode == 1) return;
    const u32 nb = (st.v + t.dnb[sym]) >> 16;
    b.add(st.v, nb);
    st.v = t.st[(i32)(st.v >> nb) + t.dfs[sym]];
}

// ---- per-block tables for the sequence codes (RFC 8878 3.1.1.3.2.1: RLE_Mode, FSE_Compressed_Mode) ---------------------
// Scratch overlays the LZ4 hash table (and ZeHuf), both dead once the block's literals are written.
struct alignas(16) ZeFseCustom {
    u16 st[1280];                                  // state tables: LL [0, 512), ML [512, 1024), OF [1024, 1280)
    u32 dnb[3][56]; i32 dfs[3][56];
    u32 count[3][56];                              // code histograms of the block
    i16 norm[3][56];
    u8  tsym[512]; u16 cumul[57];
};
// scratch of the sequence bitstream writer; overlays ZeFseCustom::count onwards (histograms and table-construction scratch are dead by then)
struct alignas(16) ZeSeqOut {
    u32 bits[192];                                 // staging buffer of a group's bits: 64 x 89 bits + a carried byte + 3 words of slack
    u16 rec[3][64];                                // [OF, ML, LL][sequence]: state (< 2^11) | number of its low bits that go out << 11
    i16 pdfs[3][64];                               // [OF, ML, LL][sequence]: LDS byte address of the kind's state table + 2 x deltaFindState of the sequence's code (deltaNbBits: in the idle sequence ring)
    u32 zero;                                      // a kind in RLE_Mode has no state: its chain reads this word for ever
};
static_assert(3u * 64u * sizeof(u32) <= LZ4E_SEQRING * sizeof(u64), "the per-sequence deltaNbBits of a group sit in the sequence ring, idle while a block is written");
static_assert(__builtin_offsetof(ZeFseCustom, count) % 16 == 0 && __builtin_offsetof(ZeFseCustom, count) + sizeof(ZeSeqOut) <= sizeof(ZeFseCustom), "ZeSeqOut fits behind the tables");
static_assert(sizeof(ZeFseCustom) <= sizeof(Lz4EncShared), "ZeFseCustom overlays the LZ4 hash table");
static_assert(sizeof(ZeFseCustom) <= ZE_SCRATCH_LDS, "the per-block scratch stays below the predefined tables");
#ifndef ZE_FSE_MIN_SEQ
#define ZE_FSE_MIN_SEQ 64u                         // blocks with fewer sequences keep the predefined tables
#endif

// log2(x) in 1/256 bit, x >= 1 (linear between powers of two: good to 0.09 bit — this only DECIDES between two valid encodings)
__device__ __forceinline__ u32 ze_log2_q8(u32 x) { const u32 h = (u32)highbit32(x); return (h << 8) + (((x << 8) >> h) - 256u); }

// normalized counts of one kind for table size 1 << log; returns false when no valid distribution comes out (predefined then)
__device__ inline bool ze_normalize(const u32* count, i16* norm, int maxsym, u32 total, int log)
{
    const u32 size = 1u << log;
    u32 low = 0, low_total = 0;
    for (int s = 0; s <= maxsym; s++) { const u32 c = count[s]; if (c && c * size < total) { low++; low_total += c; } }
    if (low >= size) return false;
    const u32 rest_size = size - low, rest_total = total - low_total;
    u32 sum = 0, best = 0, bestc = 0;
    for (int s = 0; s <= maxsym; s++) {
        const u32 c = count[s];
        u32 p = 0;
        if (c) {
            if (c * size < total) p = 1;
            else { p = (u32)(((u64)c * rest_size) / rest_total); if (p == 0) p = 1; if (c > bestc) { bestc = c; best = (u32)s; } }
        }
        norm[s] = (i16)p; sum += p;
    }
    if (bestc == 0) return false;
    const i32 fixed = (i32)norm[best] + ((i32)size - (i32)sum);            // the rounding remainder goes to the most frequent code
    if (fixed < 1) return false;
    norm[best] = (i16)fixed;
    return true;
}

// RFC 8878 4.1.1 table description of `norm[0..maxsym]` (the inverse of zf_read_ncount / FSE_readNCount); returns its size in bytes
__device__ inline u32 ze_write_ncount(u8* dst, const i16* norm, int maxsym, int log)
{
    ZeBits b; b.ptr = dst; b.c = 0; b.n = 0;
    b.add((u32)(log - 5), 4);
    int remaining = 1 << log, s = 0;
    while (remaining > 0 && s <= maxsym) {
        const int p = norm[s];
        const u32 v = (u32)(p + 1);
        const int nb = highbit32((u32)remaining + 1u) + 1;
        const u32 lower = (1u << (nb - 1)) - 1u, thr = (1u << nb) - 1u - ((u32)remaining + 1u);
        if (v < thr) b.add(v, (u32)nb - 1u);
        else if (v <= lower) b.add(v, (u32)nb);
        else b.add(v + thr, (u32)nb);
        b.flush();
        remaining -= p;
        s++;
        if (p == 0) {
            int r = 0;
            while (s + r <= maxsym && norm[s + r] == 0) r++;
            s += r;
            while (r >= 3) { b.add(3, 2); b.flush(); r -= 3; }
            b.add((u32)r, 2); b.flush();
        }
    }
    return (u32)(b.ptr - dst) + (b.n ? 1u : 0u);
}


// ---- Huffman-compressed literals (RFC 8878 3.1.1.3.1, 4.2.1): four streams, direct weight description -----------
// Used for blocks with >= ZE_HUF_MIN_LITS literal bytes whose symbols are all <= 128 (the direct description holds at
// most 128 weights; anything else stays Raw).  Scratch overlays the LZ4 hash table, which is dead once the block's
// sequences are listed.  Code lengths: rank sort (lane-parallel) -> two-queue Huffman (one lane) -> limit to 11 bits
// (the redistribution of miniz/zlib) -> canonical codes in the order the decoder fills its table (huf_build, zstd_wg.h).
// Streams are written by 16 lanes each: a lane's piece of >= 16 symbols starts at the bit offset a row prefix sum of
// the piece lengths gives it; bytes shared by two neighbouring pieces are merged after the pass by one extra store (a
// wave's stores to one address land in program order).
#ifndef ZE_HUF_MIN_LITS
#define ZE_HUF_MIN_LITS 2048u
#endif
#define ZE_HUF_MAXBITS 11
struct alignas(16) ZeHuf {
    u32 hist[256];
    u32 ncnt[512];            // tree node counts: leaves ascending, then internal nodes
    u16 parent[512];          // parent index, then (in place) the depth
    u16 order[256];           // symbols by descending count
    u32 cl[256];              // code | length << 16
    u32 nlen[16];             // codes per length
    u32 out[4];               // [0] max bits, [1] ok
};
static_assert(sizeof(ZeHuf) <= sizeof(Lz4EncShared), "ZeHuf overlays the LZ4 hash table");
static_assert(sizeof(ZeHuf) <= ZE_SCRATCH_LDS, "the per-block scratch stays below the predefined tables");

// Huffman weights of symbols [0, last) FSE-compressed (RFC 8878 4.2.1.1; needed as soon as the alphabet reaches past symbol 128, which
// the direct 4-bit description cannot hold): table description, then the weights through TWO interleaved states, last weight first —
// even positions on state 1, odd ones on state 2, exactly the order FSE_compress_usingCTable writes and huf_read_tree reads.
// One lane.  Scratch: the tree-construction arrays of ZeHuf, dead by now.  Returns the size (1..127 bytes) or 0.
__device__ inline u32 ze_huf_weights_fse(ZeHuf& hf, u8* out, u32 last, u32 mb)
{
    u16* const st = (u16*)&hf.ncnt[0]; u32* const dnb = &hf.ncnt[32]; i32* const dfs = (i32*)&hf.ncnt[48]; u32* const cnt = &hf.ncnt[64];
    i16* const norm = (i16*)&hf.ncnt[80]; u16* const cumul = (u16*)&hf.ncnt[88]; u8* const tsym = (u8*)&hf.ncnt[100];
    #define ZE_W(i) ({ const u32 l_ = hf.cl[(i)] >> 16; l_ ? mb + 1u - l_ : 0u; })
    for (int w = 0; w < 16; w++) cnt[w] = 0;
    for (u32 i = 0; i < last; i++) cnt[ZE_W(i)]++;
    int maxw = 0, distinct = 0;
    for (int w = 0; w <= 12; w++) if (cnt[w]) { maxw = w; distinct++; }
    if (distinct < 2) return 0;
    int log = highbit32(last - 1) - 2;
    if (log > 6) log = 6;
    { int minbits = highbit32((u32)maxw) + 2; const int m2 = highbit32(last) + 1; if (m2 < minbits) minbits = m2; if (log < minbits) log = minbits; }
    if (log < 5) log = 5;
    if (log > 6) return 0;
    if (!ze_normalize(cnt, norm, maxw, last, log)) return 0;
    const u32 hb = ze_write_ncount(out, norm, maxw, log);
    ze_build_ctable_at(st, dnb, dfs, tsym, cumul, norm, maxw + 1, log);
    ZeTab t; t.st = st; t.dnb = dnb; t.dfs = dfs; t.log = (u32)log; t.mode = 2;
    ZeBits b; b.ptr = out + hb; b.c = 0; b.n = 0;
    ZeState s1, s2; s1.v = s2.v = 0;
    bool i1 = false, i2 = false;
    for (u32 i = last; i-- > 0;) {
        const u32 w = ZE_W(i);
        if (i & 1u) { if (!i2) { ze_init_state(t, s2, w); i2 = true; } else ze_encode(t, s2, b, w); }
        else { if (!i1) { ze_init_state(t, s1, w); i1 = true; } else ze_encode(t, s1, b, w); }
        b.flush();
        if (b.ptr > out + 140) return 0;
    }
    #undef ZE_W
    b.add(s2.v, (u32)log); b.flush();
    b.add(s1.v, (u32)log); b.flush();
    b.add(1, 1); b.flush();
    const u32 size = (u32)(b.ptr - out) + (b.n ? 1u : 0u);
    return size < 128u ? size : 0u;
}

__device__ inline u32 ze_huf_literals(ZeHuf& hf, const u8* lits, u32 n, u8* dst, u32 raw_size, int lane)
{
    // ---- histogram ----
    for (int i = lane; i < 256; i += WAVE) hf.hist[i] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    for (u32 i = (u32)lane * 16; i < n; i += WAVE * 16) {
        if (i + 16 <= n) {
            const u128 v = ld128(lits + i);
            #pragma unroll
            for (int k = 0; k < 8; k++) { atomicAdd(&hf.hist[(v.lo >> (8 * k)) & 0xFF], 1u); atomicAdd(&hf.hist[(v.hi >> (8 * k)) & 0xFF], 1u); }
        } else for (u32 k = i; k < n; k++) atomicAdd(&hf.hist[ld8(lits + k)], 1u);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    u32 nsym = 0, last = 0;
    #pragma unroll
    for (int k = 0; k < 4; k++) {
        const u64 m = __ballot(hf.hist[lane + 64 * k] != 0);
        nsym += (u32)__popcll(m);
        if (m) last = 64u * k + 63u - (u32)__clzll((long long)m);
    }
    if (nsym < 2) return 0;
    const bool fse_weights = last > 128;                                   // the direct description holds 128 weights
    // ---- symbols by descending count (ties: ascending symbol): every lane ranks four symbols ----
    #pragma unroll 1
    for (int k = 0; k < 4; k++) {
        const u32 sym = (u32)lane + 64u * k, cs = hf.hist[sym];
        u32 rank = 0;
        #pragma unroll 4
        for (u32 t = 0; t < 256; t++) { const u32 ct = hf.hist[t]; rank += (ct > cs || (ct == cs && t < sym)) ? 1u : 0u; }
        hf.order[rank] = (u16)sym;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    // ---- code lengths and codes, one lane ----
    lane0_guard();
    if (lane == 0) {
        const u32 ns = nsym;
        for (u32 i = 0; i < ns; i++) hf.ncnt[i] = hf.hist[hf.order[ns - 1 - i]];
        u32 li = 0, ii = ns, nn = ns;
        for (u32 k = 0; k + 1 < ns; k++) {
            u32 a, b;
            if (li < ns && (ii >= nn || hf.ncnt[li] <= hf.ncnt[ii])) a = li++; else a = ii++;
            if (li < ns && (ii >= nn || hf.ncnt[li] <= hf.ncnt[ii])) b = li++; else b = ii++;
            hf.ncnt[nn] = hf.ncnt[a] + hf.ncnt[b];
            hf.parent[a] = (u16)nn; hf.parent[b] = (u16)nn;
            nn++;
        }
        hf.parent[nn - 1] = 0;                                           // root: depth 0
        for (u32 k = nn - 1; k-- > 0;) hf.parent[k] = (u16)(hf.parent[hf.parent[k]] + 1);
        for (int l = 0; l < 16; l++) hf.nlen[l] = 0;
        for (u32 i = 0; i < ns; i++) { u32 d = hf.parent[i]; if (d > ZE_HUF_MAXBITS) d = ZE_HUF_MAXBITS; hf.nlen[d]++; }
        u32 total = 0;
        for (int l = 1; l <= ZE_HUF_MAXBITS; l++) total += hf.nlen[l] << (ZE_HUF_MAXBITS - l);
        while (total > (1u << ZE_HUF_MAXBITS)) {
            hf.nlen[ZE_HUF_MAXBITS]--;
            for (int l = ZE_HUF_MAXBITS - 1; l > 0; l--) if (hf.nlen[l]) { hf.nlen[l]--; hf.nlen[l + 1] += 2; break; }
            total--;
        }
        u32 mb = 0;
        for (int l = 1; l <= ZE_HUF_MAXBITS; l++) if (hf.nlen[l]) mb = (u32)l;
        for (int i = 0; i < 256; i++) hf.cl[i] = 0;
        u32 idx = 0;                                                      // most frequent symbols get the shortest codes
        for (u32 l = 1; l <= mb; l++) for (u32 c = 0; c < hf.nlen[l]; c++) hf.cl[hf.order[idx++]] = l << 16;
        // canonical codes as the decoder lays its table out: weight classes ascending (longest codes first), natural
        // symbol order inside a class, every symbol of weight w taking 2^(w-1) slots
        u32 start[ZE_HUF_MAXBITS + 2];
        u32 pos = 0;
        for (u32 w = 1; w <= mb; w++) { start[w] = pos; pos += hf.nlen[mb + 1 - w] << (w - 1); }
        for (u32 sy = 0; sy <= last; sy++) {
            const u32 l = hf.cl[sy] >> 16;
            if (!l) continue;
            const u32 w = mb + 1 - l;
            hf.cl[sy] = (l << 16) | (start[w] >> (w - 1));
            start[w] += 1u << (w - 1);
        }
        hf.out[0] = mb; hf.out[1] = pos == (1u << mb) ? 1u : 0u;         // complete code (always, for >= 2 symbols)
        hf.out[2] = 0;
        // FSE-compressed weights go straight to their place behind a 5-byte literals header (Size_Format 3) and the header byte
        if (fse_weights && hf.out[1]) hf.out[2] = ze_huf_weights_fse(hf, dst + 5 + 1, last, mb);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    lane0_guard();
    const u32 mb = uni(hf.out[0]);
    if (!uni(hf.out[1]) || mb == 0) return 0;

    // ---- the four streams: pass 1 = bits per piece ----
    const int grp = lane >> 4, j = lane & 15;
    const u32 seg = (n + 3) / 4;
    const u32 sbase = seg * (u32)grp;
    const u32 S = grp < 3 ? seg : n - 3 * seg;                           // >= 256 symbols: n >= ZE_HUF_MIN_LITS
    const u32 P = S >> 4, extra = S - 16 * P;
    const u32 hi = j == 0 ? S : S - extra - (u32)j * P;                   // piece j encodes symbols [lo, hi), last one first
    const u32 lo = S - extra - ((u32)j + 1) * P;
    const u8* const sp = lits + sbase;
    // (both passes read a piece 16 bytes per load: a byte per load made every symbol wait for a memory round trip of its own)
    u32 bits = 0;
    {
        u32 i = lo;
        for (; i + 16 <= hi; i += 16) {
            const u128 v = ld128(sp + i);
            #pragma unroll
            for (int k = 0; k < 8; k++) bits += (hf.cl[(v.lo >> (8 * k)) & 0xFF] >> 16) + (hf.cl[(v.hi >> (8 * k)) & 0xFF] >> 16);
        }
        for (; i < hi; i++) bits += hf.cl[ld8(sp + i)] >> 16;
    }
    if (j == 15) bits += 1;                                               // the end mark
    u32 x = bits;
    x += (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);
    x += (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);
    x += (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);
    x += (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);
    const u32 off = x - bits, end = x;
    const u32 sb0 = ((u32)__builtin_amdgcn_readlane((int)x, 15) + 7) >> 3, sb1 = ((u32)__builtin_amdgcn_readlane((int)x, 31) + 7) >> 3;
    const u32 sb2 = ((u32)__builtin_amdgcn_readlane((int)x, 47) + 7) >> 3, sb3 = ((u32)__builtin_amdgcn_readlane((int)x, 63) + 7) >> 3;
    const u32 wsize = uni(hf.out[2]);
    if (fse_weights && wsize == 0) return 0;
    const u32 tree = fse_weights ? 1u + wsize : 1u + (last + 1) / 2;        // header byte + FSE-compressed weights / `last` 4-bit weights
    const u32 csize = tree + 6 + sb0 + sb1 + sb2 + sb3;
    if (sb0 > 65535 || sb1 > 65535 || sb2 > 65535) return 0;
    const u32 fmt = (!fse_weights && n < 16384 && csize < 16384) ? 2u : 3u;
    const u32 hl = fmt == 2 ? 4u : 5u;
    if (hl + csize + 32 >= raw_size) return 0;                            // not worth it: the caller writes Raw literals
    // ---- header, tree description, jump table ----
    lane0_guard();
    if (lane == 0) {
        if (fmt == 2) st32(dst, 2u | (fmt << 2) | (n << 4) | (csize << 18));
        else { const u64 v = 2ull | ((u64)fmt << 2) | ((u64)n << 4) | ((u64)csize << 22); st32(dst, (u32)v); st8(dst + 4, (u8)(v >> 32)); }
        u8* t = dst + hl;
        if (fse_weights) st8(t, (u8)wsize);                                // (the weights are already in place behind it)
        else {
            st8(t, (u8)(127 + last));
            for (u32 i = 0; i < last; i += 2) {
                const u32 l0 = hf.cl[i] >> 16, l1 = i + 1 < last ? hf.cl[i + 1] >> 16 : 0u;
                st8(t + 1 + i / 2, (u8)(((l0 ? mb + 1 - l0 : 0u) << 4) | (l1 ? mb + 1 - l1 : 0u)));
            }
        }
        u8* jt = t + tree;
        st16(jt, (u16)sb0); st16(jt + 2, (u16)sb1); st16(jt + 4, (u16)sb2);
    }
    u8* const stream = dst + hl + tree + 6 + (grp > 0 ? sb0 : 0u) + (grp > 1 ? sb1 : 0u) + (grp > 2 ? sb2 : 0u);
    // ---- pass 2: encode ----
    u64 acc = 0; u32 na = off & 7u;
    u8* bp = stream + (off >> 3);
    u32 head = 0, tail = 0; bool have_head = false;
    {
        // two codes (<= 22 bits) per flush test: na < 32 before, < 54 after, one flush brings it back below 32
        #define ZE_HUF_PUT2(ca_, cb_) do { acc |= (u64)((ca_) & 0xFFFFu) << na; na += (ca_) >> 16; acc |= (u64)((cb_) & 0xFFFFu) << na; na += (cb_) >> 16; \
            if (na >= 32) { if (!have_head) { head = (u32)acc & 0xFFu; have_head = true; } st32(bp, (u32)acc); bp += 4; acc >>= 32; na -= 32; } } while (0)
        u32 i = hi;
        while (i - lo >= 16) {                                             // symbols i + 15 ... i, the last one first
            i -= 16;
            const u128 v = ld128(sp + i);
            #pragma unroll
            for (int g = 3; g >= 0; g--) {
                const u32 w = g == 3 ? (u32)(v.hi >> 32) : (g == 2 ? (u32)v.hi : (g == 1 ? (u32)(v.lo >> 32) : (u32)v.lo));
                const u32 c3 = hf.cl[w >> 24], c2 = hf.cl[(w >> 16) & 0xFF], c1 = hf.cl[(w >> 8) & 0xFF], c0 = hf.cl[w & 0xFF];
                ZE_HUF_PUT2(c3, c2);
                ZE_HUF_PUT2(c1, c0);
            }
        }
        while (i > lo) {
            i--;
            const u32 c = hf.cl[ld8(sp + i)];
            acc |= (u64)(c & 0xFFFFu) << na;
            na += c >> 16;
            if (na >= 32) {
                if (!have_head) { head = (u32)acc & 0xFFu; have_head = true; }
                st32(bp, (u32)acc); bp += 4; acc >>= 32; na -= 32;
            }
        }
        #undef ZE_HUF_PUT2
    }
    if (j == 15) { acc |= 1ull << na; na += 1; }
    while (na > 0) {
        const u32 b = (u32)acc & 0xFFu;
        if (!have_head) { head = b; have_head = true; }
        tail = b;
        st8(bp++, (u8)b); acc >>= 8; na = na > 8 ? na - 8 : 0;
    }
    wave_mem_fence();
    // the byte this piece's last bits share with the next piece's first bits
    const u32 head_next = (u32)__builtin_amdgcn_update_dpp(0, (int)head, 0x101, 0xf, 0xf, false);         // row_shl:1
    if ((end & 7u) != 0 && j != 15) st8(stream + (end >> 3), (u8)(tail | head_next));
    wave_mem_fence();
    return hl + csize;
}

// One block src[0, n) -> dst as Compressed_Block body (without the 3-byte block header); returns its size or 0
// when it would not be smaller than n (the caller then writes a Raw block).  seqs: global scratch, ZE_MAXSEQ u64.
template <int HLOG>
__device__ inline u32 zstde_block_inner(Lz4EncSharedT<HLOG>& she, ZstdEncShared& sh, const u8* src, u32 n, u8* dst, u64* seqs, int lane, int effort,
                                        u64 abs_base, bool& table_saved, u32& rep_hist)
{
    // rep_hist = the frame's repeat offset 1 in front of this block: the offset of the last sequence of the last block that went out as a
    // Compressed_Block (0 = none yet).  Only sequences flagged by the repeat-offset search are coded against it, and only ever
    // as offset value 1 with literals in front — then repeat offset 1 is always the previous sequence's offset, whatever the block mixes.
    u32 nseq = 0;
    // A sequence costs ~3.3 bytes over the predefined tables and a Huffman-coded literal of text-like data ~0.55 bytes, so
    // there matches shorter than ZE_MINMATCH lose (libzstd level 1 uses 5..7 for the same reason): text 0.425 -> 0.409 and
    // 20 % faster.  Blocks with bytes above 128 keep Raw literals (direct tree description) and take every match from 4.
    bool binary;
    {   // any byte >= 128?  No early exit: a loop whose condition waits for its own load is one memory round trip per iteration (64 of
        // them per block, the block's first touch of HBM); this way the loads are in flight together
        u64 hb = 0;
        const u32 full = n & ~15u;
        #pragma unroll 4
        for (u32 i = (u32)lane * 16; i < full; i += WAVE * 16) { const u128 v = ld128(src + i); hb |= v.lo | v.hi; }
        if (full + (u32)lane < n) hb |= (u64)ld8(src + full + (u32)lane);
        binary = __ballot((hb & 0x8080808080808080ull) != 0) != 0;
    }
    u32 rep_in = rep_hist;
    const u32 tail = lz4e_block(she, src, n, nullptr, lane, seqs, &nseq, binary ? 4u : ZE_MINMATCH, effort, abs_base, binary ? &rep_in : nullptr);
    wave_mem_fence();
    const u32 last_off = nseq ? (u32)(uni64(((const ZPK_GLOBAL u64*)seqs)[nseq - 1]) >> 40) & 0x7FFFFFu : 0u;      // what repeat offset 1 is behind this block, if it goes out compressed
    if (nseq == 0 || n < 16) return 0;
    {   // the Huffman / FSE scratch below overlays the first ZE_TABLE_SAVE bytes of the hash table, which the NEXT block of the entry
        // still wants (matches into the previous block): that part goes to the workgroup's HBM scratch and comes back afterwards
        u8* const save = (u8*)(seqs + ZE_MAXSEQ + ZE_BLOCK / 8u + 8u);
        for (u32 c = (u32)lane * 16u; c < ZE_TABLE_SAVE; c += WAVE * 16u) st128(save + c, *(const u128*)((const u8*)&she + c));
        table_saved = true;
        // the predefined tables (code baselines, the three default FSE tables) live in the same LDS: built once per workgroup, kept
        // in its HBM scratch, brought in for the block-writing phase (8 KiB of LDS per workgroup instead of 10: 18 per CU, not 16)
        const u8* const img = save + ZE_TABLE_SAVE;
        wave_mem_fence();
        for (u32 c = (u32)lane * 16u; c < ZE_SHZ_BYTES; c += WAVE * 16u) *(u128*)((u8*)&sh + c) = ld128(img + c);
        wave_mem_fence();
    }
    // ---- literal lengths: total, and the position of every run (prefix sums over the list, 64 at a time) ----
    u32 lit_total = n - tail;                                              // trailing literals
    {
        u32 mine = 0;                                                      // (independent loads, one reduction at the end)
        #pragma unroll 4
        for (u32 k = (u32)lane; k < nseq; k += WAVE) mine += (u32)(((const ZPK_GLOBAL u64*)seqs)[k] & 0xFFFFFu);
        lit_total += (u32)__builtin_amdgcn_readlane((int)wave_scan_add(mine), 63);
    }
    const u32 lh = lit_total < 32 ? 1u : (lit_total < 4096 ? 2u : 3u);
    const u32 sh_bytes = nseq < 128 ? 1u : (nseq < 0x7F00 ? 2u : 3u);
    const bool try_huf = lit_total >= ZE_HUF_MIN_LITS;
    if (!try_huf && lh + lit_total + sh_bytes + 1 + 16 >= n) return 0;      // cannot win
    // ---- literals: gathered into the block (Raw_Literals_Block) or into scratch first (Huffman) ----
    u8* const stage = (u8*)(seqs + ZE_MAXSEQ);                              // ZE_BLOCK + 64 bytes behind the sequence list
    u8* lit = try_huf ? stage : dst + lh;
    {
        u32 spos = 0, lpos = 0;                                            // running source / literal positions (uniform)
        // 128 sequences per iteration: both list loads, then the first 32 bytes of both sets of runs, are in flight together before the
        // first store (one list round trip + one copy round trip per 128 sequences instead of two per 64)
        for (u32 b0 = 0; b0 < nseq; b0 += 2 * WAVE) {
            const u32 kA = b0 + (u32)lane, kB = kA + WAVE;
            const u64 qA = kA < nseq ? ((const ZPK_GLOBAL u64*)seqs)[kA] : 0ull, qB = kB < nseq ? ((const ZPK_GLOBAL u64*)seqs)[kB] : 0ull;
            const u32 llA = (u32)(qA & 0xFFFFFu), mlA = (u32)((qA >> 20) & 0xFFFFFu), llB = (u32)(qB & 0xFFFFFu), mlB = (u32)((qB >> 20) & 0xFFFFFu);
            const u32 xsA = wave_scan_add(llA + mlA), xlA = wave_scan_add(llA), xsB = wave_scan_add(llB + mlB), xlB = wave_scan_add(llB);
            const u32 tsA = (u32)__builtin_amdgcn_readlane((int)xsA, 63), tlA = (u32)__builtin_amdgcn_readlane((int)xlA, 63);
            const u8* const sA = src + spos + (xsA - (llA + mlA));
            const u8* const sB = src + spos + tsA + (xsB - (llB + mlB));
            u8* const dA = lit + lpos + (xlA - llA);
            u8* const dB = lit + lpos + tlA + (xlB - llB);
            const u32 nA = llA < 32u ? llA : 32u, nB = llB < 32u ? llB : 32u;
            const Copy32 cA = gload_wide32(sA, nA, sA + 16 <= src + n), cB = gload_wide32(sB, nB, sB + 16 <= src + n);
            gstore_wide32(dA, cA, nA);
            gstore_wide32(dB, cB, nB);
            ze_copy_long_literals(dA, sA, llA, true, lane);
            ze_copy_long_literals(dB, sB, llB, true, lane);
            spos += tsA + (u32)__builtin_amdgcn_readlane((int)xsB, 63);
            lpos += tlA + (u32)__builtin_amdgcn_readlane((int)xlB, 63);
        }
        for (u32 c = (u32)lane * 16; c < n - tail; c += WAVE * 16) gcopy_upto16(lit + lpos + c, src + tail + c, n - tail - c);
    }
    wave_mem_fence();
    u32 lit_section = 0;
    if (try_huf) lit_section = ze_huf_literals(*(ZeHuf*)&she, stage, lit_total, dst, lh + lit_total, lane);
    if (lit_section == 0) {                                                 // Raw_Literals_Block
        if (lh + lit_total + sh_bytes + 1 + 16 >= n) return 0;
        if (try_huf) for (u32 c = (u32)lane * 16; c < lit_total; c += WAVE * 16) gcopy_upto16(dst + lh + c, stage + c, lit_total - c);
        lane0_guard();
        if (lane == 0) {
            if (lh == 1) st8(dst, (u8)(lit_total << 3));
            else if (lh == 2) { const u32 v = (1u << 2) | (lit_total << 4); st8(dst, (u8)v); st8(dst + 1, (u8)(v >> 8)); }
            else { const u32 v = (3u << 2) | (lit_total << 4); st8(dst, (u8)v); st8(dst + 1, (u8)(v >> 8)); st8(dst + 2, (u8)(v >> 16)); }
        }
        lit_section = lh + lit_total;
    }
    wave_mem_fence();
    // ---- sequences section ----
    u8* sq = dst + lit_section;
    u32 seq_bytes = 0;
    {
        // Code statistics of the block (all lanes, LDS atomics): with enough sequences every kind gets its own table — RLE_Mode when
        // the block uses a single code of the kind, FSE_Compressed_Mode when the block's own distribution, description included,
        // beats the predefined one (the estimate only has to pick between two valid encodings).
        ZeFseCustom& cf = *(ZeFseCustom*)&she;
        const bool custom = nseq >= ZE_FSE_MIN_SEQ;
        if (custom) {
            for (u32 i = (u32)lane; i < 3u * 56u; i += WAVE) (&cf.count[0][0])[i] = 0;
            wave_mem_fence();
            for (u32 b0 = 0; b0 < nseq; b0 += 4 * WAVE) {                   // four list loads in flight
                u64 q[4];
                #pragma unroll
                for (int u = 0; u < 4; u++) { const u32 k = b0 + (u32)u * WAVE + (u32)lane; q[u] = k < nseq ? ((const ZPK_GLOBAL u64*)seqs)[k] : ~0ull; }
                #pragma unroll
                for (int u = 0; u < 4; u++) if (q[u] != ~0ull) {               // (no listed sequence is all ones: lengths stay below 2^17)
                    const u32 ll = (u32)(q[u] & 0xFFFFFu), ml = (u32)((q[u] >> 20) & 0xFFFFFu), ofv = (q[u] >> 63) ? 1u : ((u32)(q[u] >> 40) & 0x7FFFFFu) + 3u;       // bit 63: the offset repeats the previous sequence's -> offset value 1
                    atomicAdd(&cf.count[T_LL][ze_ll_code(ll)], 1u);
                    atomicAdd(&cf.count[T_ML][ze_ml_code(ml)], 1u);
                    atomicAdd(&cf.count[T_OF][(u32)highbit32(ofv)], 1u);
                }
            }
            wave_mem_fence();
        }
        // The bitstream is written backwards through the list by ONE lane (a serial FSE state machine), but the list
        // is read by the whole wave, 64 entries per load, and handed over with v_readlane: one global round trip per
        // 64 sequences instead of one per sequence.
        u8* p = sq;
        ZeTab tl, to, tm;
        tl.st = sh.st[T_LL]; tl.dnb = sh.dnb + ze_sym_base(T_LL); tl.dfs = sh.dfs + ze_sym_base(T_LL); tl.log = 6; tl.mode = 0;
        to.st = sh.st[T_OF]; to.dnb = sh.dnb + ze_sym_base(T_OF); to.dfs = sh.dfs + ze_sym_base(T_OF); to.log = 5; to.mode = 0;
        tm.st = sh.st[T_ML]; tm.dnb = sh.dnb + ze_sym_base(T_ML); tm.dfs = sh.dfs + ze_sym_base(T_ML); tm.log = 6; tm.mode = 0;
        u32 desc_bytes = 0;
        lane0_guard();
        if (lane == 0) {
            if (nseq < 128) { st8(p, (u8)nseq); }
            else if (nseq < 0x7F00) { st8(p, (u8)((nseq >> 8) + 128)); st8(p + 1, (u8)nseq); }
            else { st8(p, 255); st8(p + 1, (u8)(nseq - 0x7F00)); st8(p + 2, (u8)((nseq - 0x7F00) >> 8)); }
            u8* dp = p + sh_bytes + 1;                                     // table descriptions: LL, OF, ML
            if (custom) {
                #pragma unroll 1
                for (int kind = 0; kind < 3; kind++) {                     // T_LL, T_OF, T_ML: the order in the stream
                    ZeTab& t = kind == T_LL ? tl : (kind == T_OF ? to : tm);
                    const int maxlog = kind == T_OF ? 8 : 9, nsym_all = kind == T_LL ? 36 : (kind == T_OF ? 32 : 53);
                    const i16* const defn = kind == T_LL ? Z_LL_DEF : (kind == T_OF ? Z_OF_DEF : Z_ML_DEF);
                    const int defsyms = kind == T_OF ? 29 : nsym_all;
                    const u32* const cnt = cf.count[kind];
                    int maxsym = -1, distinct = 0;
                    for (int s2 = 0; s2 < nsym_all; s2++) if (cnt[s2]) { maxsym = s2; distinct++; }
                    if (distinct == 1) { st8(dp, (u8)maxsym); dp += 1; t.mode = 1; t.log = 0; continue; }
                    // table log as FSE_optimalTableLog: enough for the counts, no more than the sequences justify
                    int minbits = highbit32((u32)maxsym) + 2; { const int m2 = highbit32(nseq) + 1; if (m2 < minbits) minbits = m2; }
                    int log = highbit32(nseq - 1) - 2;
                    if (log > maxlog) log = maxlog;
                    if (log < minbits) log = minbits;
                    if (log < 5) log = 5;
                    if (log > maxlog) continue;                            // (cannot happen: minbits <= 8)
                    i16* const norm = cf.norm[kind];
                    if (!ze_normalize(cnt, norm, maxsym, nseq, log)) continue;
                    const u32 hb = ze_write_ncount(dp, norm, maxsym, log);
                    u32 cost_c = hb * 8u * 256u, cost_d = 0;                // in 1/256 bit
                    bool def_ok = true;
                    for (int s2 = 0; s2 <= maxsym; s2++) if (cnt[s2]) {
                        cost_c += cnt[s2] * (((u32)log << 8) - ze_log2_q8((u32)norm[s2]));
                        const int dn = s2 < defsyms ? defn[s2] : 0;
                        if (dn == 0) def_ok = false;
                        else cost_d += cnt[s2] * (((kind == T_OF ? 5u : 6u) << 8) - ze_log2_q8(dn < 0 ? 1u : (u32)dn));
                    }
                    if (def_ok && cost_d <= cost_c) continue;               // the predefined table is as good: keep it
                    u16* const cst = cf.st + (kind == T_LL ? 0 : (kind == T_ML ? 512 : 1024));
                    ze_build_ctable_at(cst, cf.dnb[kind], cf.dfs[kind], cf.tsym, cf.cumul, norm, maxsym + 1, log);
                    t.st = cst; t.dnb = cf.dnb[kind]; t.dfs = cf.dfs[kind]; t.log = (u32)log; t.mode = 2;
                    dp += hb;
                }
            }
            st8(p + sh_bytes, (u8)((tl.mode << 6) | (to.mode << 4) | (tm.mode << 2)));      // Symbol_Compression_Modes
            desc_bytes = (u32)(dp - (p + sh_bytes + 1));
        }
        lane0_guard();
        p += sh_bytes + 1 + uni(desc_bytes);
        u8* const limit = dst + n - 16;                                    // the block must stay below n bytes
        bool ok = p <= limit;
        // Lane 0 chose the tables; every lane needs them now.
        {
            const u32 mdl = uni(tl.mode), mdo = uni(to.mode), mdm = uni(tm.mode), lgl = uni(tl.log), lgo = uni(to.log), lgm = uni(tm.log);
            tl.mode = mdl; tl.log = lgl; to.mode = mdo; to.log = lgo; tm.mode = mdm; tm.log = lgm;
            if (mdl == 2) { tl.st = cf.st; tl.dnb = cf.dnb[T_LL]; tl.dfs = cf.dfs[T_LL]; }
            if (mdm == 2) { tm.st = cf.st + 512; tm.dnb = cf.dnb[T_ML]; tm.dfs = cf.dfs[T_ML]; }
            if (mdo == 2) { to.st = cf.st + 1024; to.dnb = cf.dnb[T_OF]; to.dfs = cf.dfs[T_OF]; }
        }
        // The bitstream, 64 sequences at a time (backwards through the list).  Only the three FSE STATE CHAINS are serial, and
        // they do not depend on each other: lanes 0 / 1 / 2 run the offset / match-length / literal-length chain side by
        // side — a step is one table lookup and leaves (bits, count) of its state in LDS.  Everything else is done by all
        // lanes at once: codes and extra bits, the bit string of each sequence (state bits OF, ML, LL, then extra bits LL, ML,
        // OF), its position in the stream (a prefix sum of the bit counts), the merge into an LDS staging buffer (ds_or) and
        // the stores of the finished bytes.  (One lane used to do all of it: ~90 instructions per sequence, 40 % of k_encode.)
        ZeSeqOut& sout = *(ZeSeqOut*)((u8*)&cf + __builtin_offsetof(ZeFseCustom, count));      // count / norm / tsym / cumul are dead by now
        ZPK_LDS u16* const r_rec = (ZPK_LDS u16*)sout.rec[lane < 3 ? lane : 0];
        // (round 3) a chain step used to be three dependent LDS round trips: the sequence's code, the code's (deltaNbBits, deltaFindState),
        // the next state.  Only the last one depends on the state: the other two are looked up by all 64 lanes at once, left per sequence
        // in LDS and read by the chain lanes four steps at a time.  What is left per step: nb = (state + deltaNbBits) >> 16, the record
        // state | nb << 11 (the 64 lanes cut the nb low bits out later), next state = the u16 at ((state >> nb) << 1) + F, where F = the
        // state table's LDS address + 2 x deltaFindState, folded per sequence.  A kind in RLE_Mode has deltaNbBits 0 and F = a zero word.
        ZPK_LDS u32* const pdnb = (ZPK_LDS u32*)she.seqring;                                   // [OF, ML, LL][64]
        const ZPK_LDS u32* const r_pd = pdnb + 64 * (lane < 3 ? lane : 0);
        const ZPK_LDS i16* const r_pf = (const ZPK_LDS i16*)sout.pdfs[lane < 3 ? lane : 0];
        const ZPK_LDS u32* const a_dnb_o = (const ZPK_LDS u32*)to.dnb; const ZPK_LDS i32* const a_dfs_o = (const ZPK_LDS i32*)to.dfs;
        const ZPK_LDS u32* const a_dnb_m = (const ZPK_LDS u32*)tm.dnb; const ZPK_LDS i32* const a_dfs_m = (const ZPK_LDS i32*)tm.dfs;
        const ZPK_LDS u32* const a_dnb_l = (const ZPK_LDS u32*)tl.dnb; const ZPK_LDS i32* const a_dfs_l = (const ZPK_LDS i32*)tl.dfs;
        const ZPK_LDS u8* const lbase = (const ZPK_LDS u8*)&she;
        const i32 zoff = (i32)((const ZPK_LDS u8*)&sout.zero - lbase);
        const bool rle_o = to.mode == 1, rle_m = tm.mode == 1, rle_l = tl.mode == 1;          // (uniform)
        const i32 st_o = (i32)((const ZPK_LDS u8*)to.st - lbase), st_m = (i32)((const ZPK_LDS u8*)tm.st - lbase), st_l = (i32)((const ZPK_LDS u8*)tl.st - lbase);
        if (lane == 0) *(ZPK_LDS u32*)&sout.zero = 0;
        u32 r_state = 0;
        u32 carry_n = 0;                                                    // bits (< 8) of the staging buffer's first byte already taken
        for (u32 c = (u32)lane * 16u; c < sizeof(sout.bits); c += WAVE * 16u) lds_st128((lds_p8)((ZPK_LDS u8*)sout.bits + c), u128{0, 0});
        // The group's list words are loaded a group AHEAD and turned into codes, extra bits and the chain's per-sequence words at the END
        // of the previous group's pass, in front of its stores: a load waited for right behind the stores (loads and stores share one
        // counter) cost every group a store round trip plus a load round trip; this way whatever is outstanding at the wait is a
        // whole chain pass old.
        u32 p_xl = 0, p_xm = 0, p_xo = 0, p_nb = 0;
        auto load_group = [&](u32 hi_) -> u64 {
            const u32 lo_ = hi_ > WAVE ? hi_ - WAVE : 0u;
            return (u32)lane < hi_ - lo_ ? ((const ZPK_GLOBAL u64*)seqs)[lo_ + (u32)lane] : 0ull;
        };
        auto prep_group = [&](u64 q, u32 cnt_) {
            p_xl = 0; p_xm = 0; p_xo = 0; p_nb = 0;
            if ((u32)lane < cnt_) {
                const u32 ll = (u32)(q & 0xFFFFFu), ml = (u32)((q >> 20) & 0xFFFFFu), ofv = (q >> 63) ? 1u : ((u32)(q >> 40) & 0x7FFFFFu) + 3u;
                const u32 lc = ze_ll_code(ll), mc = ze_ml_code(ml), oc = (u32)highbit32(ofv);
                const u32 lt = sh.symtab[0][lc], mt = sh.symtab[1][mc];
                p_xl = ll - (lt & 0xFFFFFFu); p_xm = ml - (mt & 0xFFFFFFu); p_xo = ofv - (1u << oc);
                p_nb = (lt >> 24) | ((mt >> 24) << 8) | (oc << 16);
                pdnb[lane] = rle_o ? 0u : a_dnb_o[oc]; pdnb[64 + lane] = rle_m ? 0u : a_dnb_m[mc]; pdnb[128 + lane] = rle_l ? 0u : a_dnb_l[lc];
                ((ZPK_LDS i16*)sout.pdfs[0])[lane] = (i16)(rle_o ? zoff : st_o + 2 * a_dfs_o[oc]);
                ((ZPK_LDS i16*)sout.pdfs[1])[lane] = (i16)(rle_m ? zoff : st_m + 2 * a_dfs_m[mc]);
                ((ZPK_LDS i16*)sout.pdfs[2])[lane] = (i16)(rle_l ? zoff : st_l + 2 * a_dfs_l[lc]);
            }
        };
        u64 q_ahead = load_group(nseq);
        prep_group(q_ahead, nseq > WAVE ? WAVE : nseq);
        q_ahead = nseq > WAVE ? load_group(nseq - WAVE) : 0ull;
        for (u32 hi = nseq; hi > 0;) {
            const u32 lo = hi > WAVE ? hi - WAVE : 0u;
            const u32 cnt = hi - lo;
            wave_mem_fence();
            if (lane < 3) {                                                 // the three state chains
                #define ZE_CHAIN_STEP(dnb_, f_, rec_) do { const u32 nb_ = (r_state + (dnb_)) >> 16; \
                    rec_ = r_state | (nb_ << 11); \
                    r_state = (u32)*(const ZPK_LDS u16*)(lbase + (i32)(((r_state >> nb_) << 1) + (u32)(i32)(f_))); } while (0)
                u32 k = cnt;
                if (hi == nseq) {                                           // the last sequence starts the states and puts no state bits
                    k--;
                    const u32 dnb = r_pd[k];
                    const u32 nb = (dnb + (1u << 15)) >> 16;
                    r_state = (u32)*(const ZPK_LDS u16*)(lbase + (i32)(((((nb << 16) - dnb) >> nb) << 1) + (u32)(i32)r_pf[k]));
                    r_rec[k] = 0;
                }
                while (k & 3u) { k--; u32 rc; ZE_CHAIN_STEP(r_pd[k], r_pf[k], rc); r_rec[k] = (u16)rc; }
                while (k) {                                                  // four steps per pair of LDS reads, one 8-byte store of their records
                    k -= 4;
                    const u128 d4 = lds_ld128((lds_cp8)(r_pd + k));
                    const u64 f4 = *(const ZPK_LDS u64*)(r_pf + k);
                    u32 r3, r2, r1, r0;
                    ZE_CHAIN_STEP((u32)(d4.hi >> 32), (i16)(f4 >> 48), r3);
                    ZE_CHAIN_STEP((u32)d4.hi, (i16)(f4 >> 32), r2);
                    ZE_CHAIN_STEP((u32)(d4.lo >> 32), (i16)(f4 >> 16), r1);
                    ZE_CHAIN_STEP((u32)d4.lo, (i16)f4, r0);
                    *(ZPK_LDS u64*)(r_rec + k) = (u64)r0 | ((u64)r1 << 16) | ((u64)r2 << 32) | ((u64)r3 << 48);
                }
                #undef ZE_CHAIN_STEP
            }
            wave_mem_fence();
            // every sequence's bit string (<= 26 state bits + 16 + 16 + 31 extra bits) and where it goes
            u32 nbits = 0; u64 lo64 = 0, hi64 = 0;
            if ((u32)lane < cnt) {
                const u32 ro = ((ZPK_LDS u16*)sout.rec[0])[lane], rm = ((ZPK_LDS u16*)sout.rec[1])[lane], rl = ((ZPK_LDS u16*)sout.rec[2])[lane];
                const u32 no = ro >> 11, nm = rm >> 11, nl = rl >> 11;         // record = state | count << 11: the count's low bits of the state go out
                u32 nn = no;
                lo64 = ro & ((1u << no) - 1u);
                lo64 |= (u64)(rm & ((1u << nm) - 1u)) << nn; nn += nm;
                lo64 |= (u64)(rl & ((1u << nl) - 1u)) << nn; nn += nl;
                lo64 |= (u64)p_xl << nn; nn += p_nb & 0xFFu;
                lo64 |= (u64)p_xm << nn; nn += (p_nb >> 8) & 0xFFu;         // <= 58 so far
                const u32 nxo = p_nb >> 16;
                lo64 |= (u64)p_xo << nn;
                if (nn + nxo > 64u) hi64 = (u64)p_xo >> (64u - nn);          // (then nn >= 34: the shift is 1..30)
                nbits = nn + nxo;
            }
            const u32 x = wave_scan_add(nbits);
            const u32 total = (u32)__builtin_amdgcn_readlane((int)x, 63);
            if (nbits) {                                                     // sequences are put in DESCENDING order: the ones after this lane's come first
                const u32 off = carry_n + total - x, w = off >> 5, sft = off & 31u;
                const u64 A = lo64 << sft, B = (hi64 << sft) | ((lo64 >> 32) >> (32u - sft));
                ZPK_LDS u32* const bw = (ZPK_LDS u32*)sout.bits + w;
                __hip_atomic_fetch_or(bw, (u32)A, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_or(bw + 1, (u32)(A >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_or(bw + 2, (u32)B, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_or(bw + 3, (u32)(B >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            wave_mem_fence();
            const u32 nby = (carry_n + total) >> 3;                          // finished bytes
            if (p + nby > limit) { ok = false; break; }
            if (lo > 0) {                                                    // the next group: its codes and chain words, and the list words of the one after it
                const u32 lo2 = lo > WAVE ? lo - WAVE : 0u;
                prep_group(q_ahead, lo - lo2);
                q_ahead = lo2 > 0 ? load_group(lo2) : 0ull;
            }
            for (u32 c = (u32)lane * 16u; c < nby; c += WAVE * 16u) {
                const u128 v = lds_ld128((lds_cp8)((const ZPK_LDS u8*)sout.bits + c));
                if (c + 16u <= nby) st128(p + c, v); else gstore_upto16(p + c, v, nby - c);
            }
            const u32 cb = ((const ZPK_LDS u8*)sout.bits)[nby];              // the unfinished byte moves to the front
            wave_mem_fence();
            for (u32 c = (u32)lane * 16u; c < sizeof(sout.bits); c += WAVE * 16u) lds_st128((lds_p8)((ZPK_LDS u8*)sout.bits + c), u128{0, 0});
            wave_mem_fence();
            if (lane == 0) ((ZPK_LDS u32*)sout.bits)[0] = cb;
            wave_mem_fence();
            p += nby;
            carry_n = (carry_n + total) & 7u;
            hi = lo;
        }
        ZeBits b; b.ptr = p; b.n = carry_n; b.c = ((const ZPK_LDS u8*)sout.bits)[0];
        ZeState sl, so, sm;
        so.v = (u32)__builtin_amdgcn_readlane((int)r_state, 0); sm.v = (u32)__builtin_amdgcn_readlane((int)r_state, 1); sl.v = (u32)__builtin_amdgcn_readlane((int)r_state, 2);
        lane0_guard();
        if (lane == 0 && ok) {
            if (tm.mode != 1) { b.add(sm.v, tm.log); b.flush_exact(); }
            if (to.mode != 1) { b.add(so.v, to.log); b.flush_exact(); }
            if (tl.mode != 1) { b.add(sl.v, tl.log); b.flush_exact(); }
            b.add(1, 1); b.flush_exact();                                   // end mark
            seq_bytes = (u32)(b.ptr - sq) + (b.n ? 1u : 0u);
        }
    }
    seq_bytes = uni(seq_bytes);
    wave_mem_fence();
    if (seq_bytes == 0) return 0;
    const u32 total = lit_section + seq_bytes;
    if (total >= n) return 0;
    rep_hist = last_off;
    return total;
}

template <int HLOG>
__device__ inline u32 zstde_block(Lz4EncSharedT<HLOG>& she, ZstdEncShared& sh, const u8* src, u32 n, u8* dst, u64* seqs, int lane, int effort,
                                  u64 abs_base, u32& rep_hist)
{
    bool table_saved = false;
    const u32 r = zstde_block_inner(she, sh, src, n, dst, seqs, lane, effort, abs_base, table_saved, rep_hist);
    if (table_saved) {
        wave_mem_fence();
        const u8* const save = (const u8*)(seqs + ZE_MAXSEQ + ZE_BLOCK / 8u + 8u);
        for (u32 c = (u32)lane * 16u; c < ZE_TABLE_SAVE; c += WAVE * 16u) *(u128*)((u8*)&she + c) = ld128(save + c);
        wave_mem_fence();
    }
    return r;
}

// k_encode<12> takes the entries of level <= 2 (and every stored entry), k_encode<13> those of levels 3..5, k_encode<14> those of
// level >= 6: same code, a hash table two / four times the size — the level decides the kernel, not the format
template <int HLOG>
__global__ __launch_bounds__(64, HLOG == LZ4E_HASH_LOG ? ZE_WAVES_PER_SIMD : (HLOG == LZ4E_HASH_LOG_MID ? 2 : 1)) void k_encode(const u8* __restrict__ src, const zpk_encode_desc* __restrict__ desc, u64 n,
                                               u8* __restrict__ dst, zpk_encode_result* __restrict__ res, u64* __restrict__ seq_scratch,
                                               u32* __restrict__ queue, const u32* __restrict__ order)
{
    const int lane = lane_id();
    if (order && queue[C_ENC_CLASS + (HLOG - LZ4E_HASH_LOG)] == 0) return;            // nothing of this instantiation's levels in the batch (k_enc_order_count looked)
    __shared__ Lz4EncSharedT<HLOG> she;
    static_assert(sizeof(ZstdEncShared) == ZE_SHZ_BYTES && ZE_TABLE_SAVE <= sizeof(Lz4EncSharedT<HLOG>), "the predefined tables overlay the hash table");
    ZstdEncShared& shz = *(ZstdEncShared*)((u8*)&she + ZE_SHZ_OFF);
    u64* const seqs = seq_scratch + (u64)blockIdx.x * ZE_WG_SCRATCH;
    {   // encoder tables of the three predefined distributions, once per workgroup: built in place, then parked in the HBM scratch
        for (int i = lane; i < 36; i += WAVE) shz.symtab[0][i] = Z_LL_BASE[i] | ((u32)Z_LL_BITS[i] << 24);
        for (int i = lane; i < 53; i += WAVE) shz.symtab[1][i] = Z_ML_BASE[i] | ((u32)Z_ML_BITS[i] << 24);
        lane0_guard();
        if (lane == 0) {
            ze_build_ctable(shz, T_LL, Z_LL_DEF, 36, 6);
            ze_build_ctable(shz, T_OF, Z_OF_DEF, 29, 5);
            ze_build_ctable(shz, T_ML, Z_ML_DEF, 53, 6);
        }
        __syncthreads();
        u8* const img = (u8*)(seqs + ZE_MAXSEQ + ZE_BLOCK / 8u + 8u) + ZE_TABLE_SAVE;
        for (u32 c = (u32)lane * 16u; c < ZE_SHZ_BYTES; c += WAVE * 16u) st128(img + c, *(const u128*)((const u8*)&shz + c));
        wave_mem_fence();
    }
    // entries are pulled from a counter, not dealt out by stride: an entry is ~100 ms of one wave, a batch is only a few rounds of the
    // resident workgroups, and the classes differ by 5x — whoever is free takes the next one
    // (not dequeue() of zpk_device.h: the ticket is looked up in `order` between the compare and the second guard, and this kernel's
    // instruction stream is left as it was measured)
    for (;;) {
    lane0_guard();
    u32 ticket = 0;
    if (lane == 0) ticket = atomicAdd(&queue[C_ENC_HEAD + (HLOG - LZ4E_HASH_LOG)], 1u);
    if (uni(ticket) >= n) break;
    const u64 w = order ? uni(order[uni(ticket)]) : uni(ticket);                  // largest entries first (k_enc_order_*)
    lane0_guard();
    zpk_encode_desc d = desc[w];
    const bool piece = (d.method & ZPK_EF_PIECE) != 0;                            // a run of BLOCKS of a larger frame (round 5): no frame header, no end of frame, no hash of its own
    d.method &= ~ZPK_EF_PIECE;
    if (HLOG != ((d.method == ZPK_METHOD_NONE || d.level <= 2) ? LZ4E_HASH_LOG : (d.level <= 5 ? LZ4E_HASH_LOG_MID : LZ4E_HASH_LOG_HC))) continue;      // another instantiation's entry
    zpk_encode_result r; r.status = R_OK; r.detail = 0; r.comp_size = 0; r.hash = 0;
    const u8* in = uni_ptr(src + d.src_offset);
    u8* out = uni_ptr(dst + d.dst_offset);
    const u64 len = uni64(d.size), cap = uni64(d.dst_capacity);
    if (d.method == ZPK_METHOD_NONE) {
        if (cap < len) r.status = R_BUFFER_TOO_SMALL;                             // lib/zpack_write.c:167
        else {
            for (u64 i = (u64)lane * 16; i < len; i += WAVE * 16) gcopy_upto16(out + i, in + i, (u32)(len - i < 16 ? len - i : 16));
            r.comp_size = len;
        }
    } else if (d.method == ZPK_METHOD_LZ4) {
        const u64 nblocks = (len + 65535) >> 16;
        const u32 hdr = piece ? 0u : 7u;
        if (cap < hdr + nblocks * 4 + len + (piece ? 0u : 4u)) r.status = R_COMPRESS_FAILED;      // cannot hold the all-stored worst case
        else {
            lane0_guard();
            if (lane == 0 && !piece) { st32(out, 0x184D2204u); st8(out + 4, 0x40); st8(out + 5, 0x40); st8(out + 6, 0xC0); }
            u8* op = out + hdr;
            for (u64 b = 0; b < nblocks; b++) {
                const u8* bsrc = in + (b << 16);
                const u32 bn = (u32)(len - (b << 16) < 65536 ? len - (b << 16) : 65536);
                const u32 c = lz4e_block(she, bsrc, bn, op + 4, lane, seqs, nullptr, 4u, lz4e_effort(d.level), b << 16);
                wave_mem_fence();
                if (c == 0) {
                    lane0_guard();
                    if (lane == 0) st32(op, bn | 0x80000000u);
                    for (u32 i = (u32)lane * 16; i < bn; i += WAVE * 16) gcopy_upto16(op + 4 + i, bsrc + i, bn - i);
                    op += 4 + bn;
                } else {
                    lane0_guard();
                    if (lane == 0) st32(op, c);
                    op += 4 + c;
                }
            }
            lane0_guard();
            if (!piece) { if (lane == 0) st32(op, 0); op += 4; }                  // EndMark
            r.comp_size = (u64)(op - out);
        }
    } else if (d.method == ZPK_METHOD_ZSTD) {
        // single-segment frame header + blocks of <= 64 KiB: Compressed (raw literals, predefined FSE), RLE or Raw
        const u32 fcs_bytes = len < 256 ? 1 : (len < 65536 + 256 ? 2 : (len <= 0xFFFFFFFFull ? 4 : 8));
        const u64 nblocks = len ? (len + ZE_BLOCK - 1) / ZE_BLOCK : 1;
        const u32 zhdr = piece ? 0u : 5u + fcs_bytes;
        if (cap < zhdr + nblocks * 3 + len) r.status = R_COMPRESS_FAILED;
        else {
            lane0_guard();
            if (lane == 0 && !piece) {
                st32(out, 0xFD2FB528u);
                st8(out + 4, (u8)(0x20 | ((fcs_bytes == 1 ? 0 : fcs_bytes == 2 ? 1 : fcs_bytes == 4 ? 2 : 3) << 6)));
                const u64 f = fcs_bytes == 2 ? len - 256 : len;
                for (u32 i = 0; i < fcs_bytes; i++) st8(out + 5 + i, (u8)(f >> (8 * i)));
            }
            u8* op = out + zhdr;
            u32 rep_hist = 0;                                                   // 0 = the frame has not emitted a sequence yet (its initial repeat offset 1 is not used)
            for (u64 b = 0; b < nblocks; b++) {
                const u64 pos = b * ZE_BLOCK;
                const u32 bn = (u32)(len - pos < ZE_BLOCK ? len - pos : ZE_BLOCK);
                const bool last = !piece && b + 1 == nblocks;               // (the frame a piece belongs to is closed by whoever assembles it: an empty last block)
                // RLE when every byte equals the first
                bool same = bn > 1;
                const u8 first = bn ? ld8(in + pos) : 0;
                for (u32 i = lane; i < bn && same; i += WAVE) if (ld8(in + pos + i) != first) same = false;
                const bool rle = bn > 1 && __ballot(!same) == 0;
                u32 csize = 0;
                if (!rle && bn >= 64) csize = zstde_block(she, shz, in + pos, bn, op + 3, seqs, lane, lz4e_effort(d.level), pos, rep_hist);
                const u32 btype = rle ? 1u : (csize ? 2u : 0u);
                const u32 bh = (last ? 1u : 0u) | (btype << 1) | ((csize ? csize : bn) << 3);
                lane0_guard();
                if (lane == 0) { st8(op, (u8)bh); st8(op + 1, (u8)(bh >> 8)); st8(op + 2, (u8)(bh >> 16)); if (rle) st8(op + 3, first); }
                if (rle) op += 4;
                else if (csize) op += 3 + csize;
                else {
                    for (u32 i = (u32)lane * 16; i < bn; i += WAVE * 16) gcopy_upto16(op + 3 + i, in + pos + i, bn - i);
                    op += 3 + bn;
                }
                wave_mem_fence();
            }
            r.comp_size = (u64)(op - out);
        }
    } else {
        r.status = R_COMP_METHOD_INVALID;                                          // lib/zpack_write.c:219-220
    }
    if (r.status == R_OK && !piece) r.hash = xxh3_64_wave(in, len, lane);          // lib/zpack_write.c:256 (a piece: the entry's hash is computed over all of it elsewhere)
    lane0_guard();
    if (lane == 0) res[w] = r;
    }
}

// ---- K7: compressed-size exclusive scan + compaction (replaces the serial `write_offset += comp_size` of
// lib/zpack_write.c:338 for a whole batch: entry offsets = prefix sum of the compressed sizes, payloads gathered
// back-to-back into one packed stream — the data section of the archive) -------------------------------------------
#define PK_BLOCK 1024u                            // entries per scan block (256 threads x 4)

__device__ __forceinline__ u64 pk_size(const zpk_encode_result* res, u64 i, u64 n)
{
    if (i >= n) return 0;
    const zpk_encode_result r = res[i];
    return r.status == R_OK ? r.comp_size : 0;    // failed entries take no room
}

// MODE 0: bytes of the entry; MODE 1: number of PK_SPAN pieces the gather cuts it into
#define PK_SPAN (16u << 10)
template <int MODE> __device__ __forceinline__ u64 pk_val(const zpk_encode_result* res, u64 i, u64 n)
{
    const u64 sz = pk_size(res, i, n);
    return MODE == 0 ? sz : (sz + PK_SPAN - 1) / PK_SPAN;
}

// pass 1: block totals; pass 2 (one workgroup): exclusive scan of the block totals in place, grand total to offsets[n];
// pass 3: offsets[i] = block base + exclusive scan inside the block
template <int MODE>
__global__ __launch_bounds__(256) void k_pack_block_sums(const zpk_encode_result* __restrict__ res, u64 n, u64* __restrict__ block_sums)
{
    __shared__ u64 part[4];
    const u64 i0 = (u64)blockIdx.x * PK_BLOCK + threadIdx.x * 4u;
    u64 v = pk_val<MODE>(res, i0, n) + pk_val<MODE>(res, i0 + 1, n) + pk_val<MODE>(res, i0 + 2, n) + pk_val<MODE>(res, i0 + 3, n);
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += shfl_xor64(v, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) block_sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(256) void k_pack_scan_blocks(u64* __restrict__ block_sums, u64 nblocks, u64* __restrict__ total_out)
{
    __shared__ u64 carry_sh[5];
    u64 carry = 0;
    for (u64 b0 = 0; b0 < nblocks; b0 += 256) {
        const u64 i = b0 + threadIdx.x;
        const u64 v = i < nblocks ? block_sums[i] : 0;
        u64 x = v;                                 // inclusive scan inside the wave, then across the four waves
        #pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 lo = (u32)__shfl_up((int)(u32)x, d, 64), hi = (u32)__shfl_up((int)(u32)(x >> 32), d, 64);
            if ((int)(threadIdx.x & 63) >= d) x += ((u64)hi << 32) | lo;
        }
        __syncthreads();
        if ((threadIdx.x & 63) == 63) carry_sh[threadIdx.x >> 6] = x;
        __syncthreads();
        u64 wbase = 0;
        for (u32 w = 0; w < (threadIdx.x >> 6); w++) wbase += carry_sh[w];
        if (i < nblocks) block_sums[i] = carry + wbase + x - v;
        const u64 chunk_total = carry_sh[0] + carry_sh[1] + carry_sh[2] + carry_sh[3];
        carry += chunk_total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_pack_offsets(const zpk_encode_result* __restrict__ res, u64 n, const u64* __restrict__ block_base,
                                                      u64* __restrict__ offsets)
{
    __shared__ u64 wsum[4];
    const u64 i0 = (u64)blockIdx.x * PK_BLOCK + threadIdx.x * 4u;
    const u64 a = pk_val<MODE>(res, i0, n), b = pk_val<MODE>(res, i0 + 1, n), c = pk_val<MODE>(res, i0 + 2, n), d = pk_val<MODE>(res, i0 + 3, n);
    const u64 v = a + b + c + d;
    u64 x = v;
    #pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const u32 lo = (u32)__shfl_up((int)(u32)x, k, 64), hi = (u32)__shfl_up((int)(u32)(x >> 32), k, 64);
        if ((int)(threadIdx.x & 63) >= k) x += ((u64)hi << 32) | lo;
    }
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = x;
    __syncthreads();
    u64 base = block_base[blockIdx.x];
    for (u32 w = 0; w < (threadIdx.x >> 6); w++) base += wsum[w];
    u64 o = base + x - v;
    if (i0 < n) offsets[i0] = o;
    o += a; if (i0 + 1 < n) offsets[i0 + 1] = o;
    o += b; if (i0 + 2 < n) offsets[i0 + 2] = o;
    o += c; if (i0 + 3 < n) offsets[i0 + 3] = o;
}

// gather: PK_SPAN bytes of one entry per wave, 16 bytes per lane per access (slots and the packed stream may sit at any
// alignment); every byte is read once and written once
__global__ __launch_bounds__(256) void k_pack_gather(const u8* __restrict__ slots, const zpk_encode_desc* __restrict__ desc,
                                                     const zpk_encode_result* __restrict__ res, u64 n, const u64* __restrict__ offsets,
                                                     const u64* __restrict__ span_first, u8* __restrict__ packed, u64 packed_cap)
{
    // work item = (entry, span): span_first[e] = index of entry e's first span; binary search maps a wave to its entry
    const u64 w = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = lane_id();
    const u64 nspans = span_first[n];
    if (w >= nspans) return;
    u64 lo = 0, hi = n;                             // last e with span_first[e] <= w
    while (hi - lo > 1) { const u64 mid = (lo + hi) >> 1; if (span_first[mid] <= w) lo = mid; else hi = mid; }
    const u64 e = lo;
    const u64 size = pk_size(res, e, n);
    const u64 from = (w - span_first[e]) * (u64)PK_SPAN;
    if (from >= size) return;
    const u64 len = size - from < PK_SPAN ? size - from : PK_SPAN;
    const u64 dst_off = offsets[e] + from;
    if (dst_off > packed_cap || len > packed_cap - dst_off) return;      // caller's buffer too small: offsets[n] tells
    const u8* s = slots + desc[e].dst_offset + from;
    u8* d = packed + dst_off;
    for (u64 i = (u64)lane * 16; i < len; i += WAVE * 16) gcopy_upto16(d + i, s + i, (u32)(len - i < 16 ? len - i : 16));
}

extern "C" {

// offsets[0..n] (device, u64): offsets[i] = start of entry i's payload in the packed stream, offsets[n] = its length.
// packed may be NULL (sizes only).  Everything is enqueued on `stream`; nothing synchronises.
}  // extern "C"
// (the bodies without the codec lock: the host path's pipeline launches from a second thread while the calling thread holds it)
static int pack_launch(zpk_codec* c, const uint8_t* slots, const zpk_encode_desc* desc, const zpk_encode_result* results,
                       uint64_t n, uint8_t* packed, uint64_t packed_cap, uint64_t* offsets, uint64_t max_entry_size, hipStream_t st)
{
    if (n == 0) { HIPCHK(c, hipMemsetAsync(offsets, 0, sizeof(u64), st)); return ZPK_OK; }
    if (n > 0x7FFFFFFFull) return ZPK_E_INVALID;
    const u64 nblocks = (n + PK_BLOCK - 1) / PK_BLOCK;
    int rc;
    if ((rc = grow(c, c->d_pack, 2 * nblocks * sizeof(u64) + (n + 1) * sizeof(u64) + 64))) return rc;
    u64* const block_sums = (u64*)c->d_pack;
    u64* const span_blocks = block_sums + nblocks;
    u64* const span_first = span_blocks + nblocks;
    hipLaunchKernelGGL(k_pack_block_sums<0>, dim3((u32)nblocks), dim3(256), 0, st, results, n, block_sums);
    hipLaunchKernelGGL(k_pack_scan_blocks, dim3(1), dim3(256), 0, st, block_sums, nblocks, offsets + n);
    hipLaunchKernelGGL(k_pack_offsets<0>, dim3((u32)nblocks), dim3(256), 0, st, results, n, block_sums, offsets);
    if (packed) {
        hipLaunchKernelGGL(k_pack_block_sums<1>, dim3((u32)nblocks), dim3(256), 0, st, results, n, span_blocks);
        hipLaunchKernelGGL(k_pack_scan_blocks, dim3(1), dim3(256), 0, st, span_blocks, nblocks, span_first + n);
        hipLaunchKernelGGL(k_pack_offsets<1>, dim3((u32)nblocks), dim3(256), 0, st, results, n, span_blocks, span_first);
        // upper bound of the number of spans without reading the device: every entry has at most ceil(max/PK_SPAN) of them
        const u64 per = (max_entry_size + PK_SPAN - 1) / PK_SPAN;
        const u64 waves = n * (per ? per : 1);
        if (waves > 0x3FFFFFFFull) return ZPK_E_INVALID;
        if (c->profiling) (void)hipEventRecord(c->kev[ZPK_K_PACK][0], st);
        hipLaunchKernelGGL(k_pack_gather, dim3((u32)((waves + 3) / 4)), dim3(256), 0, st, slots, desc, results, n, offsets, span_first, packed, packed_cap);
        if (c->profiling) (void)hipEventRecord(c->kev[ZPK_K_PACK][1], st);
    }
    HIPCHK(c, hipGetLastError());
    return ZPK_OK;
}
extern "C" {
int zpk_codec_pack_batch_device(zpk_codec* c, const uint8_t* slots, const zpk_encode_desc* desc, const zpk_encode_result* results,
                                uint64_t n, uint8_t* packed, uint64_t packed_cap, uint64_t* offsets, uint64_t max_entry_size, void* stream)
{
    if (!c || !offsets || (n && (!desc || !results))) return ZPK_E_INVALID;
    CodecLock lk(c);
    HIPCHK(c, hipSetDevice(c->device));
    return pack_launch(c, slots, desc, results, n, packed, packed_cap, offsets, max_entry_size, stream ? (hipStream_t)stream : c->stream);
}

size_t zpk_codec_compress_bound(uint32_t method, size_t n) { return enc_compress_bound(method, n); }       // (enc_plan.h)

}  // extern "C"
// ---- largest entries first: an entry is tens of ms of ONE wave and a batch is a few rounds of the resident waves, so a 1 MiB entry that
// is taken last runs on alone (the reasoning and the counting sort of k_order_* for the decode lists, over the descriptors themselves)
__global__ __launch_bounds__(256) void k_enc_order_count(const zpk_encode_desc* __restrict__ desc, u64 n, u32* __restrict__ counters)
{
    __shared__ u32 h[ORD_CLASSES];
    if (threadIdx.x < ORD_CLASSES) h[threadIdx.x] = 0;
    __syncthreads();
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    const int lane = lane_id();
    const int b = k < n ? order_class(desc[k].size) : -1;
    if (k < n) {                                                                       // which instantiations have work at all (an empty one leaves before its set-up)
        const zpk_encode_desc& d = desc[k];
        const u32 m = d.method & ~ZPK_EF_PIECE;
        const int cls = (m == ZPK_METHOD_NONE || d.level <= 2) ? 0 : (d.level <= 5 ? 1 : 2);
        for (int c3 = 0; c3 < 3; c3++) { const u64 any = __ballot(cls == c3); if (any && lane == __ffsll((long long)any) - 1 && counters[C_ENC_CLASS + c3] == 0) atomicOr(&counters[C_ENC_CLASS + c3], 1u); }
    }
    u32 rank, count;
    order_wave_rank(b, lane, rank, count);
    if (b >= 0 && rank == 0) atomicAdd(&h[b], count);
    __syncthreads();
    if (threadIdx.x < ORD_CLASSES && h[threadIdx.x]) {
        atomicAdd(&counters[C_ORDER_HIST + threadIdx.x], h[threadIdx.x]);
        atomicMax(&counters[C_ORDER_SPAN], (u32)threadIdx.x); atomicMax(&counters[C_ORDER_SPAN_INV], (u32)(ORD_CLASSES - 1 - threadIdx.x));
    }
}
__global__ __launch_bounds__(256) void k_enc_order_fill(const zpk_encode_desc* __restrict__ desc, u64 n, u32* __restrict__ order, u32* __restrict__ counters)
{
    __shared__ u32 wcount[4][ORD_CLASSES], base[ORD_CLASSES];
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (order_single_class(counters)) { if (k < n) order[k] = (u32)k; return; }          // a uniform batch keeps its order
    if (threadIdx.x < 4 * ORD_CLASSES) (&wcount[0][0])[threadIdx.x] = 0;
    __syncthreads();
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int b = k < n ? order_class(desc[k].size) : -1;
    u32 rank, count;
    order_wave_rank(b, lane, rank, count);
    if (b >= 0 && rank == 0) wcount[w][b] = count;
    __syncthreads();
    if (threadIdx.x < ORD_CLASSES) {
        const int cl = threadIdx.x;
        const u32 total = wcount[0][cl] + wcount[1][cl] + wcount[2][cl] + wcount[3][cl];
        u32 before = 0;
        for (int j = 0; j < cl; j++) before += counters[C_ORDER_HIST + j];
        base[cl] = total ? before + atomicAdd(&counters[C_ORDER_FILL + cl], total) : 0;
    }
    __syncthreads();
    if (b >= 0) {
        u32 at = base[b] + rank;
        for (int j = 0; j < w; j++) at += wcount[j][b];
        order[at] = (u32)k;
    }
}

static int encode_launch(zpk_codec* c, const uint8_t* src, const zpk_encode_desc* desc, uint64_t n, uint8_t* dst, zpk_encode_result* results, hipStream_t st)
{
    if (n == 0) return ZPK_OK;
    if (n > 0x7FFFFFFFull) return ZPK_E_INVALID;
    const u32 grid = (u32)(n < ZPK_ENC_GRID_MAX ? n : ZPK_ENC_GRID_MAX);       // persistent: bounds the sequence scratch
    int rc;
    // (one scratch region per WORKGROUP of the launch: a batch of a few entries — the streaming writer's steps — takes a few MB, not
    // the 1.8 GB of a full grid)
    if ((rc = grow(c, c->d_seq, (u64)grid * ZE_WG_SCRATCH * sizeof(u64)))) return rc;
    if (c->profiling) (void)hipEventRecord(c->kev[ZPK_K_ENCODE][0], st);
    HIPCHK(c, hipMemsetAsync(c->d_counters, 0, N_COUNTERS * sizeof(u32), st));   // the two kernels' dequeue heads, the order histogram
    const u32* order = nullptr;
    if (n >= c->opt.enc_order_min) {
        if ((rc = grow(c, c->wave.d_lists, (u64)N_LIST_SLOTS * n * sizeof(u32)))) return rc;     // (sized like the decode lists)
        hipLaunchKernelGGL(k_enc_order_count, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, desc, n, c->d_counters);
        hipLaunchKernelGGL(k_enc_order_fill, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, desc, n, c->wave.d_lists, c->d_counters);
        order = c->wave.d_lists;
    }
    hipLaunchKernelGGL(k_encode<LZ4E_HASH_LOG>, dim3(grid), dim3(64), 0, st, src, desc, n, dst, results, c->d_seq, c->d_counters, order);
    hipLaunchKernelGGL(k_encode<LZ4E_HASH_LOG_MID>, dim3(grid), dim3(64), 0, st, src, desc, n, dst, results, c->d_seq, c->d_counters, order);
    hipLaunchKernelGGL(k_encode<LZ4E_HASH_LOG_HC>, dim3(grid), dim3(64), 0, st, src, desc, n, dst, results, c->d_seq, c->d_counters, order);
    if (c->profiling) (void)hipEventRecord(c->kev[ZPK_K_ENCODE][1], st);
    HIPCHK(c, hipGetLastError());
    return ZPK_OK;
}
extern "C" {
int zpk_codec_encode_batch_device(zpk_codec* c, const uint8_t* src, uint64_t src_size, const zpk_encode_desc* desc, uint64_t n,
                                  uint8_t* dst, uint64_t dst_size, zpk_encode_result* results, void* stream)
{
    (void)src_size; (void)dst_size;
    if (!c || (n && (!desc || !results))) return ZPK_E_INVALID;
    CodecLock lk(c);
    HIPCHK(c, hipSetDevice(c->device));
    return encode_launch(c, src, desc, n, dst, results, stream ? (hipStream_t)stream : c->stream);
}
}  // extern "C"

// (Round 4 measured the write side as a three-stage pipeline — a second thread gathering + uploading piece k + 1 into its own pinned
// pair beside the encode of piece k beside the download + scatter of piece k - 1, pieces of 4608 entries: 114-121 ms for 40 000 x 64 KiB
// against 96-103 ms one after the other on the same box (profiles/r04/r04_host_write_pipeline_ab.txt).  Upload is 2/3 of the call and
// it is bound by the host's memory system — gather read + write, DMA read, and the download's DMA write + scatter on top: run beside
// each other they slow each other down by more than the overlap gains.  Removed; the stages run one after the other.)

extern "C" {
// Entries of at least c->opt.enc_split_min bytes go to the device as 512 KiB pieces, one wave each, and come back as ONE frame (enc_plan.h: which
// entries, their pieces, the frame's header and end, the entry's verdict); the packed stream keeps the pieces in order.  The entry's hash
// is that of the whole plaintext (the two kernels of xxh3_span.h).
// (dsrc: zpk_codec_encode_batch_dsrc — src_ptrs are DEVICE pointers, gathered into the same staging by one launch of k_span_copy)
static int encode_batch_host_any(zpk_codec* c, const uint8_t* const* src_ptrs, const zpk_encode_desc* desc, uint64_t n,
                                 uint8_t* const* dst_ptrs, zpk_encode_result* results, bool dsrc, const Planes& pl = Planes())
{
    if (!c || (n && (!desc || !results || !src_ptrs || !dst_ptrs))) return ZPK_E_INVALID;
    if (n == 0) return ZPK_OK;
    CodecLock lk(c);
    c->last.no_planes();
    HIPCHK(c, hipSetDevice(c->device));
    if (planes_check(c, pl.elem, n)) return ZPK_E_INVALID;
    // the pointer rule (zpk_codec.hip, PtrRule): before anything is enqueued
    PtrRule rule(c);
    if (dsrc && rule.batch("source", n, [&](u64 i) { return src_ptrs[i]; }, [&](u64 i) { return (u64)desc[i].size; })) return ZPK_E_INVALID;
    if (bases_check(c, rule, pl, n, [&](u64 i) { return (u64)desc[i].size; }, nullptr)) return ZPK_E_INVALID;
    const u64 split_min = c->opt.enc_split_min;
    u64 np = 0, nsplit = 0;
    for (u64 i = 0; i < n; i++) { np += enc_piece_count(split_min, desc[i]); nsplit += enc_is_split(split_min, desc[i]); }
    if (np > 0x7FFFFFFFull) return ZPK_E_INVALID;
    // the call's tables, one block: the pieces (entry i is pieces [first[i], first[i + 1])), their results and packed offsets; per entry
    // where its payload goes; per entry in pieces its span and hash
    const bool framed = np != n;
    u8* at = (u8*)malloc(np * (sizeof(zpk_encode_desc) + 8) + (n + 2) * 8 + (framed ? np * sizeof(zpk_encode_result) + n * sizeof(u8*) : 0) +
                         nsplit * (sizeof(zpk_span) + 8));
    struct Free { void* p; ~Free() { free(p); } } guard = { at };
    if (!at) return ZPK_E_NOMEM;
    auto take = [&](u64 bytes) { u8* const p = at; at += bytes; return p; };                  // (every size a multiple of 8)
    zpk_encode_desc* const hd = (zpk_encode_desc*)take(np * sizeof(zpk_encode_desc));
    u64* const first = (u64*)take((n + 1) * 8);
    u64* const h_off = (u64*)take((np + 1) * 8);
    zpk_encode_result* const hr = framed ? (zpk_encode_result*)take(np * sizeof(zpk_encode_result)) : results;
    u8** const payload = framed ? (u8**)take(n * sizeof(u8*)) : nullptr;
    zpk_span* const spans = (zpk_span*)take(nsplit * sizeof(zpk_span));
    u64* const h_hash = (u64*)take(nsplit * 8);
    u64 in_total = 0, out_total = 0, k = 0, ns = 0, part_blocks = 0, max_cap = 0;
    for (u64 i = 0; i < n; i++) {
        first[i] = k;
        const EncSpan sp = enc_emit_entry(split_min, desc[i], in_total, hd + k, out_total, max_cap);
        k += enc_piece_count(split_min, desc[i]);
        if (enc_is_split(split_min, desc[i])) { spans[ns++] = zpk_span{ sp.off, sp.len, part_blocks }; part_blocks += xxh3_span_blocks(sp.len); }
        in_total += span_copy_write_slot(desc[i].size);                               // (span_copy_plan.h states the layout for both kinds of source)
    }
    first[n] = k;
    int rc;
    if ((rc = grow(c, c->d_src, in_total + 64)) || (rc = grow(c, c->d_dst, out_total + 64)) ||
        (rc = grow(c, c->d_desc, np * sizeof(zpk_encode_desc))) ||
        (rc = grow(c, c->d_res, np * sizeof(zpk_encode_result)))) return rc;
    hipError_t e = hipSuccess;
    // the sources go up, entry i to its place in the staging, hd[first[i]].src_offset (zpk_codec.hip, stage_sources)
    if ((rc = stage_sources(c, src_ptrs, dsrc, n, [&](u64 i) { return (u64)hd[first[i]].src_offset; }, [&](u64 i) { return (u64)desc[i].size; }, in_total, c->stream, e, pl))) return rc;
    if (e == hipSuccess) e = hipMemcpyAsync(c->d_desc, hd, np * sizeof(zpk_encode_desc), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "H2D: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    rc = zpk_codec_encode_batch_device(c, c->d_src, in_total, (const zpk_encode_desc*)c->d_desc, np, c->d_dst, out_total,
                                       (zpk_encode_result*)c->d_res, c->stream);
    if (rc) return rc;
    // the hashes of the split entries
    if ((rc = xxh3_spans_launch(c, c->d_src, spans, nsplit, part_blocks, h_hash, c->stream))) return rc;
    // the payloads come back as ONE packed stream (device scan + compaction), not as n small copies out of bound-sized slots
    if ((rc = grow(c, c->d_packed, out_total + 64)) ||
        (rc = grow(c, c->d_packoff, (np + 1) * sizeof(u64))) ||
        (rc = zpk_codec_pack_batch_device(c, c->d_dst, (const zpk_encode_desc*)c->d_desc, (const zpk_encode_result*)c->d_res, np,
                                          c->d_packed, out_total, (u64*)c->d_packoff, max_cap, c->stream))) return rc;
    e = hipMemcpyAsync(hr, c->d_res, np * sizeof(zpk_encode_result), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_off, c->d_packoff, (np + 1) * sizeof(u64), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && framed) {
        // an entry in pieces: its verdict (enc_verdict: that of its first failing piece, else its frame against what the caller gave),
        // and where its blocks go: behind its frame header, which — like the end of the frame — the host writes itself, here
        ns = 0;
        for (u64 i = 0; i < n; i++) {
            const u64 a = first[i], b = first[i + 1];
            payload[i] = dst_ptrs[i];
            if (b - a == 1) { results[i] = hr[a]; continue; }
            const zpk_encode_result* failed = nullptr;
            for (u64 j = a; j < b && !failed; j++) if (hr[j].status) failed = &hr[j];
            const EncEnvelope E = enc_envelope(desc[i].method, desc[i].size);
            const u64 blocks = h_off[b] - h_off[a];
            results[i] = enc_verdict(failed, blocks, E.hl, E.tl, desc[i].dst_capacity, desc[i].method, h_hash[ns++]);
            if (results[i].status != 0 || E.hl == 0) continue;                         // (a stored entry has no envelope)
            memcpy(dst_ptrs[i], E.hdr, E.hl);
            memcpy(dst_ptrs[i] + E.hl + blocks, E.trl, E.tl);
            payload[i] += E.hl;
        }
    }
    if (e == hipSuccess && h_off[np]) {
        // the packed stream comes back through the pinned staging buffers, scattered piece by piece (zpk_codec.hip, d2h_scatter)
        auto payload_len = [&](u64 i) -> u64 { return results[i].status != 0 ? 0ull : h_off[first[i + 1]] - h_off[first[i]]; };
        const int src = d2h_scatter(c, c->d_packed, h_off[np], n, framed ? payload : dst_ptrs, [&](u64 i) { return h_off[first[i]]; }, payload_len, e);
        if (src) return src;
    }
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "encode: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    return ZPK_OK;
}

int zpk_codec_encode_batch_host(zpk_codec* c, const uint8_t* const* src_ptrs, const zpk_encode_desc* desc, uint64_t n,
                                uint8_t* const* dst_ptrs, zpk_encode_result* results)
{
    return encode_batch_host_any(c, src_ptrs, desc, n, dst_ptrs, results, false);
}

int zpk_codec_encode_batch_dsrc(zpk_codec* c, const uint8_t* const* d_src_ptrs, const zpk_encode_desc* desc, uint64_t n,
                                uint8_t* const* dst_ptrs, zpk_encode_result* results)
{
    return encode_batch_host_any(c, d_src_ptrs, desc, n, dst_ptrs, results, true);
}

// ... whose entry i has elements of elem[i] bytes (plane_copy_plan.h) and the base d_base[i] (delta_copy_plan.h): the staging, and with it
// everything behind it, holds the stored bytes — split(plain XOR base)
int zpk_codec_encode_batch_dsrc_delta(zpk_codec* c, const uint8_t* const* d_src_ptrs, const zpk_encode_desc* desc, uint64_t n,
                                      uint8_t* const* dst_ptrs, zpk_encode_result* results, const uint8_t* elem, const uint8_t* const* d_base)
{
    return encode_batch_host_any(c, d_src_ptrs, desc, n, dst_ptrs, results, true, Planes{ elem, d_base });
}

int zpk_codec_encode_batch_dsrc_planes(zpk_codec* c, const uint8_t* const* d_src_ptrs, const zpk_encode_desc* desc, uint64_t n,
                                       uint8_t* const* dst_ptrs, zpk_encode_result* results, const uint8_t* elem)
{
    return zpk_codec_encode_batch_dsrc_delta(c, d_src_ptrs, desc, n, dst_ptrs, results, elem, nullptr);
}

}  // extern "C"

// ---- large entries that are ALREADY in device memory (zpk_codec_encode_big_device): the pieces of the host path above, and the frame put
// together on the device — no host between the encode and the finished frame.  The pieces are compressed into the codec's staging
// (slots of zpk_codec_compress_bound bytes), one scan over their sizes says where each lands, k_big_gather moves them into the caller's
// slot behind the frame header, k_big_close writes header, end of frame and the entry's result.
struct BigEncEntry {                                   // one entry written in pieces
    u64 dst_offset, dst_capacity;                  // its slot
    u32 entry, first, npieces, method;             // index among the call's entries; its pieces are [first, first + npieces)
    EncEnvelope env;                               // its frame header and end of frame (enc_plan.h)
};
static_assert(ENC_R_OK == R_OK && ENC_R_BUFFER_TOO_SMALL == R_BUFFER_TOO_SMALL && ENC_R_COMPRESS_FAILED == R_COMPRESS_FAILED, "enc_plan.h states zpack_result's values itself");

// work item = (piece, span of PK_SPAN bytes of its slot); a piece has at most `spans_per_piece` of them (its bound), those behind its
// compressed size leave at once.  Piece j of entry i lands at slot_i + hl_i + (offsets[j] - offsets[first_i]); what would land behind
// dst_capacity - tl (a frame that does not fit: k_big_close says so) is not written.  16 bytes per lane at any alignment, four loads in
// flight; every byte is read once and written once.
__global__ __launch_bounds__(256) void k_big_gather(const u8* __restrict__ slots, const zpk_encode_desc* __restrict__ pdesc,
                                                    const zpk_encode_result* __restrict__ pres, u32 np, const u64* __restrict__ offsets,
                                                    const u32* __restrict__ piece_entry, const BigEncEntry* __restrict__ big, u32 spans_per_piece,
                                                    u8* __restrict__ dst)
{
    const u32 w = uni((u32)(((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int lane = lane_id();
    const u32 p = w / spans_per_piece;
    if (p >= np) return;
    const u64 size = pk_size(pres, p, np);
    const u64 from = (u64)(w - p * spans_per_piece) * PK_SPAN;
    if (from >= size) return;
    const BigEncEntry* const B = big + piece_entry[p];
    const u64 cap = B->dst_capacity, limit = cap > B->env.tl ? cap - B->env.tl : 0;          // end of what the blocks may use, from the slot's start
    const u64 at = B->env.hl + (offsets[p] - offsets[B->first]) + from;
    if (at >= limit) return;
    u32 len = (u32)(size - from < PK_SPAN ? size - from : PK_SPAN);
    if (len > limit - at) len = (u32)(limit - at);
    const u8* const s = uni_ptr(slots + pdesc[p].dst_offset + from);
    u8* const d = uni_ptr(dst + B->dst_offset + at);
    u32 i = (u32)lane * 16u;
    for (; i + 3u * WAVE * 16u + 16u <= len; i += 4u * WAVE * 16u) {
        u128 v[4];
        #pragma unroll
        for (u32 t = 0; t < 4; t++) v[t] = ld128(s + i + t * WAVE * 16u);
        #pragma unroll
        for (u32 t = 0; t < 4; t++) st128(d + i + t * WAVE * 16u, v[t]);
    }
    for (; i < len; i += WAVE * 16u) gcopy_upto16(d + i, s + i, len - i < 16u ? len - i : 16u);
}

// one wave per entry written in pieces: its verdict (enc_verdict, the one zpk_codec_encode_batch_host above gives); header and end of
// frame go around the blocks k_big_gather has placed
__global__ __launch_bounds__(64) void k_big_close(const zpk_encode_result* __restrict__ pres, const u64* __restrict__ offsets,
                                                  const BigEncEntry* __restrict__ big, const u64* __restrict__ hashes, u8* __restrict__ dst,
                                                  zpk_encode_result* __restrict__ results)
{
    const int lane = lane_id();
    const BigEncEntry* const B = big + blockIdx.x;
    const u32 first = B->first, npieces = B->npieces, hl = B->env.hl, tl = B->env.tl;
    u32 bad = ~0u;                                                                     // first failing piece among this lane's
    for (u32 j = (u32)lane; j < npieces && bad == ~0u; j += WAVE) if (pres[first + j].status != R_OK) bad = j;
    #pragma unroll
    for (int k = 32; k >= 1; k >>= 1) { const u32 o = (u32)__shfl_xor((int)bad, k, 64); bad = o < bad ? o : bad; }
    bad = uni(bad);
    const u64 blocks = uni64(offsets[first + npieces] - offsets[first]);
    const zpk_encode_result r = enc_verdict(bad != ~0u ? pres + first + bad : nullptr, blocks, hl, tl, B->dst_capacity, B->method, hashes[blockIdx.x]);
    if (r.status == R_OK) {
        u8* const out = uni_ptr(dst + B->dst_offset);
        if ((u32)lane < hl) st8(out + lane, B->env.hdr[lane]);
        if ((u32)lane < tl) st8(out + hl + blocks + lane, B->env.trl[lane]);
    }
    lane0_guard();
    if (lane == 0) results[B->entry] = r;
}

// a pinned block of `need` bytes for one call's tables: the two blocks take turns, and a block is handed out again only when the upload
// that read it last has run (the caller records c->bigenc.ev[*slot] behind its uploads)
static int big_tables_block(zpk_codec* c, u64 need, u8** out, int* slot)
{
    const int k = (int)(c->bigenc.turn++ & 1u);
    if (!c->bigenc.ev[k]) {
        if (const hipError_t e = c->bigenc.ev[k].ready(hipEventDisableTiming)) { snprintf(c->err, sizeof(c->err), "big encode: no event: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    } else HIPCHK(c, hipEventSynchronize(c->bigenc.ev[k]));
    if (!c->bigenc.h[k].grow(need)) { snprintf(c->err, sizeof(c->err), "pinned tables: out of memory"); return ZPK_E_NOMEM; }
    *out = c->bigenc.h[k].p; *slot = k;
    return ZPK_OK;
}

extern "C" {

int zpk_codec_encode_big_device(zpk_codec* c, const uint8_t* d_src, uint64_t src_size, const zpk_encode_desc* desc, uint64_t n,
                                uint8_t* d_dst, uint64_t dst_size, zpk_encode_result* d_results, void* stream)
{
    if (!c || (n && (!desc || !d_results))) return ZPK_E_INVALID;
    CodecLock lk(c);
    c->last.enc_big[0] = c->last.enc_big[1] = 0;
    if (n == 0) return ZPK_OK;
    if (n > 0x7FFFFFFFull) return ZPK_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const u64 split_min = c->opt.enc_split_min;
    u64 np = 0, ns = 0;
    for (u64 i = 0; i < n; i++) {
        if (desc[i].src_offset > src_size || desc[i].size > src_size - desc[i].src_offset ||
            desc[i].dst_offset > dst_size || desc[i].dst_capacity > dst_size - desc[i].dst_offset) return ZPK_E_INVALID;
        if (enc_is_split(split_min, desc[i])) { np += enc_piece_count(split_min, desc[i]); ns++; }
    }
    if (np > 0x7FFFFFFFull) return ZPK_E_INVALID;
    // the tables, in the order they lie in the pinned block and (all but the spans) in c->d_desc: the call's descriptors — an entry
    // written in pieces stands there as an EMPTY STORED entry, which the one-wave launch passes over without writing a byte of its slot
    // (k_big_close writes its result later) —, the pieces, the entry table, piece -> entry, the spans to hash
    const u64 o_piece = n * sizeof(zpk_encode_desc), o_big = o_piece + np * sizeof(zpk_encode_desc), o_pe = o_big + ns * sizeof(BigEncEntry);
    const u64 up_bytes = (o_pe + np * sizeof(u32) + 7) & ~7ull, all_bytes = up_bytes + ns * sizeof(zpk_span);
    u8* h = nullptr; int slot = 0, rc;
    if ((rc = big_tables_block(c, all_bytes, &h, &slot))) return rc;
    zpk_encode_desc* const hd = (zpk_encode_desc*)h; zpk_encode_desc* const hp = (zpk_encode_desc*)(h + o_piece);
    BigEncEntry* const hb = (BigEncEntry*)(h + o_big); u32* const hpe = (u32*)(h + o_pe); zpk_span* const spans = (zpk_span*)(h + up_bytes);
    u64 k = 0, e = 0, out_total = 0, part_blocks = 0, max_cap = 0;
    for (u64 i = 0; i < n; i++) {
        hd[i] = desc[i];
        if (!enc_is_split(split_min, desc[i])) continue;
        hd[i].method = ZPK_METHOD_NONE; hd[i].size = 0; hd[i].dst_capacity = 0; hd[i].level = 0;
        BigEncEntry& B = hb[e];
        B.dst_offset = desc[i].dst_offset; B.dst_capacity = desc[i].dst_capacity;
        B.entry = (u32)i; B.first = (u32)k; B.npieces = (u32)enc_piece_count(split_min, desc[i]); B.method = desc[i].method;
        B.env = enc_envelope(desc[i].method, desc[i].size);
        const EncSpan sp = enc_emit_entry(split_min, desc[i], desc[i].src_offset, hp + k, out_total, max_cap);
        for (u32 j = 0; j < B.npieces; j++) hpe[k++] = (u32)e;
        spans[e++] = zpk_span{ sp.off, sp.len, part_blocks }; part_blocks += xxh3_span_blocks(sp.len);
    }
    const u32 spans_per_piece = (u32)((max_cap + PK_SPAN - 1) / PK_SPAN);
    const u64 gather_waves = np * spans_per_piece;
    if (gather_waves > 0x3FFFFFFFull) return ZPK_E_INVALID;
    if ((rc = grow(c, c->d_desc, up_bytes))) return rc;
    if (ns && ((rc = grow(c, c->d_dst, out_total + 64)) || (rc = grow(c, c->d_res, np * sizeof(zpk_encode_result))) ||
               (rc = grow(c, c->d_packoff, (np + 1) * sizeof(u64))))) return rc;
    u8* const dt = (u8*)c->d_desc;
    HIPCHK(c, hipMemcpyAsync(dt, h, up_bytes, hipMemcpyHostToDevice, st));
    u64* d_hash = nullptr;
    rc = xxh3_spans_enqueue(c, d_src, spans, ns, part_blocks, &d_hash, st);           // the hashes of the entries in pieces: by the whole chip, over the plaintext where it lies
    HIPCHK(c, hipEventRecord(c->bigenc.ev[slot], st));                                 // (behind the last upload out of the block, whatever rc says)
    if (rc) return rc;
    if (ns < n && (rc = encode_launch(c, d_src, (const zpk_encode_desc*)dt, n, d_dst, d_results, st))) return rc;      // the others: as zpk_codec_encode_batch_device does them
    if (ns == 0) return ZPK_OK;
    const zpk_encode_desc* const dp = (const zpk_encode_desc*)(dt + o_piece);
    const zpk_encode_result* const dr = (const zpk_encode_result*)c->d_res;
    u64* const doff = (u64*)c->d_packoff;
    if ((rc = encode_launch(c, d_src, dp, np, c->d_dst, (zpk_encode_result*)c->d_res, st)) ||
        (rc = pack_launch(c, nullptr, dp, dr, np, nullptr, 0, doff, 0, st))) return rc;
    if (c->profiling) (void)hipEventRecord(c->kev[ZPK_K_PACK][0], st);
    hipLaunchKernelGGL(k_big_gather, dim3((u32)((gather_waves + 3) / 4)), dim3(256), 0, st, (const u8*)c->d_dst, dp, dr, (u32)np, (const u64*)doff,
                       (const u32*)(dt + o_pe), (const BigEncEntry*)(dt + o_big), spans_per_piece, d_dst);
    if (c->profiling) (void)hipEventRecord(c->kev[ZPK_K_PACK][1], st);
    hipLaunchKernelGGL(k_big_close, dim3((u32)ns), dim3(64), 0, st, dr, (const u64*)doff, (const BigEncEntry*)(dt + o_big), (const u64*)d_hash, d_dst, d_results);
    HIPCHK(c, hipGetLastError());
    c->last.enc_big[0] = (u32)ns; c->last.enc_big[1] = (u32)np;
    return ZPK_OK;
}

int zpk_codec_encode_stats(zpk_codec* c, uint32_t out[8])
{
    if (!c || !out) return ZPK_E_INVALID;
    CodecLock lk(c);
    memset(out, 0, 8 * sizeof(uint32_t));
    out[0] = c->last.enc_big[0]; out[1] = c->last.enc_big[1];
    return ZPK_OK;
}

}  // extern "C"
