// xxh3_device.h — XXH3-64 (seed 0, default secret) as a wave64 primitive for gfx950, plus serial
// XXH32 / XXH64 for the frame-internal checksums of foreign LZ4F / Zstandard frames.
//
// Replaces XXH3_64bits of the reference (lib/zpack_read.c:466, lib/zpack_write.c:256).
//
// Long inputs (> 240 B): the 8 u64 accumulators are spread over the wave, pair q = (l & 3) in every lane.
//   * Xxh3Wave::block() / Xxh3Lite::block(): one 1 KiB block whose bytes are already in registers, lane l = 16-byte slot l = stripe
//     (l >> 2).  The 16 stripe contributions to one accumulator only ADD: a 16-lane reduction per block (ds_bpermute, or DPP row
//     rotations + v_permlane16/32_swap), then the scramble redundantly in every lane.  For kernels that hash what they copy or flush
//     (k_stored, the Zstandard ring, the streams).
//   * xxh3_64_wave(): a pass over memory, FOUR blocks per step, one DPP row of 16 lanes per block.  A lane sums the four stripes it
//     takes of its block in its own registers, two DPP rotations finish the block sum inside the row, and only the chain
//     acc = scramble(acc + S_b) crosses rows: 4 dwords per block instead of a reduction (117 against 213 vector instructions and 16
//     against 64 ds_bpermute per 4 KiB in k_lz4_wave).
#pragma once
#include "zpk_device.h"

namespace zpk {

#define ZPK_P32_1 0x9E3779B1U
#define ZPK_P32_2 0x85EBCA77U
#define ZPK_P32_3 0xC2B2AE3DU
#define ZPK_P32_4 0x27D4EB2FU
#define ZPK_P32_5 0x165667B1U
#define ZPK_P64_1 0x9E3779B185EBCA87ULL
#define ZPK_P64_2 0xC2B2AE3D27D4EB4FULL
#define ZPK_P64_3 0x165667B19E3779F9ULL
#define ZPK_P64_4 0x85EBCA77C2B2AE63ULL
#define ZPK_P64_5 0x27D4EB2F165667C5ULL
#define ZPK_PMX_1 0x165667919E3779F9ULL
#define ZPK_PMX_2 0x9FB21C651E98DF25ULL

// default XXH3 secret (xxHash specification, "kSecret"), padded to a multiple of 8
__device__ __constant__ const u8 XXH3_SECRET[192] = {
    0xb8, 0xfe, 0x6c, 0x39, 0x23, 0xa4, 0x4b, 0xbe, 0x7c, 0x01, 0x81, 0x2c, 0xf7, 0x21, 0xad, 0x1c,
    0xde, 0xd4, 0x6d, 0xe9, 0x83, 0x90, 0x97, 0xdb, 0x72, 0x40, 0xa4, 0xa4, 0xb7, 0xb3, 0x67, 0x1f,
    0xcb, 0x79, 0xe6, 0x4e, 0xcc, 0xc0, 0xe5, 0x78, 0x82, 0x5a, 0xd0, 0x7d, 0xcc, 0xff, 0x72, 0x21,
    0xb8, 0x08, 0x46, 0x74, 0xf7, 0x43, 0x24, 0x8e, 0xe0, 0x35, 0x90, 0xe6, 0x81, 0x3a, 0x26, 0x4c,
    0x3c, 0x28, 0x52, 0xbb, 0x91, 0xc3, 0x00, 0xcb, 0x88, 0xd0, 0x65, 0x8b, 0x1b, 0x53, 0x2e, 0xa3,
    0x71, 0x64, 0x48, 0x97, 0xa2, 0x0d, 0xf9, 0x4e, 0x38, 0x19, 0xef, 0x46, 0xa9, 0xde, 0xac, 0xd8,
    0xa8, 0xfa, 0x76, 0x3f, 0xe3, 0x9c, 0x34, 0x3f, 0xf9, 0xdc, 0xbb, 0xc7, 0xc7, 0x0b, 0x4f, 0x1d,
    0x8a, 0x51, 0xe0, 0x4b, 0xcd, 0xb4, 0x59, 0x31, 0xc8, 0x9f, 0x7e, 0xc9, 0xd9, 0x78, 0x73, 0x64,
    0xea, 0xc5, 0xac, 0x83, 0x34, 0xd3, 0xeb, 0xc3, 0xc5, 0x81, 0xa0, 0xff, 0xfa, 0x13, 0x63, 0xeb,
    0x17, 0x0d, 0xdd, 0x51, 0xb7, 0xf0, 0xda, 0x49, 0xd3, 0x16, 0x55, 0x26, 0x29, 0xd4, 0x68, 0x9e,
    0x2b, 0x16, 0xbe, 0x58, 0x7d, 0x47, 0xa1, 0xfc, 0x8f, 0xf8, 0xb8, 0xd1, 0x7a, 0xd0, 0x31, 0xce,
    0x45, 0xcb, 0x3a, 0x8f, 0x95, 0x16, 0x04, 0x28, 0xaf, 0xd7, 0xfb, 0xca, 0xbb, 0x4b, 0x40, 0x7e,
};

__device__ __forceinline__ u64 sec64(int off) { return ld64(XXH3_SECRET + off); }
__device__ __forceinline__ u32 sec32(int off) { return ld32(XXH3_SECRET + off); }

__device__ __forceinline__ u64 mul128_fold64(u64 a, u64 b) { return (a * b) ^ __umul64hi(a, b); }
__device__ __forceinline__ u64 xxh64_avalanche(u64 h)
{
    h ^= h >> 33; h *= ZPK_P64_2; h ^= h >> 29; h *= ZPK_P64_3; h ^= h >> 32; return h;
}
__device__ __forceinline__ u64 xxh3_avalanche(u64 h) { h ^= h >> 37; h *= ZPK_PMX_1; h ^= h >> 32; return h; }
__device__ __forceinline__ u64 bswap64(u64 x) { return __builtin_bswap64(x); }

__device__ __forceinline__ u64 xxh3_mix16(const u8* in, int soff)
{
    return mul128_fold64(ld64(in) ^ sec64(soff), ld64(in + 8) ^ sec64(soff + 8));
}

// 0..240 bytes, serial (executed by whichever lanes call it; callers use one lane or the whole wave
// redundantly — every load is in bounds of [in, in+len))
__device__ inline u64 xxh3_short(const u8* in, u32 len)
{
    if (len == 0) return xxh64_avalanche(sec64(56) ^ sec64(64));
    if (len <= 3) {
        u32 c1 = ld8(in), c2 = ld8(in + (len >> 1)), c3 = ld8(in + len - 1);
        u32 combined = (c1 << 16) | (c2 << 24) | c3 | (len << 8);
        u64 flip = (u64)(sec32(0) ^ sec32(4));
        return xxh64_avalanche((u64)combined ^ flip);
    }
    if (len <= 8) {
        u32 a = ld32(in), b = ld32(in + len - 4);
        u64 flip = sec64(8) ^ sec64(16);
        u64 in64 = (u64)b + ((u64)a << 32);
        u64 h = in64 ^ flip;
        h ^= rotl64(h, 49) ^ rotl64(h, 24);
        h *= ZPK_PMX_2;
        h ^= (h >> 35) + len;
        h *= ZPK_PMX_2;
        return h ^ (h >> 28);
    }
    if (len <= 16) {
        u64 lo = ld64(in) ^ (sec64(24) ^ sec64(32));
        u64 hi = ld64(in + len - 8) ^ (sec64(40) ^ sec64(48));
        u64 acc = len + bswap64(lo) + hi + mul128_fold64(lo, hi);
        return xxh3_avalanche(acc);
    }
    if (len <= 128) {
        u64 acc = (u64)len * ZPK_P64_1;
        if (len > 32) {
            if (len > 64) {
                if (len > 96) {
                    acc += xxh3_mix16(in + 48, 96);
                    acc += xxh3_mix16(in + len - 64, 112);
                }
                acc += xxh3_mix16(in + 32, 64);
                acc += xxh3_mix16(in + len - 48, 80);
            }
            acc += xxh3_mix16(in + 16, 32);
            acc += xxh3_mix16(in + len - 32, 48);
        }
        acc += xxh3_mix16(in, 0);
        acc += xxh3_mix16(in + len - 16, 16);
        return xxh3_avalanche(acc);
    }
    u64 acc = (u64)len * ZPK_P64_1;
    u32 rounds = len / 16;
    for (u32 i = 0; i < 8; i++) acc += xxh3_mix16(in + 16 * i, 16 * (int)i);
    acc = xxh3_avalanche(acc);
    for (u32 i = 8; i < rounds; i++) acc += xxh3_mix16(in + 16 * i, 16 * (int)(i - 8) + 3);
    acc += xxh3_mix16(in + len - 16, 136 - 17);
    return xxh3_avalanche(acc);
}

// ---- wave-parallel long hash -------------------------------------------------------------------

struct Xxh3Wave {
    u64 a0, a1;        // acc[2q], acc[2q+1], q = lane & 3 (identical in the 16 lanes sharing q)
    u64 k0, k1;        // secret words of this lane's slot in a full block: secret[8*(l>>2) + 16q (+8)]
    u64 s0, s1;        // scramble keys secret[128 + 16q (+8)]

    // accumulators and scramble keys only: the four-block loop of xxh3_64_wave has keys of its own and loads k0 / k1 behind it
    __device__ __forceinline__ void init_acc(int lane)
    {
        const int q = lane & 3;
        const u64 init[8] = { ZPK_P32_3, ZPK_P64_1, ZPK_P64_2, ZPK_P64_3, ZPK_P64_4, ZPK_P32_2, ZPK_P64_5, ZPK_P32_1 };
        a0 = q == 0 ? init[0] : q == 1 ? init[2] : q == 2 ? init[4] : init[6];
        a1 = q == 0 ? init[1] : q == 1 ? init[3] : q == 2 ? init[5] : init[7];
        s0 = sec64(128 + 16 * q);   s1 = sec64(128 + 16 * q + 8);
    }
    __device__ __forceinline__ void init_keys(int lane)
    {
        const int q = lane & 3, s = lane >> 2;
        k0 = sec64(8 * s + 16 * q); k1 = sec64(8 * s + 16 * q + 8);
    }
    __device__ __forceinline__ void init(int lane) { init_acc(lane); init_keys(lane); }

    // contribution of one 16-byte slot (d0 = u64 index 2q of its stripe, d1 = index 2q+1)
    static __device__ __forceinline__ void slot(u64 d0, u64 d1, u64 key0, u64 key1, u64& c0, u64& c1)
    {
        u64 x0 = d0 ^ key0, x1 = d1 ^ key1;
        c0 = (u64)(u32)x0 * (u64)(u32)(x0 >> 32) + d1;      // acc[2q]   += product(2q)   + data(2q+1)
        c1 = (u64)(u32)x1 * (u64)(u32)(x1 >> 32) + d0;      // acc[2q+1] += product(2q+1) + data(2q)
    }

    // Sum over the 16 lanes that share q = lane & 3 (lanes q, q + 4, ... q + 60), result in all of them.  No LDS: inside a DPP row
    // two rotations (row_ror:4, row_ror:8) add up the four lanes q + 4i; across the four rows v_permlane16_swap / v_permlane32_swap
    // (gfx950) exchange whole rows / halves between a value and its copy, so that value + copy is the sum of the pair.  (Round 2 did
    // this with 16 ds_bpermute per 1 KiB block: ~100 LDS cycles per block on a CU whose LDS pipe the decoders keep 80 % busy.)
    // Two dwords as one 64-bit value the compiler cannot take apart again.  Left to itself it turns a + ((hi << 32) | lo) into
    // a + lo + (hi << 32): two 64-bit additions and a zeroed register where one addition does (seen in the four-block loop: 8 + 16
    // extra vector instructions per step).  The empty asm costs nothing and only hides where the halves came from.
    static __device__ __forceinline__ u64 pair64(u32 lo, u32 hi)
    {
        u64 v = ((u64)hi << 32) | lo;
        asm volatile("" : "+v"(v));
        return v;
    }
    // c + (c rotated inside its DPP row).  LEAN (the four-block loop): every lane of the row is read, so bound_ctrl spares the
    // zeroed `old` register of each v_mov_dpp, and the rotated value is pinned (pair64).  The Zstandard flush keeps the form it
    // was measured with.
    template <int CTRL, bool LEAN = false>
    static __device__ __forceinline__ u64 add_rotated(u64 c)
    {
        const u32 rl = (u32)__builtin_amdgcn_update_dpp(0, (int)(u32)c, CTRL, 0xf, 0xf, LEAN);
        const u32 rh = (u32)__builtin_amdgcn_update_dpp(0, (int)(u32)(c >> 32), CTRL, 0xf, 0xf, LEAN);
        return c + (LEAN ? pair64(rl, rh) : (((u64)rh << 32) | rl));
    }
    static __device__ __forceinline__ u64 add_rows(u64 c)
    {
        const u32 lo = (u32)c, hi = (u32)(c >> 32);
        auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        const u64 s = (((u64)h16[0] << 32) | l16[0]) + (((u64)h16[1] << 32) | l16[1]);        // rows {0,1} and {2,3} summed pairwise
        const u32 slo = (u32)s, shi = (u32)(s >> 32);
        auto l32 = __builtin_amdgcn_permlane32_swap(slo, slo, false, false);
        auto h32 = __builtin_amdgcn_permlane32_swap(shi, shi, false, false);
        return (((u64)h32[0] << 32) | l32[0]) + (((u64)h32[1] << 32) | l32[1]);
    }
    // Which form is faster depends on what the kernel around it is short of (measured, round 3): k_lz4_wave is bound by vector
    // issue with LDS cycles to spare — there the 16 ds_bpermute are the cheaper ones (508 vs 498 GiB/s on text); the Zstandard execute
    // stage is short of LDS cycles and gains with the DPP / permlane form (13.1 -> 12.7 ms on C3).
    template <bool NO_LDS>
    static __device__ __forceinline__ void reduce16(u64& c0, u64& c1)
    {
        if (!NO_LDS) {
            #pragma unroll
            for (int m = 4; m < 64; m <<= 1) { c0 += shfl_xor64(c0, m); c1 += shfl_xor64(c1, m); }
        } else {
            c0 = add_rotated<0x124>(c0); c1 = add_rotated<0x124>(c1);         // row_ror:4
            c0 = add_rotated<0x128>(c0); c1 = add_rotated<0x128>(c1);         // row_ror:8
            c0 = add_rows(c0); c1 = add_rows(c1);
        }
    }

    __device__ __forceinline__ void scramble()
    {
        a0 = ((a0 ^ (a0 >> 47)) ^ s0) * ZPK_P32_1;
        a1 = ((a1 ^ (a1 >> 47)) ^ s1) * ZPK_P32_1;
    }

    // one full 1 KiB block whose 16 bytes for this lane are already in registers
    __device__ __forceinline__ void block(u128 d)
    {
        u64 c0, c1;
        slot(d.lo, d.hi, k0, k1, c0, c1);
        reduce16<false>(c0, c1);
        a0 += c0; a1 += c1;
        scramble();
    }

    // ---- four blocks per step (xxh3_64_wave) -----------------------------------------------------------------------------------------
    // lane = 16 r + 4 sub + q: DPP row r owns block 4 g + r of group g, q is the slot as above, and in iteration it = 0..3 the lane
    // takes stripe 4 it + sub of its block.  A lane sums its four contributions in its own registers; the 16 stripes of a block are
    // then the four lanes of one row that share q (row_sum: two DPP rotations, no LDS, no step across rows).  The block sums do not
    // depend on the accumulators: only acc = scramble(acc + S_b) is a chain, and it takes the four sums in block order, each
    // broadcast from its row to the wave (4 dwords per block, against the 16-lane reduction per block of block(): 16 ds_bpermute).
    static __device__ __forceinline__ void quad_keys(int lane, int it, u64& key0, u64& key1)
    {
        const int off = 32 * it + 8 * ((lane >> 2) & 3) + 16 * (lane & 3);        // secret[8 s + 16 q], s = 4 it + sub
        key0 = sec64(off); key1 = sec64(off + 8);
    }
    // ... from a copy of the secret in LDS (stage_secret): one 8-byte-aligned 16-byte read, nothing kept in registers
    static __device__ __forceinline__ void quad_keys(lds_cp8 sec, int lane, int it, u64& key0, u64& key1)
    {
        const ZPK_LDS u64* w = (const ZPK_LDS u64*)(sec + 8 * ((lane >> 2) & 3) + 16 * (lane & 3)) + 4 * it;
        key0 = w[0]; key1 = w[1];
    }
    // the 192-byte secret into LDS at `sec` (16-byte aligned); the wave's earlier LDS traffic there is over (in order per wave)
    static __device__ __forceinline__ void stage_secret(lds_p8 sec, int lane)
    {
        wave_mem_fence();
        if (lane < 12) lds_st128(sec + 16 * lane, ld128(XXH3_SECRET + 16 * lane));
        wave_mem_fence();
    }
    static __device__ __forceinline__ void quad_slot(u128 d, u64 key0, u64 key1, u64& t0, u64& t1)
    {
        u64 c0, c1;
        slot(d.lo, d.hi, key0, key1, c0, c1);
        t0 += c0; t1 += c1;
    }
    static __device__ __forceinline__ void row_sum(u64& t0, u64& t1)
    {
        t0 = add_rotated<0x124, true>(t0); t1 = add_rotated<0x124, true>(t1);   // row_ror:4
        t0 = add_rotated<0x128, true>(t0); t1 = add_rotated<0x128, true>(t1);   // row_ror:8
    }
    // row R of v in every row: one ds_bpermute per dword, the row picked by the instruction's offset field.  (A form without LDS,
    // three v_permlane32/16_swap per dword for all four rows, compiles to 141 against 117 vector instructions per step and was never
    // run on a GPU: profiles/r09/.)
    template <int R>
    static __device__ __forceinline__ u64 row_bcast_lds(u64 v, int l15x4)
    {
        const u32 lo = (u32)__builtin_amdgcn_ds_bpermute(l15x4 + 64 * R, (int)(u32)v);
        const u32 hi = (u32)__builtin_amdgcn_ds_bpermute(l15x4 + 64 * R, (int)(u32)(v >> 32));
        return pair64(lo, hi);
    }
    __device__ __forceinline__ void fold(u64 S0, u64 S1) { a0 += S0; a1 += S1; scramble(); }
    // the block sums t0 / t1 of up to four blocks (row r = block r of the group; `n` = 1..4 of them exist, uniform) into the chain
    __device__ __forceinline__ void fold_rows(u64 t0, u64 t1, u32 n, int lane)
    {
        const int l15x4 = 4 * (lane & 15);
        fold(row_bcast_lds<0>(t0, l15x4), row_bcast_lds<0>(t1, l15x4));
        if (n > 1) fold(row_bcast_lds<1>(t0, l15x4), row_bcast_lds<1>(t1, l15x4));
        if (n > 2) fold(row_bcast_lds<2>(t0, l15x4), row_bcast_lds<2>(t1, l15x4));
        if (n > 3) fold(row_bcast_lds<3>(t0, l15x4), row_bcast_lds<3>(t1, l15x4));
    }

    // tail: `nstripes` (0..15) whole stripes at `p`, then the last stripe [end-64, end).
    // Lane group 15 is never used by a partial block, so it carries the last stripe.
    __device__ __forceinline__ u64 finish(const u8* p, u32 nstripes, const u8* end, u64 total_len, int lane)
    {
        const int q = lane & 3, s = lane >> 2;
        u64 c0 = 0, c1 = 0;
        if ((u32)s < nstripes) {
            u128 d = ld128(p + 16 * lane);
            slot(d.lo, d.hi, k0, k1, c0, c1);
        } else if (s == 15) {
            u128 d = ld128(end - 64 + 16 * q);
            slot(d.lo, d.hi, sec64(121 + 16 * q), sec64(121 + 16 * q + 8), c0, c1);
        }
        reduce16<false>(c0, c1);
        a0 += c0; a1 += c1;
        u64 t = mul128_fold64(a0 ^ sec64(11 + 16 * q), a1 ^ sec64(11 + 16 * q + 8));
        t += shfl_xor64(t, 1);
        t += shfl_xor64(t, 2);
        return xxh3_avalanche(total_len * ZPK_P64_1 + t);
    }
};

// The same state in 4 registers instead of 12: the per-lane secret words are re-read from the constant table for every block (for
// kernels whose occupancy is worth more than four cached loads per KiB)
struct Xxh3Lite {
    u64 a0, a1;
    __device__ __forceinline__ void init(int lane)
    {
        Xxh3Wave w; w.init(lane); a0 = w.a0; a1 = w.a1;
    }
    // `sec` = a copy of the 192-byte secret in LDS, or null (constant memory).  The constant-memory reads are vector loads: their
    // s_waitcnt vmcnt(0) also waits for the 1 KiB flush store issued just before — a full store round trip per flushed block.
    __device__ __forceinline__ void block(u128 d, int lane, lds_cp8 sec = nullptr)
    {
        const int q = lane & 3, s = lane >> 2;
        u64 k0, k1, s0, s1;
        if (sec) {
            k0 = ((const ZPK_LDS u64*)(sec + 8 * s + 16 * q))[0]; k1 = ((const ZPK_LDS u64*)(sec + 8 * s + 16 * q))[1];
            s0 = ((const ZPK_LDS u64*)(sec + 128 + 16 * q))[0];   s1 = ((const ZPK_LDS u64*)(sec + 128 + 16 * q))[1];
        } else { k0 = sec64(8 * s + 16 * q); k1 = sec64(8 * s + 16 * q + 8); s0 = sec64(128 + 16 * q); s1 = sec64(128 + 16 * q + 8); }
        u64 c0, c1;
        Xxh3Wave::slot(d.lo, d.hi, k0, k1, c0, c1);
        Xxh3Wave::reduce16<true>(c0, c1);
        a0 += c0; a1 += c1;
        a0 = ((a0 ^ (a0 >> 47)) ^ s0) * ZPK_P32_1;
        a1 = ((a1 ^ (a1 >> 47)) ^ s1) * ZPK_P32_1;
    }
    __device__ __forceinline__ u64 finish(const u8* p, u32 nstripes, const u8* end, u64 total_len, int lane)
    {
        Xxh3Wave w; w.init(lane); w.a0 = a0; w.a1 = a1;
        return w.finish(p, nstripes, end, total_len, lane);
    }
};

// XXH3_64bits(p, len) computed by one full wave (all 64 lanes must call; result uniform).
// `p` may have any alignment.
// LDS_KEYS: the per-lane secret words of the four-block loop are read from a copy of the secret in LDS (`sec`: 192 bytes the
// caller owns, written here) instead of being kept in 16 registers — for kernels built for 64 VGPRs (k_lz4_wave and its kin).
template <bool LDS_KEYS = false>
__device__ __forceinline__ u64 xxh3_64_wave(const u8* p, u64 len, int lane, lds_p8 sec = nullptr)
{
    if (len <= 240) {
        u64 h = 0;
        lane0_guard();
        if (lane == 0) h = xxh3_short(p, (u32)len);
        return uni64(h);
    }
    Xxh3Wave st;
    st.init_acc(lane);
    const u64 nblocks = uni64((len - 1) >> 10);
    // Four blocks per step (Xxh3Wave, "four blocks per step"): row r = lane >> 4 reads block 4 g + r, 256 contiguous bytes per row
    // and load.  Software prefetch in two halves: while iterations 0, 1 are multiplied the loads of 2, 3 are in flight, and the next
    // group's 0, 1 while 2, 3 are multiplied and the group is reduced and folded.  The loads are UNCONDITIONAL (past the end they
    // re-read the last block) and no loaded register is ever moved: the compiler counts outstanding
    // loads exactly only then (s_waitcnt vmcnt(2)); with a guarded load or a register rotation it waits for everything, i.e. for
    // the loads it has just issued — a full memory round trip per half, which is what this loop once cost (18 % of k_lz4_wave).
    if (nblocks > 0) {
        const u64 lastg = (nblocks - 1) >> 2;                         // the last group: 1..4 blocks
        const u32 nlast = (((u32)nblocks - 1u) & 3u) + 1u;
        const u32 row = (u32)lane >> 4, l16 = 16u * ((u32)lane & 15u);
        u64 kc[4][2] = {};
        if (LDS_KEYS) Xxh3Wave::stage_secret(sec, lane);
        else { Xxh3Wave::quad_keys(lane, 0, kc[0][0], kc[0][1]); Xxh3Wave::quad_keys(lane, 1, kc[1][0], kc[1][1]);
               Xxh3Wave::quad_keys(lane, 2, kc[2][0], kc[2][1]); Xxh3Wave::quad_keys(lane, 3, kc[3][0], kc[3][1]); }
        #define XXH3_SLOT(d, it) do { u64 k0_ = kc[it][0], k1_ = kc[it][1]; if (LDS_KEYS) Xxh3Wave::quad_keys((lds_cp8)sec, lane, it, k0_, k1_); \
                                      Xxh3Wave::quad_slot(d, k0_, k1_, t0, t1); } while (0)
        // byte offset of the lane's row in a full group / in the last one (rows past its last block re-read that block: their sums
        // stay in their rows and are never folded)
        const u32 off_full = (row << 10) + l16, off_last = ((row < nlast ? row : nlast - 1u) << 10) + l16;
        #define XXH3_LD(g, it) ld128(p + ((g) << 12) + ((g) == lastg ? off_last : off_full) + 256u * (it))
        u128 a0 = XXH3_LD((u64)0, 0), a1 = XXH3_LD((u64)0, 1);
        #pragma clang loop unroll(disable)                            // (no peeled last step either: its hand-over moves the loaded registers)
        for (u64 g = 0; g <= lastg; g++) {
            const u128 c0 = XXH3_LD(g, 2), c1 = XXH3_LD(g, 3);
            __builtin_amdgcn_sched_barrier(0);                        // (the machine scheduler would issue all four loads up here)
            u64 t0 = 0, t1 = 0;
            XXH3_SLOT(a0, 0);
            XXH3_SLOT(a1, 1);
            const u64 gn = g < lastg ? g + 1 : lastg;                 // past the end: the last group again
            asm volatile("" : "+v"(t0), "+v"(t1));                    // (the sums so far are finished here: a0 / a1 are dead, not copied)
            __builtin_amdgcn_sched_barrier(0);
            a0 = XXH3_LD(gn, 0); a1 = XXH3_LD(gn, 1);
            __builtin_amdgcn_sched_barrier(0);
            XXH3_SLOT(c0, 2);
            XXH3_SLOT(c1, 3);
            Xxh3Wave::row_sum(t0, t1);
            st.fold_rows(t0, t1, g == lastg ? nlast : 4u, lane);
        }
        #undef XXH3_LD
        #undef XXH3_SLOT
    }
    st.init_keys(lane);
    const u32 nstripes = (u32)(((len - 1) - (nblocks << 10)) >> 6);
    return st.finish(p + (nblocks << 10), nstripes, p + len, len, lane);
}

// ---- serial XXH32 / XXH64 (foreign-frame checksums; single lane) --------------------------------

__device__ inline u32 xxh32_serial(const u8* p, u64 len, u32 seed)
{
    const u8* end = p + len;
    u32 h;
    if (len >= 16) {
        u32 v1 = seed + ZPK_P32_1 + ZPK_P32_2, v2 = seed + ZPK_P32_2, v3 = seed, v4 = seed - ZPK_P32_1;
        do {
            v1 = rotl32(v1 + ld32(p) * ZPK_P32_2, 13) * ZPK_P32_1;
            v2 = rotl32(v2 + ld32(p + 4) * ZPK_P32_2, 13) * ZPK_P32_1;
            v3 = rotl32(v3 + ld32(p + 8) * ZPK_P32_2, 13) * ZPK_P32_1;
            v4 = rotl32(v4 + ld32(p + 12) * ZPK_P32_2, 13) * ZPK_P32_1;
            p += 16;
        } while (p + 16 <= end);
        h = rotl32(v1, 1) + rotl32(v2, 7) + rotl32(v3, 12) + rotl32(v4, 18);
    } else {
        h = seed + ZPK_P32_5;
    }
    h += (u32)len;
    while (p + 4 <= end) { h = rotl32(h + ld32(p) * ZPK_P32_3, 17) * ZPK_P32_4; p += 4; }
    while (p < end) { h = rotl32(h + (u32)ld8(p) * ZPK_P32_5, 11) * ZPK_P32_1; p++; }
    h ^= h >> 15; h *= ZPK_P32_2; h ^= h >> 13; h *= ZPK_P32_3; h ^= h >> 16;
    return h;
}

__device__ __forceinline__ u64 xxh64_round(u64 acc, u64 in) { return rotl64(acc + in * ZPK_P64_2, 31) * ZPK_P64_1; }

__device__ inline u64 xxh64_serial(const u8* p, u64 len, u64 seed)
{
    const u8* end = p + len;
    u64 h;
    if (len >= 32) {
        u64 v1 = seed + ZPK_P64_1 + ZPK_P64_2, v2 = seed + ZPK_P64_2, v3 = seed, v4 = seed - ZPK_P64_1;
        do {
            v1 = xxh64_round(v1, ld64(p)); v2 = xxh64_round(v2, ld64(p + 8));
            v3 = xxh64_round(v3, ld64(p + 16)); v4 = xxh64_round(v4, ld64(p + 24));
            p += 32;
        } while (p + 32 <= end);
        h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
        h = (h ^ xxh64_round(0, v1)) * ZPK_P64_1 + ZPK_P64_4;
        h = (h ^ xxh64_round(0, v2)) * ZPK_P64_1 + ZPK_P64_4;
        h = (h ^ xxh64_round(0, v3)) * ZPK_P64_1 + ZPK_P64_4;
        h = (h ^ xxh64_round(0, v4)) * ZPK_P64_1 + ZPK_P64_4;
    } else {
        h = seed + ZPK_P64_5;
    }
    h += len;
    while (p + 8 <= end) { h ^= xxh64_round(0, ld64(p)); h = rotl64(h, 27) * ZPK_P64_1 + ZPK_P64_4; p += 8; }
    if (p + 4 <= end) { h ^= (u64)ld32(p) * ZPK_P64_1; h = rotl64(h, 23) * ZPK_P64_2 + ZPK_P64_3; p += 4; }
    while (p < end) { h ^= (u64)ld8(p) * ZPK_P64_5; h = rotl64(h, 11) * ZPK_P64_1; p++; }
    return xxh64_avalanche(h);
}

}  // namespace zpk
