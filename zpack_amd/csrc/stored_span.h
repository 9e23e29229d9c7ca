// Large STORED entries of a device-resident batch, copied and hashed by the whole chip (round 17): k_stored gives an entry one wave —
// 1.05 / 1.36 GiB/s for one large entry, a fifth of a second for 256 MiB — while the chip copies at TB/s when the entries are many.
// k_stored_span is k_xxh3_partials (xxh3_span.h) with the copy fused in: every 1 KiB block is loaded once, stored to the entry's slot and
// folded into its partial sum; k_xxh3_chain then runs on the sums unchanged.  Which entries come here and the span table: stored_plan.h.
#pragma once
#include "zpk_device.h"
#include "xxh3_device.h"
#include "xxh3_span.h"
#include "stored_plan.h"

namespace zpk {

static_assert(ZPK_SPAN_GROUP == XS_GROUP, "stored_plan.h lays the partial sums out in the groups of xxh3_span.h");
static_assert(sizeof(StoredSpanRow) == sizeof(zpk_span) && offsetof(StoredSpanRow, off) == offsetof(zpk_span, off) &&
              offsetof(StoredSpanRow, len) == offsetof(zpk_span, len) && offsetof(StoredSpanRow, part_base) == offsetof(zpk_span, part_base),
              "a row of the span table is the zpk_span k_xxh3_chain reads");

// One wave per group of 64 blocks of one span, four waves per workgroup, any number of spans in one launch.  Source and destination may
// have any alignment, independent of each other (16-byte global accesses at any address, as everywhere here).  Nothing outside
// [off, off + len) of the source is read and nothing outside [dst_off, dst_off + len) is written: the 16-byte accesses end with the last
// FULL block, the tail [nblocks << 10, len) — 1..1024 bytes, the block the chain hashes from the source — is copied byte by byte by the
// wave of the span's last group, behind its blocks.  The sums go out [accumulator][block] per group, as k_xxh3_partials writes them.
__global__ __launch_bounds__(256) void k_stored_span(const u8* __restrict__ src, u8* __restrict__ dst, const zpk_span* __restrict__ spans,
                                                     const u64* __restrict__ dst_off, u32 nspans, u64 ngroups, u64* __restrict__ partial)
{
    const int lane = lane_id();
    const u64 g = uni64((u64)blockIdx.x * 4 + (threadIdx.x >> 6));
    if (g >= ngroups) return;
    u32 lo = 0, hi = nspans;                                                          // last span with part_base / 64 <= g
    while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (spans[mid].part_base / XS_GROUP <= g) lo = mid; else hi = mid; }
    const zpk_span sp = spans[lo];
    const u64 len = uni64(sp.len), nblocks = (len - 1) >> 10;                         // the block with the last byte belongs to the chain
    const u64 b0 = (g - sp.part_base / XS_GROUP) * XS_GROUP;
    if (b0 >= nblocks) return;
    const u32 nb = (u32)(nblocks - b0 < XS_GROUP ? nblocks - b0 : XS_GROUP);
    Xxh3Wave w; w.init(lane);
    const u8* const in = uni_ptr(src + sp.off);
    u8* const to = uni_ptr(dst + dst_off[lo]);
    const u8* q = in + (b0 << 10) + 16 * lane;
    u8* o = to + (b0 << 10) + 16 * lane;
    u64* out = partial + (sp.part_base + b0) * 8 + 128 * (lane & 3);                  // a group's sums lie [accumulator][block] (k_xxh3_partials)
    for (u32 j = 0; j < nb; j += 4) {                                                 // four blocks' loads in flight (unconditional: past the end the last block again)
        u128 d[4];
        #pragma unroll
        for (u32 t = 0; t < 4; t++) d[t] = ld128(q + ((u64)(j + t < nb ? j + t : nb - 1) << 10));
        #pragma unroll
        for (u32 t = 0; t < 4; t++) {
            if (j + t < nb) st128(o + ((u64)(j + t) << 10), d[t]);
            u64 c0, c1;
            Xxh3Wave::slot(d[t].lo, d[t].hi, w.k0, w.k1, c0, c1);
            Xxh3Wave::reduce16<true>(c0, c1);
            if (lane < 4 && j + t < nb) { out[j + t] = c0; out[64 + j + t] = c1; }
        }
    }
    if (b0 + nb == nblocks)                                                           // the span's last group: the tail, 1..1024 bytes
        for (u64 i = (nblocks << 10) + lane; i < len; i += WAVE) st8(to + i, ld8(in + i));
}

}  // namespace zpk
