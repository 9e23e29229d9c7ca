// k_span_hash: XXH3-64 (seed 0, the reference's XXH3_64bits) of any number of spans of device memory in one launch, one wave per row —
// k_stored_hash (stored_hash.h) without an archive around it: a row is a device address and a length, at any alignment, and the hash goes
// to out[row].  The same block loop — each 1 KiB block loaded once, the next one in flight while it is folded — and the same short
// path.  Rows long enough to be worth the whole chip do not come here: the partial sums and the chain of xxh3_span.h take them, with the
// source pointer null and the row's address as the span's offset.  Which rows go where, the tables and the launches: span_hash_plan.h.
// Nothing outside [addr, addr + len) is read (span_hash_loads states the ranges), nothing but out[row] is written.  No LDS beyond what
// Xxh3Wave uses, no scratch.
#pragma once
#include "zpk_device.h"
#include "xxh3_device.h"
#include "xxh3_span.h"
#include "span_hash_plan.h"

namespace zpk {

static_assert(ZPK_SPAN_GROUP == XS_GROUP, "span_hash_plan.h lays the partial sums out in the groups of xxh3_span.h");
static_assert(sizeof(SpanHashWide) == sizeof(zpk_span) && offsetof(SpanHashWide, off) == offsetof(zpk_span, off) &&
              offsetof(SpanHashWide, len) == offsetof(zpk_span, len) && offsetof(SpanHashWide, part_base) == offsetof(zpk_span, part_base),
              "a chip-wide row is the zpk_span k_xxh3_partials and k_xxh3_chain read");

// Rows [first, end) of the table, four per workgroup: wave w of the launch takes row first + w.
__global__ __launch_bounds__(256) void k_span_hash(const SpanHashRow* __restrict__ rows, u64 first, u64 end, u64* __restrict__ out)
{
    const int lane = lane_id();
    const u64 w = uni64(first + (u64)blockIdx.x * 4 + (threadIdx.x >> 6));
    if (w >= end) return;
    const SpanHashRow r = rows[w];
    const u8* in = uni_ptr((const u8*)r.addr);
    const u64 len = uni64(r.len);
    u64 h;
    if (len <= 240) {
        h = 0;
        lane0_guard();
        if (lane == 0) h = xxh3_short(in, (u32)len);
        h = uni64(h);
    } else {
        Xxh3Wave st; st.init(lane);
        const u64 nblocks = (len - 1) >> 10;
        const u8* q = in + 16 * lane;
        u128 cur = {0, 0};
        if (nblocks) cur = ld128(q);
        for (u64 b = 0; b < nblocks; b++) {
            u128 nxt = {0, 0};
            if (b + 1 < nblocks) nxt = ld128(q + ((b + 1) << 10));
            st.block(cur);
            cur = nxt;
        }
        const u64 done = nblocks << 10;
        const u32 nstripes = (u32)(((len - 1) - done) >> 6);
        h = st.finish(in + done, nstripes, in + len, len, lane);
    }
    lane0_guard();
    if (lane == 0) out[w] = h;
}

}  // namespace zpk
