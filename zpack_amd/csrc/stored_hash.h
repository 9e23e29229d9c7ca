// k_stored_hash: the stored entries (method 0) of a batch that is only TESTED (zpk_codec_verify_batch_host / _dimage: no destination) —
// k_stored (zpk_codec.hip) without the copy.  The payload is hashed where it lies, the staged source or the archive image in device
// memory, at any alignment; the entry has no output slot, dst_offset and dst_capacity of its descriptor are not looked at.  The same
// work list (S_NONE / counters[C_NONE], one wave per slot), the same block loop — each 1 KiB block loaded once, the next one in flight
// while it is folded into the XXH3 — the same short path, the same result record, ZPK_DF_SKIP_HASH honoured.
// Nothing outside [src_offset, src_offset + uncomp_size) is read: the 16-byte loads end with the last FULL block in front of the block
// that holds the entry's last byte (k_classify put the entry on the list only with uncomp_size <= comp_size and the payload inside the
// image); nothing but res[e] is written.  No LDS.
#pragma once
#include "zpk_device.h"
#include "xxh3_device.h"

namespace zpk {

__global__ __launch_bounds__(256) void k_stored_hash(const u8* __restrict__ src, const zpk_decode_desc* __restrict__ desc,
                                                     zpk_decode_result* __restrict__ res, const u32* __restrict__ list,
                                                     const u32* __restrict__ counters)
{
    const int lane = lane_id();
    const u32 idx = uni((u32)(((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6));     // one wave per work-list slot, as k_stored
    if (idx >= uni(counters[C_NONE])) return;
    const u32 e = uni(list[idx]);
    const zpk_decode_desc d = desc[e];
    const u8* in = uni_ptr(src + d.src_offset);
    const u64 len = uni64(d.uncomp_size);
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
    int status = R_OK;
    if (!(d.flags & ZPK_DF_SKIP_HASH) && h != d.expect_hash) status = R_FILE_HASH_MISMATCH;
    lane0_guard();
    if (lane == 0) {
        zpk_decode_result r; r.status = status; r.detail = 0; r.produced = len; r.hash = h;
        res[e] = r;
    }
}

}  // namespace zpk
