// big_walk.h — k_big_walk: the block walk of host_walk.h (walk_lz4_single_into, walk_zstd_single_into) run ON THE DEVICE, over every large
// entry of a device-resident batch at once (zpk_codec_decode_big_batch_device).  The walk inside one entry is a chain of dependent loads —
// a block header says where the next one is — but entries are independent: one wave per candidate, lane 0 carries the chain, the other
// lanes leave at once.  The compressed bytes are read where they are (d_archive + src_offset, any alignment, every read checked against
// comp_size by the shared walkers exactly as on the host); only the block tables and one record per candidate go home.
//   - loads: the entry's bytes have no alignment (hrd32 / hrd64 are memcpy of align 1), so the compiler reads them with VECTOR loads —
//     bytes or unaligned dwords, which global memory takes; a scalar load needs a dword-aligned address and is chosen only for the
//     aligned candidate record;
//   - stores: plain C++ assignments by lane 0 = vector stores, table entries first, the record last;
//   - no LDS, no barrier, no atomics: a wave needs only its registers, so as many candidates are resident as the chip has wave slots.
#pragma once
#include "dec_plan.h"                            // (the public header, host_walk.h)

namespace zpk {

// BigWalkItem (one per candidate, host -> device), BigWalkRec (device -> host) and the staging layout [ items | records | tables ]: dec_plan.h

__global__ __launch_bounds__(64) void k_big_walk(const u8* __restrict__ archive, const BigWalkItem* __restrict__ items, u32 n,
                                                 u8* __restrict__ staging, BigWalkRec* __restrict__ recs)
{
    const u32 i = blockIdx.x;
    if (i >= n || threadIdx.x != 0) return;
    const BigWalkItem it = items[i];
    const u8* const p = archive + it.src_off;
    BigWalkRec r; r.accepted = 0; r.nblocks = 0; r.independent = 0; r.pad = 0; r.slots = 0; r.lit_total = 0;
    if (it.method == ZPK_METHOD_LZ4) {
        int independent = 0;
        r.accepted = walk_lz4_single_into(p, it.comp, it.uncomp, (PjBlock*)(staging + it.tab_off), it.cap, &r.nblocks, &independent) ? 1u : 0u;
        r.independent = (u32)independent;
    } else {
        r.accepted = walk_zstd_single_into(p, it.comp, it.uncomp, (ZpjBlock*)(staging + it.tab_off), it.cap, &r.nblocks, &r.slots, &r.lit_total) ? 1u : 0u;
    }
    recs[i] = r;
}

}  // namespace zpk
