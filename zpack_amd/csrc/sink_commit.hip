// sink_commit.hip — k_sink_cut and k_sink_place (sink_commit.h) as a code object of their own, and the one host function that launches
// them.  zpk_codec.hip stages, encodes and scans a sub-batch and calls sink_commit_launch; keeping the kernels out of that file keeps its
// code object, and where every other kernel lies in it, unchanged (as row_copy.hip does for the four row copies).
#include <hip/hip_runtime.h>
#include "sink_commit.h"

namespace zpk {

void sink_commit_launch(const u8* d_slots, const u64* d_slot_off, const zpk_encode_result* d_res, const u64* d_offsets, const u64* d_span_first,
                        u32 n, u64 room, u64* d_rec, u8* d_sink, u32 grid, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st)
{
    hipLaunchKernelGGL(k_sink_cut, dim3(1), dim3(256), 0, st, d_res, d_offsets, n, room, d_rec);
    if (ev0) (void)hipEventRecord(ev0, st);
    hipLaunchKernelGGL(k_sink_place, dim3(grid), dim3(256), 0, st, d_slots, d_slot_off, d_res, d_offsets, d_span_first, d_rec, d_sink);
    if (ev1) (void)hipEventRecord(ev1, st);
}

}  // namespace zpk
