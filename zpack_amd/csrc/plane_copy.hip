// plane_copy.hip — k_plane_copy (plane_copy.h) as a code object of its own, and the one host function that launches it.  zpk_codec.hip
// builds the row table and calls plane_copy_launch; keeping the kernel out of that file keeps its code object, and those of span_copy.hip,
// sink_commit.hip and stored_hash.hip, unchanged.
#include <hip/hip_runtime.h>
#include "plane_copy.h"

namespace zpk {

void plane_copy_launch(const PlaneCopyRow* d_rows, u32 nrows, u64 item0, u64 nitems, u32 grid, hipStream_t st)
{
    hipLaunchKernelGGL(k_plane_copy, dim3(grid), dim3(256), 0, st, d_rows, nrows, item0, nitems);
}

}  // namespace zpk
