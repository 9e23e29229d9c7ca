// window_copy.hip — k_window_copy (window_copy.h) as a code object of its own, and the one host function that launches it.  zpk_codec.hip
// builds the row table and calls window_copy_launch; keeping the kernel out of that file keeps its code object, and those of span_copy.hip,
// sink_commit.hip, stored_hash.hip, plane_copy.hip, delta_copy.hip and span_hash.hip, unchanged.
#include <hip/hip_runtime.h>
// plane_copy.h, which window_copy.h includes for pc_group, pc_ld and pc_st, also defines the kernel k_plane_copy, and that file stays as
// it is.  The kernel belongs to plane_copy.hip: a second definition under the same name would not link, so the copy this file cannot
// avoid compiling gets another name, as in delta_copy.hip.  Nothing launches it.
#define k_plane_copy k_plane_copy_twin_of_window_copy
#include "window_copy.h"
#undef k_plane_copy

namespace zpk {

void window_copy_launch(const WindowCopyRow* d_rows, u32 nrows, u64 item0, u64 nitems, u32 grid, hipStream_t st)
{
    hipLaunchKernelGGL(k_window_copy, dim3(grid), dim3(256), 0, st, d_rows, nrows, item0, nitems);
}

}  // namespace zpk
