// span_copy.hip — k_span_copy (span_copy.h) as a code object of its own, and the one host function that launches it.  zpk_codec.hip
// builds the row table and calls span_copy_launch; keeping the kernel out of that file keeps its code object, and where every other
// kernel lies in it, unchanged.
#include <hip/hip_runtime.h>
#include "span_copy.h"

namespace zpk {

void span_copy_launch(const SpanCopyRow* d_rows, u32 nrows, u64 item0, u64 nitems, u32 grid, hipStream_t st)
{
    hipLaunchKernelGGL(k_span_copy, dim3(grid), dim3(256), 0, st, d_rows, nrows, item0, nitems);
}

}  // namespace zpk
