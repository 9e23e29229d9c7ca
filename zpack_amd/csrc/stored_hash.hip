// stored_hash.hip — k_stored_hash (stored_hash.h) as a code object of its own, and the one host function that launches it.  decode_launch
// (zpk_codec.hip) calls stored_hash_launch in place of k_stored when the batch has no destination; keeping the kernel out of that file
// keeps its code object, and where every other kernel lies in it, unchanged (as row_copy.hip does for the four row copies).
#include <hip/hip_runtime.h>
#include "stored_hash.h"

namespace zpk {

void stored_hash_launch(const u8* src, const zpk_decode_desc* desc, zpk_decode_result* res, const u32* list, const u32* counters, u32 grid, hipStream_t st)
{
    hipLaunchKernelGGL(k_stored_hash, dim3(grid), dim3(256), 0, st, src, desc, res, list, counters);
}

}  // namespace zpk
