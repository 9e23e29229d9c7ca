/* zpack_amd.h — extensions of libzpack_amd.so beyond the reference's API.
 *
 * zpack.h stays the reference's header, prototype for prototype; what this library adds on its own lives here. */
#ifndef ZPACK_AMD_H
#define ZPACK_AMD_H

#include "zpack.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Read-ahead counters of the context a zpack_read_file(reader, ..., dctx) call would use: dctx, else the reader's own
 * (all zero when it has none yet).
 *   out[0] calls served from a read-ahead window      out[1] calls decoded on their own
 *   out[2] windows decoded                            out[3] entries decoded ahead and never served
 *   out[4] host bytes the window holds now            out[5] the window cap in bytes (ZPACK_AMD_READ_AHEAD; 0 = off)
 * Returns ZPACK_OK, or ZPACK_ERROR_STREAM_INVALID when out is NULL. */
ZPACK_EXPORT int zpack_amd_read_ahead_stats(const zpack_reader* reader, void* dctx, zpack_u64 out[6]);

#ifdef __cplusplus
}
#endif

#endif
