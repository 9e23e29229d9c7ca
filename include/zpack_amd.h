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

/* ---- plaintext in DEVICE memory ---------------------------------------------------------------------------------------------------
 * zpack_read_files, zpack_read_files_packed and zpack_write_files with the PLAINTEXT in device memory: it stays on the device and only
 * the compressed bytes cross the bus, where a caller of the host forms pays the bus twice (the plaintext home, then up again; or down,
 * then up again).
 *
 * Call model.  Synchronous: a call returns when the buffers hold the plaintext / the archive holds the entries.  `entries`, `results`,
 *   `max_sizes`, `out_offsets` and the zpack_file array (its filenames and options) are host memory; the reader is memory-backed or
 *   file-backed and the writer heap- or file-backed, as for the host forms.
 * results[i], the bytes, last_return.  results[i] and the bytes in d_buffers[i] are what zpack_read_files gives for the same arguments
 *   with host buffers; reader->last_return is set by the same rule (the last entry's, or the last failing one's).  One bad entry does
 *   not stop the others.
 * Packed offsets.  out_offsets[i] is the running sum of the uncomp_size of the entries before i, EACH ROUNDED UP TO 256 (the host form
 *   packs without gaps); an entry that does not fit buffer_size from there gets ZPACK_ERROR_BUFFER_TOO_SMALL, as in the host form.
 * The written archive.  Byte for byte the one zpack_write_files writes from host copies of the same bytes; the writer's file entries,
 *   hashes, offsets and write_offset are equal too, and so is the return value when a file fails.
 * No device.  Every call returns ZPACK_ERROR_NOT_AVAILABLE: there is no CPU fallback.
 * Bad arguments.  A NULL reader / writer, or a NULL array (or d_buffer) with count > 0, is ZPACK_ERROR_STREAM_INVALID, checked before
 *   any context is created.  A device pointer that is not what it has to be — NULL with bytes to move, host memory, memory of another
 *   device than the others', a range that leaves its allocation — is ZPACK_ERROR_STREAM_INVALID too: every [pointer, pointer + size)
 *   is checked on the host against the allocation it points into before anything is enqueued, nothing has run and no result is set.
 * Which device.  All device pointers of a call belong to ONE device; it must be one of the context's (dctx, the files' common cctx,
 *   else the reader's / writer's own: ZPACK_AMD_DEVICES), else ZPACK_ERROR_NOT_AVAILABLE.  The batch runs on that device's codec alone.
 * Stream ordering.  The caller's earlier work on the buffers must have completed (synchronise the stream that produced them): the codec
 *   runs on a stream of its own.  When a call returns, its own work on them has completed.
 * Read-ahead.  The calls neither use nor feed the read-ahead windows of zpack_read_file. */

/* zpack_read_files with DEVICE destinations: d_buffers[i] / max_sizes[i] are device memory */
ZPACK_EXPORT int zpack_amd_read_files_device(zpack_reader* reader, zpack_file_entry* const* entries, zpack_u64 count,
                                             void* const* d_buffers, const size_t* max_sizes, int* results, void* dctx);
/* zpack_read_files_packed with a DEVICE buffer; entry i lands at out_offsets[i] */
ZPACK_EXPORT int zpack_amd_read_files_device_packed(zpack_reader* reader, zpack_file_entry* const* entries, zpack_u64 count,
                                                    void* d_buffer, size_t buffer_size, zpack_u64* out_offsets,
                                                    int* results, void* dctx);
/* zpack_write_files where files[i].buffer is a DEVICE pointer (files[i].size bytes) */
ZPACK_EXPORT int zpack_amd_write_files_device(zpack_writer* writer, zpack_file* files, zpack_u64 file_count);

#ifdef __cplusplus
}
#endif

#endif
