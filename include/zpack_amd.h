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
 *   `max_sizes`, `out_offsets` and the zpack_file array (its filenames and options) are host memory; the reader is memory-backed,
 *   file-backed or over an image in device memory (zpack_amd_init_reader_device, below) and the writer heap- or file-backed or over an image in device memory
 *   (zpack_amd_init_writer_device, further below).
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

/* ---- BYTE-PLANE entries: float tensors that compress ----------------------------------------------------------------------------------
 * A float tensor alternates bytes that compress (sign and exponent) with bytes that are noise (mantissa); stored with byte 0 of every
 * element first, then byte 1 of every element, and so on, the codecs gain on it (DESIGN.md section 10.5 has the figures).  For an entry of
 * n bytes with element size k in {2, 4, 8} and m = n / k whole elements:
 *     stored[p * m + j] = plain[j * k + p]   (0 <= p < k, 0 <= j < m),   stored[k * m + t] = plain[k * m + t] for the n - k * m tail bytes;
 * k = 1 is the identity.  The two calls below are zpack_amd_write_files_device and zpack_amd_read_files_device with one element size per
 * entry (host memory, file_count / count values): the grouping happens inside the copy that moves the plaintext between the caller's
 * buffers and the codec's staging anyway, so it costs no further pass over the plaintext and no second copy of it.  The .zpk format does
 * not change: a grouped entry is an ordinary entry whose plaintext is the grouped bytes, its hash is over those, any reader reads and
 * verifies it (and gets the grouped bytes), zpack_amd_test_files works on it unchanged.  The element size is NOT in the archive: the
 * caller hands the same value to both sides.  Every kind of writer (heap, file, device image) and reader (memory, file, device image).
 *
 * elem_sizes == NULL is zpack_amd_write_files_device / zpack_amd_read_files_device, the same code.
 * A value outside {1, 2, 4, 8} is ZPACK_ERROR_STREAM_INVALID, checked before any context is created: nothing is written, no result is set.
 * The written archive is byte for byte the one zpack_amd_write_files_device writes from device buffers that already hold the grouped
 *   bytes; entries, hashes, offsets, write_offset and the return value when a file fails are equal too.
 * results[i], the return value and reader->last_return are those of zpack_amd_read_files_device for the same entries.  The bytes in
 *   d_buffers[i] are the JOIN of the bytes that call delivers when entry i decodes to all of its uncomp_size bytes (ZPACK_OK or
 *   ZPACK_ERROR_FILE_HASH_MISMATCH); otherwise the buffer is untouched.
 * Which device, stream ordering, read-ahead, bad pointers, no device: as for the calls beside them (above). */
ZPACK_EXPORT int zpack_amd_write_files_device_planes(zpack_writer* writer, zpack_file* files, zpack_u64 file_count, const zpack_u8* elem_sizes);
ZPACK_EXPORT int zpack_amd_read_files_device_planes(zpack_reader* reader, zpack_file_entry* const* entries, zpack_u64 count,
                                                    void* const* d_buffers, const size_t* max_sizes, const zpack_u8* elem_sizes,
                                                    int* results, void* dctx);

/* ---- DELTA entries: a tensor stored as its XOR against a base in device memory --------------------------------------------------------
 * What compresses in a checkpoint is its difference to the previous one, which the caller holds in device memory anyway: most weights do
 * not change in a step, those that do change in their low mantissa bits, so `new XOR old` is mostly zero bytes and its high byte planes
 * are almost all zero (DESIGN.md section 10.6 has the figures).  For an entry of n bytes with element size k in {1, 2, 4, 8} and a base
 * of n bytes:
 *     stored = split_k(plain XOR base)          plain = join_k(stored) XOR base
 * where split_k / join_k are the byte-plane layout above and k = 1 is the bare XOR; the base is indexed by plain byte index and the tail
 * bytes are XORed like the rest.  The two calls below are the _planes calls with one base per entry (host array of file_count / count
 * DEVICE pointers, on the same device as the other pointers; d_bases[i] covers files[i].size bytes writing and entries[i]->uncomp_size
 * bytes reading; NULL: entry i has no base and is a byte-plane entry).  The XOR rides on the copy that carries the plaintext anyway: one
 * more read stream, no further pass over the plaintext, no second copy of it.  The .zpk format does not change: a delta entry is an
 * ordinary entry whose plaintext is the stored bytes, its hash is over those, any reader reads and verifies it (and gets the stored
 * bytes), zpack_amd_test_files works on it unchanged.  NEITHER the element size NOR the base is in the archive: the caller hands the
 * same values to both sides; a base that is itself a delta entry is the caller's business.  Every kind of writer and reader.
 *
 * d_bases == NULL is the _planes call, the same code; elem_sizes == NULL: every entry has element size 1.
 * Reading, d_bases[i] == d_buffers[i] exactly is legal: the buffer that holds the previous checkpoint becomes the new one, no second copy
 *   of the tensor.  A base that is not that many bytes of one allocation on that device, or that overlaps its destination in any other
 *   way, is ZPACK_ERROR_STREAM_INVALID, checked before anything is enqueued: nothing is read or written, no result is set.
 * The written archive is byte for byte the one zpack_amd_write_files_device_planes writes from device buffers that already hold
 *   plain XOR base; entries, hashes, offsets, write_offset and the return value when a file fails are equal too.
 * results[i], the return value and reader->last_return are those of zpack_amd_read_files_device_planes for the same entries.  The bytes
 *   in d_buffers[i] are that call's bytes XOR the base when entry i decodes to all of its uncomp_size bytes (ZPACK_OK or
 *   ZPACK_ERROR_FILE_HASH_MISMATCH); otherwise the buffer is untouched — with d_bases[i] == d_buffers[i] the previous checkpoint
 *   survives a damaged entry.
 * Which device, stream ordering, read-ahead, no device (ZPACK_ERROR_NOT_AVAILABLE): as for the calls beside them (above). */
ZPACK_EXPORT int zpack_amd_write_files_device_delta(zpack_writer* writer, zpack_file* files, zpack_u64 file_count,
                                                    const zpack_u8* elem_sizes, const void* const* d_bases);
ZPACK_EXPORT int zpack_amd_read_files_device_delta(zpack_reader* reader, zpack_file_entry* const* entries, zpack_u64 count,
                                                   void* const* d_buffers, const size_t* max_sizes, const zpack_u8* elem_sizes,
                                                   const void* const* d_bases, int* results, void* dctx);

/* ---- the BASE of a delta entry, checked on the device before it is applied --------------------------------------------------------------
 * A delta entry's hash is over its STORED bytes, so a read against the wrong base — the checkpoint of another step, the same step after
 * an optimizer update, a buffer of the right size from another tensor — decodes, verifies, returns ZPACK_OK and hands out garbage; with
 * d_bases[i] == d_buffers[i] it overwrites the only copy of the previous checkpoint with it.  The two calls below close that: the writing
 * side hashes its bases where they lie and keeps the values (there is no new write call; the .zpk format does not record them), the
 * reading side hands them back in and the library hashes the bases it is given before it applies them.
 *
 * zpack_amd_hash_device.  hashes[i] = XXH3-64 (seed 0) of the sizes[i] bytes of device memory at d_ptrs[i], any alignment, hashed on
 *   the device — one wave per span, a large span by the whole chip; nothing but the hashes crosses the bus.  The value is the `hash` field
 *   the reference writes for an entry with those plain bytes, so a tensor in device memory can also be compared with a plain archive's
 *   entry without reading it.  sizes[i] == 0 gives the hash of the empty input and d_ptrs[i] is not looked at.  Synchronous.  dctx: a
 *   context of zpack_create_dctx whose devices include the pointers' (else ZPACK_ERROR_NOT_AVAILABLE), or NULL: a context of the call's
 *   own, created and freed inside it.  Pointers, device and errors as for the calls above: all on ONE device, ZPACK_ERROR_STREAM_INVALID
 *   for a NULL array with count > 0 or a span that is not that many bytes of one allocation (nothing has run), ZPACK_ERROR_NOT_AVAILABLE
 *   without a device.
 * zpack_amd_read_files_device_delta_checked.  zpack_amd_read_files_device_delta with base_hashes[i], the XXH3-64 the base of entry i has
 *   to have (host memory, count values; the value of an entry with d_bases[i] == NULL is ignored).  base_hashes == NULL IS the _delta
 *   call, the same code.  An entry with a base is delivered only when its base hashes to its value.  When it does not, NO byte of
 *   d_buffers[i] is written — in place, the previous checkpoint survives — and, exactly where the entry would otherwise have been
 *   delivered (ZPACK_OK or ZPACK_ERROR_FILE_HASH_MISMATCH), results[i] is ZPACK_AMD_ERROR_BASE_MISMATCH; every other result stays the
 *   entry's own.  The call still returns ZPACK_OK: one bad entry does not stop the others.  reader->last_return follows the rule of the
 *   _delta call with that result.  Every kind of reader. */
#define ZPACK_AMD_ERROR_BASE_MISMATCH 64     /* a value of results[i] beside enum zpack_result (zpack.h), which ends at ZPACK_ERROR_NOT_AVAILABLE = 24 */
ZPACK_EXPORT int zpack_amd_hash_device(const void* const* d_ptrs, const size_t* sizes, zpack_u64 count, zpack_u64* hashes, void* dctx);
ZPACK_EXPORT int zpack_amd_read_files_device_delta_checked(zpack_reader* reader, zpack_file_entry* const* entries, zpack_u64 count,
                                                           void* const* d_buffers, const size_t* max_sizes, const zpack_u8* elem_sizes,
                                                           const void* const* d_bases, const zpack_u64* base_hashes, int* results, void* dctx);

/* ---- WINDOW reads: a slice of an entry delivered to device memory -------------------------------------------------------------------------
 * A checkpoint is often loaded under another layout than it was written under: tensor-parallel ranks that each own rows or columns of
 * every weight, a pipeline stage that needs part of an embedding.  Such a reader needs a SLICE of every tensor, and the calls above make
 * it allocate every tensor whole and cut its part out with a second pass.  A WINDOW is a 2-D sub-block of an entry's plain bytes seen
 * as a matrix of rows x row_bytes; the copy that delivers the entry writes it densely into a buffer of window size, joining the byte
 * planes and XORing the base on the way.  All fields in bytes; row_bytes == 0: no window, the entry whole.
 * For an entry of n = uncomp_size plain bytes with element size k = elem_sizes[i] (1 without) a window is VALID when row_bytes > 0,
 *   n % row_bytes == 0, row_bytes, col0 and cols are multiples of k, col0 + cols <= row_bytes and row0 + rows <= n / row_bytes, no sum
 *   wrapping.  window_bytes = rows * cols, which may be 0.  Byte d of the buffer, d in [0, window_bytes), is plain byte
 *   (row0 + d / cols) * row_bytes + col0 + d % cols of the entry, XOR byte d of the base when there is one.
 * A slice [start, stop) along dimension `dim` of a contiguous tensor of `shape` and `itemsize` is the window
 *   row_bytes = shape[dim] * inner, row0 = 0, rows = prod(shape[:dim]), col0 = start * inner, cols = (stop - start) * inner,
 *   with inner = prod(shape[dim + 1:]) * itemsize.
 *
 * zpack_amd_read_files_device_windows.  zpack_amd_read_files_device_delta_checked with windows[i], the window of entry i (host memory,
 *   count values).  windows == NULL IS that call, the same code.  Every kind of reader.  For an entry with a window:
 *   d_buffers[i], d_bases[i] and base_hashes[i] are about window_bytes bytes — the base is the caller's shard of the previous checkpoint,
 *     indexed like the buffer; d_bases[i] == d_buffers[i] exactly is legal.
 *   max_sizes[i] < window_bytes: results[i] is ZPACK_ERROR_BUFFER_TOO_SMALL where zpack_read_file's guards, in their order, would say so
 *     of too small a buffer, nothing of the entry is decoded and nothing is written.
 *   Otherwise results[i] is what zpack_amd_test_files gives the entry (the tail of a short decode counts as zeros: a window buffer is
 *     no buffer of uncomp_size bytes), and ZPACK_AMD_ERROR_BASE_MISMATCH by the rule above.
 *   The bytes are the map above when the entry decoded to all of its uncomp_size bytes (ZPACK_OK or ZPACK_ERROR_FILE_HASH_MISMATCH) and
 *     its base was accepted; otherwise the buffer is untouched.
 * A window that is not valid, or a base of a windowed entry that overlaps its buffer other than by being it, is
 *   ZPACK_ERROR_STREAM_INVALID, judged before any context is created or anything is enqueued: no result is set.
 * Entries without a window in the same call, the return value and reader->last_return: as in the _delta_checked call. */
typedef struct zpack_amd_window { zpack_u64 row_bytes, row0, rows, col0, cols; } zpack_amd_window;
ZPACK_EXPORT int zpack_amd_read_files_device_windows(zpack_reader* reader, zpack_file_entry* const* entries, zpack_u64 count,
                                                     void* const* d_buffers, const size_t* max_sizes, const zpack_u8* elem_sizes,
                                                     const void* const* d_bases, const zpack_u64* base_hashes,
                                                     const zpack_amd_window* windows, int* results, void* dctx);

/* ---- PLACED reads: an entry delivered into a sub-block of a device tensor -------------------------------------------------------------------
 * The opposite direction.  A checkpoint written by 8 tensor-parallel ranks holds 8 shard entries per weight; a loader at another width —
 * an inference server, an evaluation job — puts several shards side by side in ONE tensor.  Along dimension 0 that is a pointer offset;
 * along any other each shard is a strided sub-block of the destination, and the calls above make the caller read every shard into a
 * scratch buffer and concatenate: a second pass over every plaintext byte and a scratch copy of the checkpoint.  A PLACED entry has a
 * window and a destination ROW PITCH in bytes; the copy that delivers the entry writes window row r at byte r * pitch of the buffer.
 * An entry read whole is the window row0 = 0, col0 = 0, cols = row_bytes, rows = uncomp_size / row_bytes.
 * A placement is VALID when the window is, pitch >= cols, and place_extent = (rows - 1) * pitch + cols (0 when rows * cols == 0) does
 *   not wrap; the pitch needs no alignment to the element size.  Window byte d, d in [0, window_bytes), lands at buffer byte
 *   (d / cols) * pitch + d % cols, XOR that same byte of the base when there is one: the base is the caller's previous checkpoint in
 *   the MERGED layout.  The bytes of the extent in the gaps [cols, pitch) of every row are never written and never read from the base.
 * The slice [start, start + length) along dimension `dim` of a contiguous destination of `shape` and `itemsize` is
 *   rows = prod(shape[:dim]), cols = length * inner, pitch = shape[dim] * inner, and d_buffers[i] = the tensor + start * inner,
 *   with inner = prod(shape[dim + 1:]) * itemsize.
 *
 * zpack_amd_read_files_device_placed.  zpack_amd_read_files_device_windows with dst_pitches[i], the pitch of entry i (host memory, count
 *   values).  dst_pitches == NULL IS that call, the same code; dst_pitches[i] == 0: entry i as that call treats it.  Every kind of
 *   reader.  For a placed entry:
 *   d_buffers[i] points at the FIRST BYTE of the sub-block: the caller adds the column offset.  max_sizes[i], d_bases[i] and the pointer
 *     rule are about place_extent bytes; d_bases[i] == d_buffers[i] exactly is legal, any other overlap of the two extents is not.
 *   max_sizes[i] < place_extent: results[i] is ZPACK_ERROR_BUFFER_TOO_SMALL as in the _windows call, and nothing is written.
 *   Otherwise results[i], the return value and reader->last_return are the _windows call's.  The bytes are delivered only when the entry
 *     decoded to all of its uncomp_size bytes (ZPACK_OK or ZPACK_ERROR_FILE_HASH_MISMATCH) and its base was accepted; otherwise no byte
 *     of the buffer is touched.  The gap bytes are never touched.
 *   The extents of different entries may interleave — that is the point.  Two entries whose PLACED bytes overlap are the caller's
 *     error and are not diagnosed.
 *   base_hashes[i] is the hash of a contiguous span, and a placed base is not one: a placed entry with a base in a call whose
 *     base_hashes is not NULL is refused (below) unless its extent equals its window bytes (rows <= 1 or pitch == cols), which is
 *     checked as ever.  Hash the whole merged base with zpack_amd_hash_device instead and read with base_hashes NULL.
 * A placement that is not valid, a pitch on an entry without a window, a base of a placed entry that overlaps its buffer other than by
 *   being it, or that base-hash case is ZPACK_ERROR_STREAM_INVALID, judged before any context is created or anything is enqueued: no
 *   result is set. */
ZPACK_EXPORT int zpack_amd_read_files_device_placed(zpack_reader* reader, zpack_file_entry* const* entries, zpack_u64 count,
                                                    void* const* d_buffers, const size_t* max_sizes, const zpack_u8* elem_sizes,
                                                    const void* const* d_bases, const zpack_u64* base_hashes,
                                                    const zpack_amd_window* windows, const zpack_u64* dst_pitches, int* results, void* dctx);

/* ---- the archive IMAGE in DEVICE memory -------------------------------------------------------------------------------------------
 * A third kind of reader beside the memory-backed and the file-backed one: the archive lies in device memory — a data set or checkpoint
 * kept compressed in HBM, an archive that arrived by a device-to-device transfer — and its compressed bytes never cross the bus.
 *
 * After a successful init.  version, file_entries, file_count, comp_size, uncomp_size, file_size, cdr_offset and eocdr_offset are what
 *   zpack_init_reader_memory gives for the same bytes; the names are reader-owned.  buffer == NULL and file == NULL: where the image
 *   lives is kept beside the reader (zpack_reader has the reference's fixed layout), zpack_amd_reader_device_image tells.  The image is
 *   BORROWED, as in zpack_init_reader_memory_shared: the caller keeps it alive and unmodified until zpack_close_reader, which does not
 *   free it.  zpack_close_reader and a failed init drop the record: the struct then reads ZPACK_ERROR_ARCHIVE_NOT_LOADED like any reader
 *   that was never opened, and can be opened again, as any kind.
 * Return codes of the init.  A NULL reader or d_image is ZPACK_ERROR_STREAM_INVALID.  No HIP device: ZPACK_ERROR_NOT_AVAILABLE.  A
 *   pointer that is not device memory, or a range [d_image, d_image + size) that leaves its allocation, is ZPACK_ERROR_STREAM_INVALID,
 *   checked on the host before anything is copied.  For a valid range every container error is the code zpack_init_reader_memory
 *   returns for the same bytes (too small, a bad signature, a CDR that lies about its size ...).  Only the header, the EOCDR and the
 *   CDR are fetched to the host.
 * Which read calls work, and their results.  zpack_read_file, zpack_read_files, zpack_read_files_packed, zpack_amd_read_files_device,
 *   zpack_amd_read_files_device_packed, zpack_read_raw_file, zpack_read_raw_file_stream, zpack_read_file_stream, and
 *   zpack_write_files_from_archive with it as the source.  results[i], the bytes [0, produced) of every buffer, the return value and
 *   reader->last_return are exactly what the same call gives on a memory reader over a host copy of the image; nothing outside
 *   [buffer, buffer + max_size) is written.  The batch reads decode where the image lies: large frames block-parallel, large stored
 *   entries chip-wide, everything else one wave per entry, into the codec's staging; one kernel (device destinations) or one copy home
 *   (host destinations) hands the plaintext over.
 * Raw and stream reads fetch the bytes they need with a device-to-host copy; nothing else about them changes.
 * Read-ahead.  In-order zpack_read_file loops keep their read-ahead; its windows decode on the device like any batch.
 * Which device.  The image's device must be one of the context's (dctx, else the reader's own: ZPACK_AMD_DEVICES), else
 *   ZPACK_ERROR_NOT_AVAILABLE; device destinations must be on the image's device, else ZPACK_ERROR_STREAM_INVALID.  The batch runs on
 *   that device's codec alone, with no shard.
 * Stream ordering.  The caller's earlier work on the image (the copy that filled it ...) must have completed; the image is read-only to
 *   the library.
 * Calls that do not apply.  zpack_read_archive_memory and zpack_read_archive on such a reader return ZPACK_ERROR_ARCHIVE_NOT_LOADED: it
 *   has no host image and no file. */

/* A reader over an archive image in DEVICE memory: [d_image, d_image + size) on one HIP device.  The image is BORROWED
 * (as in zpack_init_reader_memory_shared): the caller keeps it alive and unmodified until zpack_close_reader, which
 * does not free it.  Parses header, EOCDR and CDR by fetching only those bytes to the host. */
ZPACK_EXPORT int zpack_amd_init_reader_device(zpack_reader* reader, const void* d_image, size_t size);
/* *d_image / *device of a reader opened by the call above (NULL / -1 for any other reader). */
ZPACK_EXPORT int zpack_amd_reader_device_image(const zpack_reader* reader, const void** d_image, int* device);

/* ---- entries TESTED on the device: verdicts without plaintext --------------------------------------------------------------------------
 * What `t` of the reference's command line does (programs/commands.c:706-773) and what a user does to a checkpoint before trusting it:
 * every entry is decoded and hashed, the verdict is kept, the bytes are not.  The verdict is complete on the device, so no plaintext
 * byte crosses the bus and the caller provides no buffer — for a reader over an image in device memory nothing crosses but descriptors
 * and results, and the image can stay compressed.
 *
 * Results.  results[i], the return value and reader->last_return are exactly what zpack_read_files gives for the same entries when
 *   buffer i is uncomp_size bytes, zero-filled; last_return by the same rule (the last entry's, or the last failing one's).  One bad
 *   entry does not stop the others.  ZPACK_ERROR_BUFFER_TOO_SMALL cannot occur.
 * Readers.  Memory-backed, file-backed and over an image in device memory.  Host and file readers shard over the context's devices
 *   (ZPACK_AMD_DEVICES) as zpack_read_files does; a file reader gathers the payloads as that call does; a device image runs on the
 *   image's device alone, which must be one of the context's (else ZPACK_ERROR_NOT_AVAILABLE).
 * Read-ahead.  The call neither uses nor feeds the read-ahead windows: zpack_amd_read_ahead_stats is unchanged by it.
 * Errors.  A NULL reader, or a NULL array with count > 0, is ZPACK_ERROR_STREAM_INVALID, checked before any context is created.
 *   count == 0 is ZPACK_OK.  No device: ZPACK_ERROR_NOT_AVAILABLE.  A reader that is not loaded: ZPACK_ERROR_ARCHIVE_NOT_LOADED.  Staging
 *   that cannot be allocated, on the host or on the device: ZPACK_ERROR_MALLOC_FAILED, and no result is set.
 * Short decodes.  An entry whose frames end before uncomp_size bytes exist is hashed by the reference over its decoded bytes and
 *   whatever the caller's buffer held behind them (lib/zpack_read.c:466).  Here there is no buffer: the tail counts as ZEROS — which is
 *   why the contract above says "zero-filled". */
ZPACK_EXPORT int zpack_amd_test_files(zpack_reader* reader, zpack_file_entry* const* entries, zpack_u64 count, int* results, void* dctx);

/* ---- a WRITER whose sink is an archive image in DEVICE memory ----------------------------------------------------------------------
 * A third kind of writer beside the heap- and the file-backed one: the archive is written where it will be used — a checkpoint or data
 * set kept compressed beside the model, an image about to leave by a device-to-device transfer — and its compressed bytes never cross
 * the bus.  With zpack_amd_init_reader_device the loop closes: written on the device, read on the device; only descriptors, results and
 * the small host-built blocks (header, data signature, CDR, EOCDR) touch the host.
 *
 * After a successful init.  buffer == NULL and file == NULL; buffer_capacity holds `capacity`.  Where the image lives is kept beside the
 *   writer (zpack_writer has the reference's fixed layout), zpack_amd_writer_device_image tells.  The image is BORROWED: the caller keeps
 *   it alive until zpack_close_writer, which frees the entry table and the writer's context, drops the record and leaves the image
 *   alone.  The sink does NOT grow.  A writer that was never opened still answers ZPACK_ERROR_WRITER_NOT_OPENED.
 * Return codes of the init.  A NULL writer or d_image is ZPACK_ERROR_STREAM_INVALID.  No HIP device: ZPACK_ERROR_NOT_AVAILABLE.  A
 *   pointer that is not device memory, or a range [d_image, d_image + capacity) that leaves its allocation, is
 *   ZPACK_ERROR_STREAM_INVALID, checked on the host; nothing is touched.
 * Which write calls work, and their results.  zpack_write_header[_ex], zpack_write_data_header, zpack_write_files, zpack_write_file,
 *   zpack_amd_write_files_device, zpack_write_files_from_archive, zpack_write_file_stream and _end, zpack_write_cdr[_ex],
 *   zpack_write_eocdr[_ex], zpack_write_archive.  After any sequence of calls the bytes [0, write_offset) of the image are the bytes of
 *   a heap writer's buffer after the same calls, and file_entries (names, offsets, sizes, hashes, methods), file_count, write_offset,
 *   file_size, cdr_offset, eocdr_offset, every return value and last_return are equal too.  Bytes in [write_offset, capacity) are
 *   unspecified; nothing outside [d_image, d_image + capacity) is ever written.
 * A full sink.  The reference's loop appends the files in front of the first failing one and stops (lib/zpack_write.c:299-303); a file
 *   that does not fit what is left of the image is treated the same way: the files in front of it are appended and entered, the call
 *   returns ZPACK_ERROR_BUFFER_TOO_SMALL and last_return is that file's comp_size.  A fixed block — header, data signature, CDR, EOCDR,
 *   an entry of a raw copy, a stream window — that does not fit writes nothing and returns ZPACK_ERROR_BUFFER_TOO_SMALL; the offsets do
 *   not move.
 * How a batch gets there.  zpack_write_files and zpack_amd_write_files_device make ONE codec call: the frames are compressed into the
 *   codec's staging (large entries in pieces, assembled on the device) and committed to the image by two kernels under the rule above;
 *   results and the cut come home, no compressed byte does.  zpack_write_files_from_archive from a reader over a device image on the
 *   same device is one copy kernel; from any other reader the payloads are fetched or read, then stored.
 * Which device.  The image's device must be one of the context's (the files' common cctx, else the writer's own: ZPACK_AMD_DEVICES),
 *   else ZPACK_ERROR_NOT_AVAILABLE; device plaintext (zpack_amd_write_files_device) on another device than the image is
 *   ZPACK_ERROR_STREAM_INVALID, and so is device memory handed to zpack_write_files as a host buffer: nothing is written.  The batch runs
 *   on the image's device's codec alone, with no shard.
 * Stream ordering.  Synchronous, like the other device calls: when a call returns, the image holds the bytes.  The caller's earlier work
 *   on the image and on device plaintext must have completed. */

/* A writer whose sink is [d_image, d_image + capacity) on one HIP device.  BORROWED: the caller keeps it alive until
 * zpack_close_writer, which does not free it.  The sink does not grow. */
ZPACK_EXPORT int zpack_amd_init_writer_device(zpack_writer* writer, void* d_image, size_t capacity);
/* *d_image / *capacity / *device of such a writer (NULL / 0 / -1 for any other writer). */
ZPACK_EXPORT int zpack_amd_writer_device_image(const zpack_writer* writer, void** d_image, size_t* capacity, int* device);

#ifdef __cplusplus
}
#endif

#endif
