/*
 * zpack_codec.h — the thin C-ABI between the ZPack host library and the MI355X entry codec.
 *
 * This is the INWARD drop-in boundary: every third-party codec call the reference
 * makes on the per-entry hot path is replaced by one of the entry points below.  Plain C, plain
 * pointers and sizes, no torch / HIP types in any signature (streams travel as void*).
 *
 *   reference call site (file:line under /root/reference)              replaced by
 *   ------------------------------------------------------------------ ---------------------------
 *   lib/zpack_read.c:350-468   switch(comp_method){memcpy |            zpk_codec_decode_batch_device
 *        ZSTD_decompressDCtx :380 | LZ4F_decompress loop :414-439}      zpk_codec_decode_batch_host
 *        + XXH3_64bits verify :466-468, guards :328-332                 (one descriptor per entry)
 *                                                                       zpk_codec_decode_big_device / _big_batch_device
 *                                                                       (large entries in device memory, block-parallel)
 *   lib/zpack_write.c:161-224  zpack_compress_file {memcpy |            zpk_codec_encode_batch_device
 *        ZSTD_compressCCtx :179 | LZ4F_compressBegin/Update/End         zpk_codec_encode_batch_host
 *        :204-210} + XXH3_64bits :256
 *   lib/zpack_write.c:125-150  zpack_get_compress_bound                 zpk_codec_compress_bound
 *   lib/zpack_write.c:338      write_offset += comp_size (per file)     zpk_codec_pack_batch_device (scan + compaction)
 *   lib/zpack_read.c:466, lib/zpack_write.c:256  XXH3_64bits            zpk_codec_hash_batch_device / _host
 *   lib/zpack_read.c:17-31,776-812; lib/zpack_write.c:20-34,899-935     zpk_codec_create / _destroy / _reset
 *        ZSTD_createDCtx / LZ4F_createDecompressionContext / ...        (one opaque context for every method)
 *   lib/zpack_stream.c:4-28 XXH3 state; zpack_read.c:515-640;           zpk_dstream_* / zpk_cstream_*
 *        zpack_write.c:461-685 streaming calls                          (chunk aggregation over the batch codec)
 *
 * Status values are `enum zpack_result` codes (zpack.h): the device evaluates the same guards in the
 * same order as zpack_read_file, so `results[i].status` is exactly what zpack_read_file would have
 * returned for entry i, and one bad entry never poisons the batch.
 *
 * There is NO CPU fallback behind this interface: if no HIP device is usable, zpk_codec_create fails
 * with ZPK_E_NO_DEVICE and every zpack.h call that needs the codec returns ZPACK_ERROR_NOT_AVAILABLE.
 */
#ifndef ZPACK_CODEC_H
#define ZPACK_CODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZPK_CODEC_ABI_VERSION 3      /* 3: the two-stage LZ4 path of version 2 is gone (options 2..5 are ZPK_E_INVALID again, decode_stats2 out[2] = out[4] = 0,
                                        out[3] = LZ4 entries that are mostly runs, decoded by k_lz4_left); 2: set_option has options again.
                                        (Additive since 3, no renumbering: decode_stats2 out[8], out[9], which read 0: LZ4 entries the lean kernel handed to the general decoder / not plain frames.
                                        zpk_codec_encode_big_device, zpk_codec_encode_stats: large entries in device memory written in pieces.
                                        zpk_codec_decode_big_batch_device: a device-resident batch with large entries, their block headers walked on the device;
                                        decode_stats2 out[10], out[11], which read 0: entries walked there / those the walk accepted.
                                        ZPK_OPT_STORED_SPAN_MIN, decode_stats2 out[12], out[13], which read 0: large stored entries in device memory copied chip-wide / their groups.
                                        zpk_codec_decode_batch_host_dptr, zpk_codec_encode_batch_dsrc, zpk_codec_copy_spans_device, zpk_codec_pointer_device,
                                        zpk_codec_packed_stride: the host-pointer paths with the PLAINTEXT in the caller's device memory, and the kernel that moves it;
                                        decode_stats2 out[14], out[15], which read 0: sub-batches through the host path's pipeline / k_span_copy launches.
                                        zpk_codec_fetch_device, zpk_codec_decode_batch_dimage, ZPK_OPT_DIMAGE_CHUNK, zpk_codec_dimage_stats: the host-pointer paths
                                        with the ARCHIVE IMAGE in the caller's device memory.
                                        zpk_codec_store_device, zpk_codec_encode_batch_dsink, zpk_codec_dsink_stats, zpk_codec_stream_sync: a batch compressed into a bounded SINK in the
                                        caller's device memory.
                                        zpk_codec_verify_batch_host, zpk_codec_verify_batch_dimage, zpk_codec_verify_stats: a batch that is only TESTED, verdicts without plaintext.
                                        zpk_codec_plane_copy_device, the _planes forms of _encode_batch_dsrc, _encode_batch_dsink, _decode_batch_host_dptr and _decode_batch_dimage,
                                        zpk_codec_planes_stats: byte-plane entries, split and joined in the copies.
                                        zpk_codec_delta_copy_device, the _delta forms of the same four calls, zpk_codec_delta_stats: delta entries, a tensor stored as its XOR
                                        against a base in device memory.
                                        zpk_codec_hash_spans_device, ZPK_OPT_SPAN_HASH_MIN, the _delta_checked forms of the two reads that take bases, ZPK_R_BASE_MISMATCH,
                                        zpk_codec_base_check_stats: the base of a delta entry is hashed on the device before it is applied.
                                        zpk_codec_window_copy_device, the _windows forms of the same two reads, zpk_codec_window_stats: a 2-D sub-block of an entry
                                        delivered densely to device memory.
                                        zpk_codec_place_copy_device, the _placed forms of the same two reads, zpk_codec_place_stats: that sub-block delivered into a
                                        sub-block of a larger device tensor, several entries side by side.) */

/* return codes of the zpk_* entry points themselves (not per-entry statuses) */
enum {
    ZPK_OK = 0,
    ZPK_E_NO_DEVICE = -1,      /* no usable HIP device / runtime */
    ZPK_E_INVALID = -2,        /* bad argument */
    ZPK_E_NOMEM = -3,          /* host or device allocation failed */
    ZPK_E_LAUNCH = -4          /* HIP launch / copy error (hipGetLastError text via zpk_codec_last_error) */
};

/* compression methods — values of zpack_compression_method (zpack.h) */
enum { ZPK_METHOD_NONE = 0, ZPK_METHOD_ZSTD = 1, ZPK_METHOD_LZ4 = 2 };

/* One codec = one device context with ONE in-flight batch: its work lists, counters and staging buffers are shared by
 * every call.  Threading contract: the host-pointer entry points (*_host, the streaming triple) hold the codec's lock for
 * their whole duration — threads sharing a codec are serialised, never corrupted; the device-pointer entry points hold it
 * while they enqueue, and successive batches on ONE stream are ordered by that stream.  Do not drive one codec from two
 * streams at once: create one codec per stream / per thread (zpack.h contexts do exactly that). */
typedef struct zpk_codec zpk_codec;

/* One entry to decode.  Mirrors zpack_file_entry (lib/zpack.h:71-80) + the (buffer, max_size) pair of
 * zpack_read_file (lib/zpack.h:383).  `src_offset` is entry->offset: a byte offset into the archive
 * image `src` handed to the batch call (whose size plays reader->file_size in the :331 guard). */
typedef struct zpk_decode_desc {
    uint64_t src_offset;
    uint64_t comp_size;
    uint64_t uncomp_size;
    uint64_t expect_hash;
    uint64_t dst_offset;       /* byte offset of this entry's output slot inside `dst` */
    uint64_t dst_capacity;     /* max_size */
    uint32_t method;
    uint32_t flags;            /* ZPK_DF_* */
} zpk_decode_desc;

#define ZPK_DF_SKIP_HASH 1u    /* decode only; results[i].hash is still produced, status ignores it */
#define ZPK_DF_GENERAL   2u    /* accepted and ignored (round 2 used it to keep an entry off an opt-in LZ4 path that no longer exists) */

typedef struct zpk_decode_result {
    int32_t  status;           /* enum zpack_result */
    uint32_t detail;           /* codec-specific error detail (what the reference keeps in last_return) */
    uint64_t produced;         /* bytes written to the slot */
    uint64_t hash;             /* XXH3-64 of dst[0, uncomp_size) — what zpack_read.c:466 computes */
} zpk_decode_result;

typedef struct zpk_encode_desc {
    uint64_t src_offset;       /* plaintext offset inside `src` */
    uint64_t size;
    uint64_t dst_offset;       /* output slot offset inside `dst` */
    uint64_t dst_capacity;
    uint32_t method;           /* ZPK_METHOD_*, optionally | ZPK_EF_PIECE */
    int32_t  level;
} zpk_encode_desc;

/* The "entry" is a PIECE of a larger archive entry (large entries of the host write path, the streaming writer): its output is a run of
 * BLOCKS — no frame header, no EndMark / Last_Block — that whoever assembles the entry puts between a frame header and the end of the
 * frame (LZ4: the EndMark; Zstandard: an empty last block), so that the entry is ONE frame as the reference writer produces it
 * (lib/zpack_write.c:179, :204-210; round 4 made every piece a frame of its own: ABI 3 changed the meaning).  A piece's blocks do not
 * refer to the piece before it.  result.hash is left 0 (the entry's hash covers all pieces). */
#define ZPK_EF_PIECE 0x80000000u

typedef struct zpk_encode_result {
    int32_t  status;
    uint32_t detail;
    uint64_t comp_size;
    uint64_t hash;             /* XXH3-64 of the plaintext (lib/zpack_write.c:256) */
} zpk_encode_result;

/* ---- context lifecycle -------------------------------------------------------------------- */
int         zpk_codec_abi_version(void);
int         zpk_codec_device_count(void);
/* device: HIP ordinal, or -1 for "env ZPACK_AMD_DEVICE, else LOCAL_RANK, else 0" */
int         zpk_codec_create(zpk_codec** out, int device);
void        zpk_codec_destroy(zpk_codec* c);
void        zpk_codec_reset(zpk_codec* c);                  /* after an abandoned stream / error */
const char* zpk_codec_last_error(const zpk_codec* c);
int         zpk_codec_device(const zpk_codec* c);
/* options (ZPK_E_INVALID for anything else):
 *   ZPK_OPT_ENC_SPLIT_MIN           zpk_codec_encode_batch_host: an entry of at least `value` bytes is compressed as a SEQUENCE OF
 *                                   FRAMES, one per 512 KiB of plaintext, all of them side by side (one wave encodes one frame: a
 *                                   256 MiB entry is 512 waves instead of one), its XXH3 by the whole chip (per-block partial sums,
 *                                   then one short chain).  Both readers of the reference continue with the next frame
 *                                   (lib/zpack_read.c:380, :414-439), and the sequence fits the reference's own bound for the entry.
 *                                   Default 2 MiB; 0 = never split.
 *   ZPK_OPT_DEC_SPLIT_MIN           zpk_codec_decode_batch_host: an entry of at least `value` bytes that IS such a sequence (>= 2 frames
 *                                   that tile it exactly, each stating its content size; or a stored entry) is decoded with one wave
 *                                   per FRAME and hashed by the whole chip; any other entry, and any entry a frame of which fails,
 *                                   is decoded by one wave as before (verdicts come from there only).  Default 2 MiB; 0 = never.
 *   ZPK_OPT_ORDER_MIN               decode batches of at least `value` entries run their Zstandard and LZ4 work lists LARGEST ENTRIES
 *                                   FIRST (size classes by powers of two; a device counting sort behind the classification): one
 *                                   wave works on one entry, so a large entry that starts last runs on alone; encode batches order
 *                                   their ticket queue the same way.  Default 8192 (decode), 4608 (encode); 0 = never.
 *   ZPK_OPT_STORED_SPAN_MIN         zpk_codec_decode_big_batch_device, zpk_codec_decode_big_device: a STORED entry (method none) of at least
 *                                   `value` bytes that passes the guards of lib/zpack_read.c:328-354 is copied to its slot and hashed by the
 *                                   whole chip — one wave per 64 KiB, then one short chain per entry — instead of by one wave; anything
 *                                   else, and any entry that fails a guard, goes through the one-wave kernels (verdicts other than OK /
 *                                   hash mismatch come from there only).  Default 256 KiB; the least size taken is 1025; 0 = never.
 *   ZPK_OPT_DIMAGE_CHUNK            zpk_codec_decode_batch_dimage, zpk_codec_encode_batch_dsink: bytes of staging slots per sub-batch (an entry
 *                                   whose slot is larger goes alone).  0 = the default, ZPK_HOST_CHUNK_BYTES (4 GiB): what
 *                                   zpk_codec_decode_batch_host cuts by.
 *   ZPK_OPT_SPAN_HASH_MIN           zpk_codec_hash_spans_device and the base check of the _delta_checked reads: a span of at least `value`
 *                                   bytes is hashed by the whole chip — one wave per 64 KiB, then one short chain — instead of by one
 *                                   wave.  Default 256 KiB; the least size taken is 1025; 0 = never. */
/* (2..5 were the opt-in two-stage LZ4 path of round 4 and its measurement aids: measured slower than the one-kernel decoder, removed in round 5) */
enum { ZPK_OPT_ENC_SPLIT_MIN = 6, ZPK_OPT_DEC_SPLIT_MIN = 7, ZPK_OPT_ORDER_MIN = 8, ZPK_OPT_ORDER_FAST_LAST = 9 /* a batch of ONE size class runs the entries that did not compress (a copy to decode) last: 1 (default) / 0 */ };
#define ZPK_OPT_STORED_SPAN_MIN 10
#define ZPK_OPT_DIMAGE_CHUNK 11
#define ZPK_OPT_SPAN_HASH_MIN 12
int         zpk_codec_set_option(zpk_codec* c, int option, int value);

/* ---- batch decode + verify ----------------------------------------------------------------
 * Device-resident form: every pointer is a DEVICE pointer on the codec's device; work is enqueued on
 * `stream` (a hipStream_t passed as void*, NULL = the codec's own stream) and the call returns without
 * synchronising.  `src` is the archive image (or any packed frame stream), `n` descriptors.
 * `dst`, dst_offset and dst_capacity need no alignment, and slots may touch and lie in any order: nothing outside
 * [dst_offset, dst_offset + dst_capacity) of an entry is written, whatever its verdict, and nothing at all for an entry that is refused
 * before it is decoded (dst_capacity < uncomp_size, a slot that leaves dst).  The first `produced` bytes of a slot are the plaintext;
 * what lies behind them inside the slot is not specified. */
int zpk_codec_decode_batch_device(zpk_codec* c, const uint8_t* src, uint64_t src_size,
                                  const zpk_decode_desc* desc, uint64_t n,
                                  uint8_t* dst, uint64_t dst_size,
                                  zpk_decode_result* results, void* stream);

/* ONE entry whose compressed bytes are in DEVICE memory, decoded into device memory (d_dst + desc->dst_offset); desc and result are host
 * memory; returns when the entry is decoded and verified.  A large entry that is one frame of the reference writer
 * (lib/zpack_write.c:179, :204-210) is decoded block-parallel — 13-17 GiB/s instead of one wave's 0.03-0.14; anything else runs through the
 * kernels of zpk_codec_decode_batch_device.  A large STORED entry (ZPK_OPT_STORED_SPAN_MIN) is copied and hashed by the whole chip
 * (k_stored_span + the XXH3 chain); decode_stats2 out[12] / out[13] count it and its groups of 64 KiB.  Same verdicts either way (what
 * zpack_read_file would return, lib/zpack_read.c:326-471). */
int  zpk_codec_decode_big_device(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size, const zpk_decode_desc* desc,
                                 uint8_t* d_dst, uint64_t dst_size, zpk_decode_result* result);

/* A BATCH in device memory that holds large entries (the batch form of zpk_codec_decode_big_device): d_archive and d_dst are DEVICE
 * pointers, desc and results HOST memory; synchronous — returns when every entry is decoded and verified and results[0, n) are filled.
 * The compressed bytes never leave the device: one kernel (k_big_walk) walks the block headers of every candidate side by side — an LZ4 or
 * Zstandard entry of ZPK_OPT_DEC_SPLIT_MIN .. 4 GiB that passes the guards of lib/zpack_read.c:328-348 and whose slot lies inside dst_size —
 * and only its records and block tables (24 / 72 bytes per block, at most 2 * blocks-of-full-size + 8 blocks per entry: a frame with more
 * is declined) come to the host.  Of the frames the walk accepts, those worth a turn of the whole chip — by the estimate
 * zpk_codec_decode_batch_host uses — are decoded block-parallel, one after the other; every other entry, and every entry the block-parallel
 * path does not finish, goes through ONE launch of the kernels of zpk_codec_decode_batch_device.  Same verdicts as that call, entry by
 * entry; nothing outside [dst_offset, dst_offset + dst_capacity) of an entry is written.  n == 0: ZPK_OK; a NULL pointer with n > 0:
 * ZPK_E_INVALID.  zpk_codec_decode_stats2: out[5] / out[6] block-parallel entries / their blocks, out[10] entries walked on the device,
 * out[11] those the walk accepted.
 * Large STORED entries (round 17): an entry with method none of at least ZPK_OPT_STORED_SPAN_MIN bytes that passes the same guards is
 * copied to its slot and hashed by the whole chip on a second stream of the codec, beside everything else of the call — ONE launch of
 * k_stored_span for all of them (one wave per 64 KiB: each 1 KiB block is loaded once, stored and folded into its XXH3 partial sum), one
 * XXH3 chain wave per entry, the hashes come home in one copy; the call waits for that stream on every way out.  Status 0 or FILE_HASH_MISMATCH (ZPK_DF_SKIP_HASH honoured), detail 0, produced = uncomp_size: what the one-wave
 * kernel writes; nothing outside [dst_offset, dst_offset + uncomp_size) is written.  out[12] / out[13]: such entries / their groups of
 * 64 KiB; they are not part of out[0] of zpk_codec_decode_stats (no work list held them) nor of out[5] / out[6].
 * Not in this call: entries that are sequences of frames (round 4 archives) stay one wave per entry; the
 * block-parallel entries are not overlapped with one another or with the one-wave launch; zpk_codec_decode_big_device still walks on the
 * host.  libzpack_amd.so reaches this call's routing through zpk_codec_decode_batch_dimage below, for a reader whose image lies in device
 * memory (zpack_amd.h: zpack_amd_init_reader_device); a reader over host memory or a file, with the plaintext in device memory
 * (zpack_amd_read_files_device, _packed, zpack_amd_write_files_device), uses zpk_codec_decode_batch_host_dptr / zpk_codec_encode_batch_dsrc.
 * zpk-batch uses none of them. */
int  zpk_codec_decode_big_batch_device(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                       uint8_t* d_dst, uint64_t dst_size, zpk_decode_result* results);

/* Host form: host pointers, synchronous.  Stages [min src_offset, max src_offset+comp_size) of
 * `archive` to the device, decodes, and copies each slot back to dst_ptrs[i] (desc[i].dst_offset is
 * ignored; desc[i].dst_capacity is the size of dst_ptrs[i]).  zpack_read_file is a batch of one.
 * A compressed entry whose dst_capacity lies within 255 bytes of 2^64 has a staging slot no device holds: the call returns
 * ZPK_E_NOMEM ("a staging slot of ... bytes") before anything is enqueued for it; the sub-batches in front of it have run. */
int zpk_codec_decode_batch_host(zpk_codec* c, const uint8_t* archive, uint64_t archive_size,
                                const zpk_decode_desc* desc, uint64_t n,
                                uint8_t* const* dst_ptrs, zpk_decode_result* results);

/* zpk_codec_decode_batch_host with DEVICE destinations: archive, desc and results are host memory, d_dst_ptrs is a HOST array of n DEVICE
 * pointers on the codec's device (desc[i].dst_capacity bytes each); synchronous.  The routing is that call's — the sub-batches by
 * ZPK_HOST_CHUNK_BYTES, the sparse-pick gather, the frame-parallel and block-parallel routes of large entries (a block-parallel entry is
 * decoded straight into its pointer) — and so are results[i].  Where the host call copies a sub-batch's staging home and scatters it on
 * the host, this one issues ONE launch of k_span_copy that moves every slot to its pointer: exactly the bytes the host call copies to
 * dst_ptrs[i] — [0, produced) — and nothing outside [ptr, ptr + dst_capacity).  A sub-batch large enough for the three-stage pipeline keeps
 * its pipelined upload; the third stage is then one k_span_copy per piece, behind the piece's decode, in place of the download.
 * decode_stats2 out[14], out[15] (which read 0): sub-batches of the most recent host decode call that took the pipeline (either kind of
 * destination) / the k_span_copy launches of the most recent call of this kind.
 * POINTER CHECK, on the host before anything is enqueued: every [d_dst_ptrs[i], + dst_capacity) with dst_capacity > 0 must lie inside ONE
 * allocation on the codec's device (hipMemGetAddressRange; the last range is remembered, so a batch into one buffer costs one query),
 * else ZPK_E_INVALID and nothing has run — a wrong pointer is a return code, not a fault.
 * The caller's earlier work on those buffers must have completed: the codec runs on its own stream. */
int zpk_codec_decode_batch_host_dptr(zpk_codec* c, const uint8_t* archive, uint64_t archive_size,
                                     const zpk_decode_desc* desc, uint64_t n,
                                     uint8_t* const* d_dst_ptrs, zpk_decode_result* results);

/* ---- spans of device memory, copied by one kernel (k_span_copy) ----------------------------------
 * rows[0, n) is HOST memory, consumed before the call returns; src and dst are DEVICE addresses on the codec's device, any alignment;
 * spans must not overlap each other's destinations or their own source.  Every span goes through the pointer check above (source and
 * destination; len 0 passes and copies nothing): ZPK_E_INVALID and nothing has run.  Asynchronous on `stream` (NULL = the codec's own). */
typedef struct zpk_span_copy { uint64_t src, dst, len; } zpk_span_copy;
int zpk_codec_copy_spans_device(zpk_codec* c, const zpk_span_copy* rows, uint64_t n, void* stream);
/* the HIP ordinal of the device whose memory `ptr` points into, -1 when it is not device memory (host memory, NULL, no device) */
int zpk_codec_pointer_device(const void* ptr);
/* what an entry of uncomp_size bytes takes of a packed device read (zpack_amd_read_files_device_packed): uncomp_size rounded up to 256 */
uint64_t zpk_codec_packed_stride(uint64_t uncomp_size);

/* ---- the ARCHIVE IMAGE in the caller's device memory ------------------------------------------------
 * instance-free: copies [d_src, d_src + bytes) home, synchronously.  ZPK_E_INVALID when it is not `bytes` bytes of one allocation in
 * device memory (checked first, nothing copied); ZPK_E_NO_DEVICE without a runtime.  host_dst NULL: the check alone, nothing is copied
 * (how a caller validates a whole image before it fetches the few bytes it parses).  bytes 0: ZPK_OK wherever the pointers point. */
int zpk_codec_fetch_device(const void* d_src, void* host_dst, uint64_t bytes);

/* zpk_codec_decode_batch_host / _host_dptr with the ARCHIVE in device memory: desc and results are host memory, dst_ptrs a HOST array of
 * n host pointers (dst_on_device == 0) or n device pointers on the codec's device (1); synchronous.  The compressed bytes stay where
 * they are.  The batch is cut into sub-batches in the order given: a sub-batch closes when the next slot would take it past
 * ZPK_OPT_DIMAGE_CHUNK, an entry whose slot is larger goes alone; the slots are the host path's — what the entry may produce (a stored
 * entry: uncomp_size), at multiples of 256, in the codec's staging (the block-parallel readers want outputs on 256-byte boundaries, so
 * nothing is decoded straight into a caller's pointer).  Each sub-batch runs the routing of zpk_codec_decode_big_batch_device into that
 * staging — the walk on the device, the chooser, the chip-wide stored copies, one one-wave launch for everything else; results[i] are
 * that call's — and then the slots are handed over as the host calls do: ONE launch of k_span_copy with [slot, slot + produced) ->
 * pointer (device destinations), or the copy home and the host path's scatter (host destinations).  Nothing outside
 * [dst_ptrs[i], + dst_capacity) is written.
 * POINTER CHECK, on the host before anything is enqueued: [d_archive, + archive_size) and, with device destinations, every
 * [dst_ptrs[i], + dst_capacity) pass the check of zpk_codec_decode_batch_host_dptr, else ZPK_E_INVALID and nothing has run.
 * The caller's earlier work on the image and the buffers must have completed: the codec runs on its own stream.
 * decode_stats2 describes the call as it does zpk_codec_decode_big_batch_device (out[5], [6], [10]..[13] summed over the sub-batches). */
int zpk_codec_decode_batch_dimage(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size,
                                  const zpk_decode_desc* desc, uint64_t n,
                                  uint8_t* const* dst_ptrs, int dst_on_device, zpk_decode_result* results);
/* the most recent such call: out[0] sub-batches, out[1] k_span_copy launches, out[2] bytes copied home (saturating), out[3] 0 */
int zpk_codec_dimage_stats(zpk_codec* c, uint32_t out[4]);

/* ---- a batch that is only TESTED: verdicts without plaintext --------------------------------------------------------
 * zpk_codec_decode_batch_host and zpk_codec_decode_batch_dimage with NO destination (lib/zpack_read.c:326-471 as `command_test` of the
 * reference uses it, programs/commands.c:706-773: the bytes are thrown away, the verdict is kept).  desc and results are host memory;
 * `archive` is host memory, `d_archive` device memory on the codec's device (the pointer check of zpk_codec_decode_batch_dimage);
 * synchronous.  desc[i].dst_offset and .dst_capacity are ignored: the capacity counts as uncomp_size, so BUFFER_TOO_SMALL cannot occur,
 * and results[i] is field for field what the read call gives for buffers of exactly uncomp_size bytes filled with ZEROS — an entry whose
 * frames end before uncomp_size bytes exist is hashed with zeros behind its decoded bytes (the slot's tail is zeroed on the device).
 * The routing is that of the read calls, through their own code, with a third kind of destination: the frame-parallel and block-parallel
 * routes of large entries, the chip-wide route of large stored ones (k_xxh3_partials over the source instead of the fused copy), one
 * one-wave launch for the rest, the pipelined upload of a large host sub-batch (no download stream; decode_stats2 out[14] counts it).
 * A STORED entry has no staging slot at all: k_stored_hash, k_stored without the copy, hashes the payload where it lies.  Compressed
 * entries decode into the codec's staging, which is never copied anywhere: only the results come home, and no k_span_copy is launched.
 * Both calls cut their sub-batches by ZPK_OPT_DIMAGE_CHUNK.  decode_stats / decode_stats2 describe the call as they describe the read.
 * n == 0: ZPK_OK; a NULL desc, results or image with n > 0: ZPK_E_INVALID. */
int zpk_codec_verify_batch_host(zpk_codec* c, const uint8_t* archive, uint64_t archive_size,
                                const zpk_decode_desc* desc, uint64_t n, zpk_decode_result* results);
int zpk_codec_verify_batch_dimage(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size,
                                  const zpk_decode_desc* desc, uint64_t n, zpk_decode_result* results);
/* the most recent of these two calls (any later decode call counts its own): out[0] sub-batches, out[1] stored entries hashed in place —
 * those with a payload that passed every guard —, out[2] plaintext bytes that came home (saturating), which reads 0, out[3] 0 */
int zpk_codec_verify_stats(zpk_codec* c, uint32_t out[4]);

/* ---- batch encode + hash ------------------------------------------------------------------ */
size_t zpk_codec_compress_bound(uint32_t method, size_t src_size);
int zpk_codec_encode_batch_device(zpk_codec* c, const uint8_t* src, uint64_t src_size,
                                  const zpk_encode_desc* desc, uint64_t n,
                                  uint8_t* dst, uint64_t dst_size,
                                  zpk_encode_result* results, void* stream);
int zpk_codec_encode_batch_host(zpk_codec* c, const uint8_t* const* src_ptrs,
                                const zpk_encode_desc* desc, uint64_t n,
                                uint8_t* const* dst_ptrs, zpk_encode_result* results);
/* zpk_codec_encode_batch_host with DEVICE sources: d_src_ptrs is a HOST array of n DEVICE pointers on the codec's device (desc[i].size
 * bytes each), dst_ptrs and results stay host memory; synchronous.  The upload of the sources becomes ONE launch of k_span_copy that
 * gathers them into the same staging — which provides the 16 bytes of source slack the encode kernels ask for; a caller's tensor cannot
 * promise them — and everything behind it is the host call's code: dst_ptrs[i] and results[i] are byte for byte what that call gives
 * for host copies of the same bytes.  The pointer check of zpk_codec_decode_batch_host_dptr, on [d_src_ptrs[i], + size). */
int zpk_codec_encode_batch_dsrc(zpk_codec* c, const uint8_t* const* d_src_ptrs,
                                const zpk_encode_desc* desc, uint64_t n,
                                uint8_t* const* dst_ptrs, zpk_encode_result* results);

/* ---- a bounded SINK in the caller's device memory -------------------------------------------------------
 * instance-free, the mirror of zpk_codec_fetch_device: copies [host_src, host_src + bytes) to d_dst, synchronously.  ZPK_E_INVALID when
 * d_dst is not `bytes` bytes of one allocation in device memory (checked first, nothing copied); ZPK_E_NO_DEVICE without a runtime.
 * host_src NULL: the check alone.  bytes 0: ZPK_OK wherever the pointers point. */
int zpk_codec_store_device(void* d_dst, const void* host_src, uint64_t bytes);

/* zpk_codec_encode_batch_host / _dsrc whose payloads go, back to back in the order given, to [d_sink, d_sink + sink_room) in DEVICE
 * memory on the codec's device — under the append rule of the reference's loop (lib/zpack_write.c:299-303: the files in front of the
 * first failing one are appended), with "does not fit" as one more way to stop.  src_ptrs is a HOST array of n host pointers
 * (src_on_device == 0) or n device pointers on the codec's device (1); desc, results, placed and bytes are host memory; synchronous: when
 * the call returns the sink holds the bytes.  desc[i].src_offset and .dst_offset are ignored; desc[i].dst_capacity bounds entry i's frame
 * as in the host calls.
 * The sources are staged as those calls stage them (the upload, or ONE k_span_copy), the batch is cut into sub-batches by the bytes of its
 * staging slots (ZPK_OPT_DIMAGE_CHUNK), each sub-batch is encoded into slots of the codec's by the body of zpk_codec_encode_big_device
 * (large entries in pieces, their frame assembled on the device), scanned (offsets = the prefix sums of the sizes of the entries with
 * status 0) and committed by two kernels: k_sink_cut finds f, the first entry with status != 0 or offsets[f + 1] > room, and
 * k_sink_place — a persistent grid over (entry, 16 KiB span) items whose count it reads from the device — copies the payloads of [0, f)
 * to d_sink + offsets[i].  NOTHING is stored at or behind d_sink + offsets[f].  A later sub-batch lands behind the one before it; a cut
 * short of a sub-batch's entries ends the call.
 * *placed = the entries committed, in order from entry 0; *bytes = what they take; entry i of them lies at the sum of the comp_size of
 * those before it.  results[i] for i <= *placed (i < n) is byte for byte zpk_codec_encode_batch_host's, and so are the frames; entry
 * *placed, when there is one, is the one that stopped the call: by its status, else because its comp_size did not fit.  results behind
 * it are unspecified.  The only bytes that come home are [results | the cut], one copy per sub-batch.
 * POINTER CHECK, on the host before anything is enqueued: [d_sink, + sink_room) and, with device sources, every [src_ptrs[i], + size)
 * pass the check of zpk_codec_decode_batch_host_dptr; a host source with bytes must not be NULL or device memory.  Else ZPK_E_INVALID and
 * nothing has run. */
int zpk_codec_encode_batch_dsink(zpk_codec* c, const uint8_t* const* src_ptrs, int src_on_device,
                                 const zpk_encode_desc* desc, uint64_t n,
                                 uint8_t* d_sink, uint64_t sink_room,
                                 zpk_encode_result* results, uint64_t* placed, uint64_t* bytes);
/* the most recent such call: out[0] sub-batches, out[1] workgroups of its last k_sink_place launch, out[2] = out[3] = 0.  With profiling
 * on, zpk_codec_kernel_ms(ZPK_K_PACK) is the last k_sink_place's time. */
int zpk_codec_dsink_stats(zpk_codec* c, uint32_t out[4]);
/* returns when everything enqueued on the codec's own stream has run (zpk_codec_copy_spans_device with stream NULL enqueues there) */
int zpk_codec_stream_sync(zpk_codec* c);

/* ---- BYTE-PLANE entries: float tensors that compress, split and joined in the copies (k_plane_copy) -------------------------------
 * An entry of n bytes whose elements are k bytes wide (k in {2, 4, 8}; m = n / k whole elements) is STORED grouped by byte position:
 *     stored[p * m + j] = plain[j * k + p]   (0 <= p < k, 0 <= j < m),   stored[k * m + t] = plain[k * m + t] for the n - k * m tail bytes;
 * k = 1 is the identity.  The archive knows nothing of it: the grouped bytes are the entry's plaintext and its XXH3 is over them.  The
 * transposition rides on the copies that move plaintext between the caller's DEVICE buffers and the codec's staging anyway: sources are
 * SPLIT on the way in, decoded slots are JOINED on the way out — no further pass over the plaintext, no second copy of it.
 *
 * zpk_codec_plane_copy_device: the kernel on its own, as zpk_codec_copy_spans_device is k_span_copy's.  rows[0, n) is HOST memory, consumed
 * before the call returns; src and dst are DEVICE addresses on the codec's device, any alignment, not overlapping; join 0 takes plain
 * bytes at src to grouped bytes at dst, join 1 the reverse; elem 1 copies.  An element size outside {1, 2, 4, 8}, or a row that fails the
 * pointer check of zpk_codec_decode_batch_host_dptr on either end (len 0 passes): ZPK_E_INVALID and nothing has run.  Asynchronous on
 * `stream` (NULL = the codec's own). */
typedef struct zpk_plane_copy { uint64_t src, dst, len; uint32_t elem, join; } zpk_plane_copy;
int zpk_codec_plane_copy_device(zpk_codec* c, const zpk_plane_copy* rows, uint64_t n, void* stream);
/* The calls whose plaintext lies in the caller's device memory, with one more argument: elem[i] is the element size of entry i (HOST
 * memory, n values; NULL = every entry has element size 1, which IS the call without the suffix: the same body).  A value outside
 * {1, 2, 4, 8}: ZPK_E_INVALID and nothing has run.  A batch in which every elem is 1 launches exactly what the plain call launches.
 * Writing: the sources with elem > 1 reach the staging through k_plane_copy (split), the others through k_span_copy; everything behind
 * the staging sees grouped bytes.  Host sources (_dsink with src_on_device 0) take no element size but 1.
 * Reading: wherever a slot is handed to a device pointer, entries with elem > 1 go through k_plane_copy (join) — and only when the entry
 * decoded to all of its uncomp_size bytes (status OK or a hash mismatch); for every other status nothing is written to its buffer.  A
 * large frame that would decode straight into the caller's buffer decodes into the staging instead and is joined from there.  The
 * results are the plain call's.  Host destinations (_dimage with dst_on_device 0) take no element size but 1. */
int zpk_codec_encode_batch_dsrc_planes(zpk_codec* c, const uint8_t* const* d_src_ptrs,
                                       const zpk_encode_desc* desc, uint64_t n,
                                       uint8_t* const* dst_ptrs, zpk_encode_result* results, const uint8_t* elem);
int zpk_codec_encode_batch_dsink_planes(zpk_codec* c, const uint8_t* const* src_ptrs, int src_on_device,
                                        const zpk_encode_desc* desc, uint64_t n,
                                        uint8_t* d_sink, uint64_t sink_room,
                                        zpk_encode_result* results, uint64_t* placed, uint64_t* bytes, const uint8_t* elem);
int zpk_codec_decode_batch_host_dptr_planes(zpk_codec* c, const uint8_t* archive, uint64_t archive_size,
                                            const zpk_decode_desc* desc, uint64_t n,
                                            uint8_t* const* d_dst_ptrs, zpk_decode_result* results, const uint8_t* elem);
int zpk_codec_decode_batch_dimage_planes(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size,
                                         const zpk_decode_desc* desc, uint64_t n,
                                         uint8_t* const* dst_ptrs, int dst_on_device, zpk_decode_result* results, const uint8_t* elem);
/* the most recent of the calls above, or of the plain calls they extend: out[0] rows split, out[1] rows joined, out[2] k_plane_copy
 * launches, out[3] entries that decoded into the staging only because they were grouped */
int zpk_codec_planes_stats(zpk_codec* c, uint32_t out[4]);

/* ---- DELTA entries: a tensor stored as its XOR against a BASE in device memory (k_delta_copy) ---------------------------------------
 * What compresses in a checkpoint is its difference to the previous one, which the caller holds in device memory anyway: most weights do
 * not change in a step, those that do change in their low mantissa bits.  For an entry of n bytes with element size k in {1, 2, 4, 8}
 * and a base of n bytes:
 *     stored = split_k(plain XOR base)          plain = join_k(stored) XOR base
 * split_k / join_k are the byte-plane layout above; k = 1 is the bare XOR.  The base is indexed by PLAIN byte index, the tail bytes are
 * XORed like the rest.  An entry without a base is a byte-plane entry.  The archive knows nothing of it: the stored bytes are the entry's
 * plaintext and its XXH3 is over them; neither the element size nor the base is recorded, the caller hands both to both sides.  The XOR
 * rides on the copy that carries the plaintext anyway: one more read stream, no further pass, no second copy of the tensor.
 *
 * zpk_codec_delta_copy_device: the kernel on its own, as zpk_codec_plane_copy_device is k_plane_copy's.  rows[0, n) is HOST memory,
 * consumed before the call returns; src, dst and base are DEVICE addresses on the codec's device, any alignment; join 0 takes plain bytes
 * at src to stored bytes at dst, join 1 the reverse; the base has len bytes and lies beside the plain side.  On a JOIN base == dst
 * exactly is legal — the buffer that holds the previous checkpoint becomes the new one —; any other overlap of [base, base + len) with
 * [dst, dst + len), base == dst on a split, base == 0 with len > 0 (such a row belongs to zpk_codec_plane_copy_device), an element size
 * outside {1, 2, 4, 8}, or an end that fails the pointer check of zpk_codec_decode_batch_host_dptr (len 0 passes): ZPK_E_INVALID and
 * nothing has run.  The base may overlap the source freely (both are only read).  Asynchronous on `stream` (NULL = the codec's own). */
typedef struct zpk_delta_copy { uint64_t src, dst, base, len; uint32_t elem, join; } zpk_delta_copy;
int zpk_codec_delta_copy_device(zpk_codec* c, const zpk_delta_copy* rows, uint64_t n, void* stream);
/* The _planes calls with one more argument: d_base[i] is the base of entry i, DEVICE memory on the codec's device of the entry's plain
 * size (desc[i].size writing, desc[i].uncomp_size reading); HOST array of n pointers.  d_base == NULL IS the _planes call, the same body;
 * d_base[i] == NULL: entry i has no base.  elem == NULL: every element size is 1.  A base that fails the pointer check, or — reading —
 * overlaps its entry's destination other than by being it: ZPK_E_INVALID and nothing has run.  A batch without bases launches exactly
 * what the _planes call launches.
 * Writing: the sources with a base reach the staging through k_delta_copy (split); everything behind the staging sees the stored bytes.
 * Reading: an entry with a base is treated wherever an entry with elem > 1 is — it is delivered through k_delta_copy (join) only when it
 * decoded to all of its uncomp_size bytes (status OK or a hash mismatch), a large frame decodes into the staging and is joined from
 * there; for every other status nothing is written to its buffer, so with base == destination the previous checkpoint survives a damaged
 * entry.  The results are the plain call's.  Host sources and host destinations take no base. */
int zpk_codec_encode_batch_dsrc_delta(zpk_codec* c, const uint8_t* const* d_src_ptrs,
                                      const zpk_encode_desc* desc, uint64_t n,
                                      uint8_t* const* dst_ptrs, zpk_encode_result* results, const uint8_t* elem, const uint8_t* const* d_base);
int zpk_codec_encode_batch_dsink_delta(zpk_codec* c, const uint8_t* const* src_ptrs, int src_on_device,
                                       const zpk_encode_desc* desc, uint64_t n,
                                       uint8_t* d_sink, uint64_t sink_room,
                                       zpk_encode_result* results, uint64_t* placed, uint64_t* bytes, const uint8_t* elem, const uint8_t* const* d_base);
int zpk_codec_decode_batch_host_dptr_delta(zpk_codec* c, const uint8_t* archive, uint64_t archive_size,
                                           const zpk_decode_desc* desc, uint64_t n,
                                           uint8_t* const* d_dst_ptrs, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base);
int zpk_codec_decode_batch_dimage_delta(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size,
                                        const zpk_decode_desc* desc, uint64_t n,
                                        uint8_t* const* dst_ptrs, int dst_on_device, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base);
/* the most recent of the calls above, or of the calls they extend: out[0] rows split with a base, out[1] rows joined with a base, out[2]
 * k_delta_copy launches, out[3] entries that decoded into the staging only because they had a base (element size 1).
 * zpk_codec_planes_stats keeps its meaning: it counts the rows of k_plane_copy, which are those without a base. */
int zpk_codec_delta_stats(zpk_codec* c, uint32_t out[4]);

/* ---- the BASE of a delta entry, checked on the device before it is applied (k_span_hash) ------------------------------------------------
 * The XXH3 of a delta entry is over its STORED bytes: a read against the wrong base — another step's checkpoint, the same step after an
 * optimizer update, a buffer of the right size from another tensor — decodes, verifies and hands out garbage, and with base ==
 * destination it overwrites the only copy of the previous checkpoint with it.  The writer's side hashes its bases, the reader's side
 * hands the values back in, and the codec hashes the bases it is given before it joins anything.
 *
 * zpk_codec_hash_spans_device: XXH3-64 (seed 0: XXH3_64bits, the `hash` of an entry with those plain bytes) of n spans of DEVICE memory on
 * the codec's device, any alignment, out_hashes[i] that of [rows[i].addr, + rows[i].len).  rows and out_hashes are HOST memory; rows is
 * consumed and out_hashes is written before the call returns (the call waits for `stream`, NULL = the codec's own).  len 0 gives the
 * hash of the empty input and its address is not looked at.  Rows below ZPK_OPT_SPAN_HASH_MIN take one wave each, all in one launch; the
 * others go chip-wide.  Nothing outside the spans is read.  A row that fails the pointer check of zpk_codec_decode_batch_host_dptr:
 * ZPK_E_INVALID and nothing has run. */
typedef struct zpk_hash_span { uint64_t addr, len; } zpk_hash_span;
int zpk_codec_hash_spans_device(zpk_codec* c, const zpk_hash_span* rows, uint64_t n, uint64_t* out_hashes, void* stream);
/* The two _delta reads with one more argument: base_hash[i] is the XXH3-64 the base of entry i has to have (HOST memory, n values).
 * base_hash == NULL IS the _delta call, the same body; the value of an entry with d_base[i] == NULL is ignored.
 * THE RULE: an entry with a base is delivered only when its base hashes to base_hash[i].  When it does not, no byte of its destination is
 * written — with base == destination the previous checkpoint survives — and, exactly where the entry would otherwise have been
 * delivered (status OK or FILE_HASH_MISMATCH), results[i].status is ZPK_R_BASE_MISMATCH; every other status stays the entry's own.
 * hash, produced and detail are the _delta call's.  All bases are hashed in one pass in front of the decode; every verdict is known
 * before the first entry is delivered. */
#define ZPK_R_BASE_MISMATCH 64       /* a per-entry status beside enum zpack_result, whose values end at 24 */
int zpk_codec_decode_batch_host_dptr_delta_checked(zpk_codec* c, const uint8_t* archive, uint64_t archive_size,
                                                   const zpk_decode_desc* desc, uint64_t n,
                                                   uint8_t* const* d_dst_ptrs, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base,
                                                   const uint64_t* base_hash);
int zpk_codec_decode_batch_dimage_delta_checked(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size,
                                                const zpk_decode_desc* desc, uint64_t n,
                                                uint8_t* const* dst_ptrs, int dst_on_device, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base,
                                                const uint64_t* base_hash);
/* the most recent of the three calls above (or of a read they extend): out[0] spans hashed by one wave, out[1] spans hashed chip-wide,
 * out[2] bases that did not hash to their value, out[3] kernel launches of the hash pass */
int zpk_codec_base_check_stats(zpk_codec* c, uint32_t out[4]);

/* ---- WINDOW reads: a 2-D sub-block of an entry delivered to device memory (k_window_copy) ----------------------------------------------
 * A reader that owns part of every tensor — a tensor-parallel rank, a pipeline stage — otherwise reads each entry whole into a full-size
 * scratch buffer and cuts its part out with a second pass.  A WINDOW is a sub-block of the entry's plain bytes seen as a matrix of
 * rows x row_bytes; the copy that delivers the entry writes it densely into a destination of window size, joining the byte planes and
 * XORing the base on the way.  All fields in bytes; row_bytes == 0: no window, the entry whole.  For an entry of n plain bytes with
 * element size k the window is valid when row_bytes > 0, n % row_bytes == 0, row_bytes, col0 and cols are multiples of k,
 * col0 + cols <= row_bytes and row0 + rows <= n / row_bytes (no sum may wrap).  window_bytes = rows * cols, which may be 0.  For
 * destination byte d in [0, window_bytes):
 *     i(d)   = (row0 + d / cols) * row_bytes + col0 + d % cols
 *     dst[d] = stored[index_k(i(d))] ^ (base ? base[d] : 0)          index_k: where the byte-plane layout above keeps plain byte i
 * The base is indexed by DESTINATION byte: it is the caller's shard of the previous checkpoint, of window size.  A slice [start, stop)
 * along dimension `dim` of a contiguous tensor of `shape` and `itemsize` is the window row_bytes = shape[dim] * inner, row0 = 0,
 * rows = prod(shape[:dim]), col0 = start * inner, cols = (stop - start) * inner, with inner = prod(shape[dim + 1:]) * itemsize.
 *
 * zpk_codec_window_copy_device: the kernel on its own.  rows[0, n) is HOST memory, consumed before the call returns; src is the entry's
 * n stored bytes, dst and base (0: none) have window_bytes bytes; DEVICE addresses on the codec's device, any alignment.  base == dst
 * exactly is legal.  A window that is not valid, an element size outside {1, 2, 4, 8}, any other overlap of base and destination, or
 * an end that fails the pointer check of zpk_codec_decode_batch_host_dptr (no bytes pass): ZPK_E_INVALID and nothing has run.
 * Asynchronous on `stream` (NULL = the codec's own). */
typedef struct zpk_window { uint64_t row_bytes, row0, rows, col0, cols; } zpk_window;
typedef struct zpk_window_copy { uint64_t src, dst, base, n; zpk_window win; uint32_t elem, pad; } zpk_window_copy;
int zpk_codec_window_copy_device(zpk_codec* c, const zpk_window_copy* rows, uint64_t n, void* stream);
/* the rule on its own, instance-free, no device needed: 1 = `win` is a valid window of an entry of n plain bytes with element size elem
 * (*bytes, when not NULL, becomes window_bytes), 0 = it is not (row_bytes == 0 included) */
int zpk_codec_window_valid(uint64_t n, uint32_t elem, const zpk_window* win, uint64_t* bytes);
/* ... and the overlap rule of a valid window: 1 = base == dst or the two ranges of window_bytes bytes are disjoint */
int zpk_codec_window_overlap_ok(uint64_t base, uint64_t dst, const zpk_window* win);
/* The two _delta_checked reads with one more argument: win[i] is the window of entry i (HOST memory, n values).  win == NULL IS the
 * _delta_checked call, the same body; win[i].row_bytes == 0: entry i is read whole.  For an entry with a window the destination, the
 * base and base_hash[i] are about window_bytes bytes, and desc[i].dst_capacity is the room at the destination: with less than
 * window_bytes the entry is BUFFER_TOO_SMALL where the guards, in their order, say so, and nothing is written.  Otherwise the entry
 * decodes into the codec's staging with a slot of uncomp_size, a large frame too — its verdict is that of a buffer of exactly that
 * size — and is delivered through k_window_copy, whatever its element size or base, only when
 * it decoded to all of its uncomp_size bytes (status OK or a hash mismatch) and its base was not refused; for every other status no
 * byte of its buffer is written.  The tail of a short decode counts as zeros, as in zpk_codec_verify_batch_host.  A window that is not
 * valid against desc[i].uncomp_size and elem[i], a window with host destinations, or a base that overlaps its destination other than by
 * being it: ZPK_E_INVALID and nothing has run.  A batch without windows launches exactly what the _delta_checked call launches. */
int zpk_codec_decode_batch_host_dptr_windows(zpk_codec* c, const uint8_t* archive, uint64_t archive_size,
                                             const zpk_decode_desc* desc, uint64_t n,
                                             uint8_t* const* d_dst_ptrs, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base,
                                             const uint64_t* base_hash, const zpk_window* win);
int zpk_codec_decode_batch_dimage_windows(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size,
                                          const zpk_decode_desc* desc, uint64_t n,
                                          uint8_t* const* dst_ptrs, int dst_on_device, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base,
                                          const uint64_t* base_hash, const zpk_window* win);
/* the most recent of the three calls above (or of a call that could split or join): out[0] rows windowed, out[1] k_window_copy launches,
 * out[2] entries that decoded into the staging only because they had a window (element size 1, no base).  zpk_codec_planes_stats and
 * zpk_codec_delta_stats keep their meaning: they count the rows of k_plane_copy and k_delta_copy, which are those without a window. */
int zpk_codec_window_stats(zpk_codec* c, uint32_t out[3]);

/* ---- PLACED reads: an entry, or a window of it, delivered into a sub-block of a larger device tensor (k_place_copy) --------------------
 * A checkpoint written by 8 tensor-parallel ranks holds 8 shard entries per weight; a loader at another width puts several of them side
 * by side in one tensor, which along any dimension but the first makes each shard a strided sub-block of the destination.  A PLACED
 * entry has a valid window and a PITCH != 0, in bytes: window row r begins at byte r * pitch of the destination, and of the base.  An
 * entry read whole is the window row0 = 0, col0 = 0, cols = row_bytes, rows = n / row_bytes.  The placement is valid when the window is,
 * pitch >= cols, and place_extent = (rows - 1) * pitch + cols (0 when rows * cols == 0) does not wrap; the pitch needs no alignment to
 * the element size.  For window byte d in [0, window_bytes):
 *     o(d)      = (d / cols) * pitch + d % cols
 *     dst[o(d)] = plain[(row0 + d / cols) * row_bytes + col0 + d % cols] ^ (base ? base[o(d)] : 0)
 * The base is indexed by the same byte as the destination: it is the caller's previous checkpoint in the MERGED layout.  The bytes of
 * the extent in the gaps [cols, pitch) of every row are never written and never read from the base: they belong to the neighbouring
 * shards, and the extents of different rows may interleave.  The slice [start, start + length) along dimension `dim` of a contiguous
 * destination of `shape` and `itemsize` is rows = prod(shape[:dim]), cols = length * inner, pitch = shape[dim] * inner at the byte
 * offset start * inner, inner = prod(shape[dim + 1:]) * itemsize.
 * zpk_codec_place_copy_device: the kernel on its own.  rows[0, n) is HOST memory, consumed before the call returns; src is the entry's
 * n stored bytes, dst and base (0: none) span place_extent bytes; DEVICE addresses on the codec's device, any alignment.  base == dst
 * exactly is legal; any other overlap of the two ranges of place_extent bytes is not.  A placement that is not valid, an element size
 * outside {1, 2, 4, 8}, such an overlap, or a pointer that fails the rule over those lengths: ZPK_E_INVALID and NOTHING has run, the
 * good rows beside the bad one included.  A row of no bytes (n == 0 or rows * cols == 0) passes wherever it points. */
typedef struct zpk_place_copy { uint64_t src, dst, base, n; zpk_window win; uint64_t pitch; uint32_t elem, pad; } zpk_place_copy;
int zpk_codec_place_copy_device(zpk_codec* c, const zpk_place_copy* rows, uint64_t n, void* stream);
/* the rule on its own, instance-free, no device needed: 1 = `win` at `pitch` is a valid placement of an entry of n plain bytes with
 * element size elem (*extent, when not NULL, becomes place_extent), 0 = it is not (pitch == 0 and row_bytes == 0 included) */
int zpk_codec_place_valid(uint64_t n, uint32_t elem, const zpk_window* win, uint64_t pitch, uint64_t* extent);
/* ... and the overlap rule of a valid placement: 1 = base == dst or the two ranges of place_extent bytes are disjoint */
int zpk_codec_place_overlap_ok(uint64_t base, uint64_t dst, const zpk_window* win, uint64_t pitch);
/* The two _windows reads with one more argument: pitch[i] is the pitch of entry i (HOST memory, n values).  pitch == NULL IS the
 * _windows call, the same body; pitch[i] == 0: entry i as that call treats it.  A non-zero pitch on an entry without a window, a
 * placement that is not valid against desc[i].uncomp_size and elem[i], or one with host destinations: ZPK_E_INVALID and nothing has
 * run.  A placed entry decodes into the codec's staging exactly as a windowed one does and is delivered through k_place_copy — even
 * where pitch == cols — under the rule of the _windows call: only when it decoded to all of uncomp_size and its base was accepted,
 * else no byte of its buffer is written.  For a placed entry the destination, the base and the pointer rule are about place_extent
 * bytes, and desc[i].dst_capacity is the room at the destination: with less than place_extent the entry is BUFFER_TOO_SMALL where the
 * guards, in their order, say so, and nothing is written.
 * BASE HASHES.  base_hash[i] is the XXH3 of a contiguous span, and the base of a placed entry is not one: a placed entry with a base in
 * a call whose base_hash is not NULL is ZPK_E_INVALID before anything runs — unless its extent equals its window bytes (rows <= 1 or
 * pitch == cols), which is checked as ever.  The caller hashes its whole merged base itself (zpk_codec_hash_spans_device;
 * zpack_amd_hash_device) and reads with base_hash NULL. */
int zpk_codec_decode_batch_host_dptr_placed(zpk_codec* c, const uint8_t* archive, uint64_t archive_size,
                                            const zpk_decode_desc* desc, uint64_t n,
                                            uint8_t* const* d_dst_ptrs, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base,
                                            const uint64_t* base_hash, const zpk_window* win, const uint64_t* pitch);
int zpk_codec_decode_batch_dimage_placed(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size,
                                         const zpk_decode_desc* desc, uint64_t n,
                                         uint8_t* const* dst_ptrs, int dst_on_device, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base,
                                         const uint64_t* base_hash, const zpk_window* win, const uint64_t* pitch);
/* the most recent of the three calls above (or of a call that could split, join or cut): out[0] rows placed, out[1] k_place_copy
 * launches.  zpk_codec_window_stats keeps its meaning: out[0] and out[1] count the rows of k_window_copy, which are the windowed rows
 * without a pitch; out[2] counts a placed entry that was staged only because it had a window as it counts any other. */
int zpk_codec_place_stats(zpk_codec* c, uint32_t out[2]);

/* zpk_codec_encode_batch_device for batches that hold LARGE entries: d_src, d_dst and d_results are DEVICE pointers, `desc` is HOST memory
 * (consumed before the call returns).  An entry with size >= ZPK_OPT_ENC_SPLIT_MIN, size > 512 KiB and a valid method is compressed as
 * 512 KiB pieces, one wave each, and its frame is assembled ON THE DEVICE: its slot d_dst + dst_offset and d_results[i] end up holding
 * exactly what zpk_codec_encode_batch_host writes for that entry (frame header, the pieces' blocks in order, the end of the frame;
 * ZPK_METHOD_NONE: the plain copy; status / detail of the first failing piece; a frame that does not fit dst_capacity is
 * COMPRESS_FAILED — BUFFER_TOO_SMALL for a stored entry; comp_size = hash = 0 on any failure), hash = XXH3-64 of the whole plaintext by
 * the whole chip.  Every other entry gets byte for byte what zpk_codec_encode_batch_device gives it.  Nothing outside an entry's
 * [dst_offset, dst_offset + dst_capacity) is written, whatever its verdict; a failed entry's slot may hold part of its blocks.
 * Work is enqueued on `stream` (NULL = the codec's own) and the call returns without waiting for it; the results compose with
 * zpk_codec_pack_batch_device unchanged (the caller uploads `desc` for it).  A third call in a row waits until the first one's tables
 * have gone up.  ZPK_E_INVALID: an entry's source or slot does not lie inside [0, src_size) / [0, dst_size).
 * SOURCE SLACK (this call and zpk_codec_encode_batch_device): the kernels load 16 bytes per lane.  The match finder, the literal
 * copies and the XXH3 passes take a narrower load or the last block again where 16 bytes would pass the end of an entry, but the
 * contract is that of the host path's staging: the allocation extends at least 16 bytes behind the last source byte of the batch. */
int zpk_codec_encode_big_device(zpk_codec* c, const uint8_t* d_src, uint64_t src_size,
                                const zpk_encode_desc* desc /* HOST memory */, uint64_t n,
                                uint8_t* d_dst, uint64_t dst_size,
                                zpk_encode_result* d_results /* DEVICE memory */, void* stream);
/* the most recent zpk_codec_encode_big_device call: out[0] = entries written in pieces, out[1] = their pieces; out[2..7] = 0.  Known when
 * the call is enqueued: does not synchronise. */
int zpk_codec_encode_stats(zpk_codec* c, uint32_t out[8]);

/* ---- compressed-size scan + compaction (the serial `write_offset += comp_size` of lib/zpack_write.c:338, for a batch)
 * After an encode batch: offsets[i] = start of entry i's payload in the packed stream (exclusive prefix sum of the
 * comp_size of the entries with status 0; failed entries take no room), offsets[n] = its total length; when `packed`
 * is not NULL the payloads are gathered there back-to-back from their slots (`slots` + desc[i].dst_offset), i.e. the
 * archive's data section in CDR order.  Device pointers, asynchronous on `stream`.  `max_entry_size` = an upper bound
 * of any comp_size (e.g. the largest dst_capacity); it only sizes the launch.  If packed_cap < offsets[n] the bytes
 * that do not fit are not written (check offsets[n]).
 * Pinned by tests/test_gpu_pack_alone.py (the call alone against numpy, `results` and `desc` written by the test):
 * SHORT BUFFER: `offsets` is the whole scan whatever packed_cap is — offsets[n] > packed_cap tells the caller.  No byte at or
 *   behind packed + packed_cap is written; every entry that ends at or in front of packed_cap is whole; of an entry that
 *   crosses it, each byte in front of packed_cap is either its payload's or untouched (whole 16 KiB spans of it are dropped,
 *   which ones is not promised).  Nothing behind packed + offsets[n] and nothing in front of `packed` is written; `slots`,
 *   `desc` and `results` are only read, and a failed entry's comp_size is never looked at.
 * ZPK_E_INVALID, twice: n > 2^31 - 1, judged before anything is allocated or enqueued; and, with `packed`,
 *   n * max(1, ceil(max_entry_size / 16384)) > 2^30 - 1 (the gather's launch would not fit): this one is found BEHIND the
 *   scans, which are already enqueued — `offsets` may be written, `packed` is not.
 * max_entry_size below a real comp_size: the launch has n * ceil(max_entry_size / 16384) waves for the batch's 16 KiB
 *   spans, counted through the batch in order; spans beyond that number — the tail of such an entry where it is the only
 *   one, otherwise the end of the batch — stay ungathered, without a diagnostic (offsets are right all the same).  A bound
 *   that is too large costs idle waves only.
 * NOT safe from two streams at once on one codec: the block sums and the span table are scratch of the codec's (d_pack),
 *   shared by every call; calls on ONE stream follow each other correctly. */
int zpk_codec_pack_batch_device(zpk_codec* c, const uint8_t* slots, const zpk_encode_desc* desc,
                                const zpk_encode_result* results, uint64_t n,
                                uint8_t* packed, uint64_t packed_cap, uint64_t* offsets,
                                uint64_t max_entry_size, void* stream);

/* ---- hash only ---------------------------------------------------------------------------- */
/* hashes[i] = XXH3_64bits(src + offsets[i], sizes[i]); device pointers, async on stream */
int zpk_codec_hash_batch_device(zpk_codec* c, const uint8_t* src, const uint64_t* offsets,
                                const uint64_t* sizes, uint64_t n, uint64_t* hashes, void* stream);
int zpk_codec_hash_host(zpk_codec* c, const uint8_t* data, uint64_t size, uint64_t* hash);

/* ---- timing helper for benchmarks: elapsed device time of everything enqueued between the two
 * marks on `stream`, measured with HIP events on that stream ------------------------------- */
/* per-kernel timing of decode batches: when enabled, every decode batch brackets each of its kernels
 * with HIP events on the launch stream; zpk_codec_kernel_ms then returns the duration of kernel
 * `which` (ZPK_K_*) in the most recent batch (synchronises on that batch). */
enum { ZPK_K_CLASSIFY = 0, ZPK_K_STORED = 1, ZPK_K_LZ4 = 2 /* k_lz4_wave (plain frames) + k_lz4_left + k_lz4_general + k_lz4_retry */, ZPK_K_ZSTD = 3 /* k_zstd_exec + k_zstd */, ZPK_K_ZSTD_FSE = 4,
       ZPK_K_PACK = 5, ZPK_K_RESERVED6 = 6 /* (was k_lz4_parse) */, ZPK_K_ENCODE = 7, ZPK_K_COUNT = 8 };
int zpk_codec_set_profiling(zpk_codec* c, int enabled);
/* out[0], out[1] = LZ4 / Zstandard entries of the most recent decode batch whose first decode ran out of its time budget (a
 * contended or preempted GPU) and that were decoded again, behind the batch, with a 64 x larger one — a slow wave is not a
 * verdict; expected 0 on an idle GPU.  out[3] = LZ4 entries that are mostly runs (compressed to less than 1/8: the classification puts
 * them on the list of k_lz4_left, the build of the one-wave decoder with grouped cooperative copies); out[2] = out[4] = 0; out[5], out[6] = entries of the most recent
 * zpk_codec_decode_batch_host call that were decoded frame-parallel (ZPK_OPT_DEC_SPLIT_MIN) and the frames they had;
 * out[8] = LZ4 entries with the header of a plain frame (one frame, no checksums, no dictionary id) that k_lz4_wave, the kernel for such
 * frames, did not finish cleanly and handed unjudged to the general decoder behind it (damaged, truncated, trailing bytes ...; not part
 * of out[0]); out[9] = LZ4 entries whose header is not that of a plain frame: the classification sends them to k_lz4_general;
 * out[10], out[11] = entries of the most recent zpk_codec_decode_big_batch_device call walked on the device / those the walk accepted;
 * out[12], out[13] = stored entries the most recent zpk_codec_decode_big_batch_device / zpk_codec_decode_big_device call copied chip-wide
 * (ZPK_OPT_STORED_SPAN_MIN) / their groups of 64 KiB;
 * out[14] = sub-batches of the most recent zpk_codec_decode_batch_host / _dptr call that took the three-stage pipeline; out[15] = k_span_copy
 * launches of the most recent zpk_codec_decode_batch_host_dptr call.
 * The indices by name (added within ABI 3; the numbers are the ones above and do not move): */
enum { ZPK_DS2_RETRY_LZ4 = 0, ZPK_DS2_RETRY_ZSTD = 1, ZPK_DS2_RESERVED2 = 2 /* reads 0 */, ZPK_DS2_LZ4_RUNS = 3, ZPK_DS2_RESERVED4 = 4 /* reads 0 */,
       ZPK_DS2_BIG_ENTRIES = 5, ZPK_DS2_BIG_FRAMES = 6, ZPK_DS2_ZPJ_ERR = 7 /* developer: why the most recent large Zstandard frame was not finished block-parallel (0: it was, or none came) */,
       ZPK_DS2_LZ4_HANDED = 8, ZPK_DS2_LZ4_GEN = 9, ZPK_DS2_WALKED = 10, ZPK_DS2_WALK_ACCEPTED = 11, ZPK_DS2_SPAN_ENTRIES = 12, ZPK_DS2_SPAN_GROUPS = 13,
       ZPK_DS2_PIPE_SUBS = 14, ZPK_DS2_SPAN_COPIES = 15, ZPK_DS2_COUNT = 16 };
int zpk_codec_decode_stats2(zpk_codec* c, uint32_t out[16]);
/* counters of the most recent decode batch (synchronises): out[0..2] = entries on the stored / zstd / lz4 work
 * lists, out[3] = Zstandard entries finished on pre-decoded sequences (two-stage path), out[4] = by the fused decoder,
 * out[5], out[6] = entries / waves the pre-decode kernel gave up on (watchdog; expected 0) */
int zpk_codec_decode_stats(zpk_codec* c, uint32_t out[8]);
int zpk_codec_debug_read(zpk_codec* c, void* host, uint64_t bytes);   /* developer aid: phase timing words */
/* developer aid: read back the Zstandard pre-decode arena (what 0) / per-entry marks (what 1) of the last batch */
int zpk_codec_debug_fetch(zpk_codec* c, int what, uint64_t offset, void* host, uint64_t bytes);
int zpk_codec_kernel_ms(zpk_codec* c, int which, float* ms);
int zpk_codec_timer_start(zpk_codec* c, void* stream);
int zpk_codec_timer_stop(zpk_codec* c, void* stream, float* elapsed_ms);   /* synchronises the stop event */

/* ---- streaming triple (lib/zpack_read.c:515-640, lib/zpack_write.c:461-685) ------------------
 * Chunk granularity is hostile to the GPU, so a stream GATHERS small chunks on the host (256 KiB) before it steps the device:
 * every step decodes all complete blocks the bytes so far hold (resumable) and the output is handed out in avail_out-sized
 * pieces while more input arrives.  Same observable protocol as the reference (total_in/total_out/read_back). */
typedef struct zpk_dstream zpk_dstream;
int  zpk_dstream_create(zpk_codec* c, zpk_dstream** out);
void zpk_dstream_bind(zpk_dstream* s, zpk_codec* c);     /* the codec the NEXT step decodes with (a stream may outlive codecs) */
void zpk_dstream_reset(zpk_dstream* s);
void zpk_dstream_destroy(zpk_dstream* s);
/* feed in_size bytes, receive up to out_cap bytes; *consumed / *produced report progress;
 * entry_* describe the entry being streamed; *done = 1 once every output byte has been delivered and
 * the hash verified.  Returns an enum zpack_result code. */
int  zpk_dstream_step(zpk_dstream* s, uint32_t method, uint64_t entry_comp_size, uint64_t entry_uncomp_size,
                      uint64_t entry_hash, const uint8_t* in, size_t in_size, size_t* consumed,
                      uint8_t* out, size_t out_cap, size_t* produced, int* done);

/* Bounded memory (round 5): a large entry that is one plain LZ4 frame is decoded in block-parallel steps and the stream holds only a window
 * of it.  zpk_dstream_wants_input() == 0: the stream has output waiting and takes no input — call zpk_dstream_step with in_size 0.
 * zpk_dstream_step may answer ZPK_DS_RESTART (not a zpack_result): the entry is not what the steps can decide; feed the entry's bytes
 * [0, bytes given so far) again through zpk_dstream_replay (first = 1 with the first piece) and go on with zpk_dstream_step: the
 * stream continues in its windowless form, where the verdicts are; nothing is handed out twice. */
#define ZPK_DS_RESTART 1001
int  zpk_dstream_wants_input(const zpk_dstream* s);
int  zpk_dstream_replay(zpk_dstream* s, uint32_t method, uint64_t entry_comp_size, uint64_t entry_uncomp_size, uint64_t entry_hash,
                        const uint8_t* in, size_t in_size, int first);

/* diagnostics: device decode steps launched / calls served since the stream's last reset (small chunks are gathered on the host: at
 * most one launch per 256 KiB of input) */
void zpk_dstream_counters(const zpk_dstream* s, uint64_t* launches, uint64_t* calls);
uint64_t zpk_dstream_device_bytes(const zpk_dstream* s);   /* diagnostics: device memory the stream holds right now */

typedef struct zpk_cstream zpk_cstream;
int  zpk_cstream_create(zpk_codec* c, zpk_cstream** out);
void zpk_cstream_bind(zpk_cstream* s, zpk_codec* c);
void zpk_cstream_reset(zpk_cstream* s);
void zpk_cstream_destroy(zpk_cstream* s);
/* method + level of the entry about to be streamed (before its first update): from then on zpk_cstream_update compresses as the
 * plaintext arrives — every complete 512 KiB piece becomes a frame of its own, handed out by zpk_cstream_drain — and the device
 * holds a few MiB of plaintext at most.  Without it update only collects and zpk_cstream_finish compresses everything. */
int  zpk_cstream_configure(zpk_cstream* s, uint32_t method, int32_t level);
int  zpk_cstream_update(zpk_cstream* s, const uint8_t* in, size_t in_size);       /* plaintext in; may make output available */
/* compress what is left; *comp_size = all compressed bytes of the entry (handed out already or still to drain), *hash = XXH3-64 of the
 * whole plaintext; the remaining bytes are then drained with zpk_cstream_drain */
int  zpk_cstream_finish(zpk_cstream* s, uint32_t method, int32_t level, uint64_t* comp_size,
                        uint64_t* uncomp_size, uint64_t* hash);
size_t zpk_cstream_drain(zpk_cstream* s, uint8_t* out, size_t out_cap);           /* returns bytes copied */

#ifdef __cplusplus
}
#endif
#endif /* ZPACK_CODEC_H */
