/* writer.c — archive writer of the zpack.h API.
 *
 * Container emission (header, data signature, CDR, EOCDR) is host code following docs/specs.md like the
 * reference writer (lib/zpack_write.c:60-123, :687-829).  The hot path — zpack_compress_file +
 * the XXH3 of zpack_add_written_file_entry (lib/zpack_write.c:161-260), looped per file at :287-339 —
 * is ONE batched call into the GPU codec (zpk_codec_encode_batch_host); the serial
 * `write_offset += comp_size` of :338 becomes a prefix sum over the batch's compressed sizes.
 */
#include "internal.h"
#include "zpack_amd.h"
#include <pthread.h>
#include <stdint.h>

/* ------------------------------------------------------------------ sink + entry table */

static zpack_u64 pow2_at_least(zpack_u64 n) { zpack_u64 b = 1; while (b < n) b <<= 1; return b; }

/* zpack_amd.h: a writer whose sink is an image in DEVICE memory.  zpack_writer has the reference's fixed layout, so where the image lives
 * is kept beside the writer, in the writers' side table (internal.h; as the readers' records are: readahead.c). */
static zi_side_table g_writers = ZI_SIDE_TABLE_INIT;      /* image: the sink; word: its capacity */

int zi_writer_dsink_set(const zpack_writer* w, void* d_image, size_t capacity, int device)
{
    const zi_side_rec r = { d_image, capacity, device };
    return zi_side_set(&g_writers, w, &r);                /* (a record left at this address: replaced) */
}

void zi_writer_dsink_drop(const zpack_writer* w) { zi_side_drop(&g_writers, w); }

zi_sink zi_writer_sink(const zpack_writer* w, zpack_u8** d_image, size_t* capacity, int* device)
{
    if (d_image) *d_image = NULL;
    if (capacity) *capacity = 0;
    if (device) *device = -1;
    if (w->file) return ZI_SINK_FILE;
    if (w->buffer) return ZI_SINK_HEAP;
    zi_side_rec r;
    /* (a zeroed struct at the address of a writer that was never closed: not this record's) */
    if (!zi_side_find(&g_writers, w, &r) || r.word != (zpack_u64)w->buffer_capacity) return ZI_SINK_NONE;
    if (d_image) *d_image = (zpack_u8*)r.image;
    if (capacity) *capacity = (size_t)r.word;
    if (device) *device = r.device;
    return ZI_SINK_DEVICE;
}

/* append `size` bytes at the writer's cursor: file (seek + write), heap (power-of-two growth, like lib/zpack_common.c:83-104) or an
 * image in device memory (a room check, then zpk_codec_store_device: the sink does not grow) */
int zi_writer_put(zpack_writer* w, const zpack_u8* data, size_t size)
{
    if (w->file) {
        if (zi_fseek(w->file, w->write_offset, SEEK_SET) != 0) return ZPACK_ERROR_SEEK_FAILED;
        if (size && fwrite(data, 1, size, w->file) != size) return ZPACK_ERROR_WRITE_FAILED;
    } else if (w->buffer) {
        const zpack_u64 need = (zpack_u64)w->file_size + size;
        if ((zpack_u64)w->buffer_capacity < need) {
            const zpack_u64 cap = pow2_at_least(need);
            if (cap > SIZE_MAX) return ZPACK_ERROR_MALLOC_FAILED;
            zpack_u8* nb = (zpack_u8*)realloc(w->buffer, (size_t)cap);
            if (!nb) return ZPACK_ERROR_MALLOC_FAILED;
            w->buffer = nb; w->buffer_capacity = (size_t)cap;
        }
        if (size) memcpy(w->buffer + w->write_offset, data, size);
    } else {
        zpack_u8* d_image; size_t capacity;
        if (zi_writer_sink(w, &d_image, &capacity, NULL) != ZI_SINK_DEVICE) return ZPACK_ERROR_WRITER_NOT_OPENED;
        if (w->write_offset > capacity || size > capacity - w->write_offset) return ZPACK_ERROR_BUFFER_TOO_SMALL;
        if (zpk_codec_store_device(d_image + w->write_offset, data, size) != ZPK_OK) return ZPACK_ERROR_WRITE_FAILED;
    }
    w->write_offset += size;
    w->file_size += size;
    return ZPACK_OK;
}

zpack_file_entry* zi_writer_push_entry(zpack_writer* w)
{
    if (w->file_count + 1 > w->fe_capacity) {
        const zpack_u64 cap = pow2_at_least(w->file_count + 1);
        if (cap > SIZE_MAX / sizeof(zpack_file_entry)) return NULL;
        zpack_file_entry* t = (zpack_file_entry*)realloc(w->file_entries, sizeof(zpack_file_entry) * (size_t)cap);
        if (!t) return NULL;
        w->file_entries = t; w->fe_capacity = cap;
    }
    zpack_file_entry* e = w->file_entries + w->file_count++;
    memset(e, 0, sizeof(*e));
    return e;
}

int zi_writer_enter(zpack_writer* w, const char* name, zpack_u64 offset, zpack_u64 comp_size, zpack_u64 uncomp_size, zpack_u64 hash, zpack_u8 method)
{
    zpack_file_entry* e = zi_writer_push_entry(w);
    if (!e) return ZPACK_ERROR_MALLOC_FAILED;
    const size_t n = strlen(name) + 1;
    if (!(e->filename = (char*)malloc(n))) return ZPACK_ERROR_MALLOC_FAILED;
    memcpy(e->filename, name, n);
    e->offset = offset;
    e->comp_size = comp_size;
    e->uncomp_size = uncomp_size;
    e->hash = hash;                                           /* XXH3-64 of the plaintext, lib/zpack_write.c:256 */
    e->comp_method = method;
    return ZPACK_OK;
}
/* ... a raw copy of `src` whose payload went to `offset` */
static int writer_enter_copy(zpack_writer* w, const zpack_file_entry* src, zpack_u64 offset)
{
    return zi_writer_enter(w, src->filename, offset, src->comp_size, src->uncomp_size, src->hash, src->comp_method);
}
/* `bytes` that reached a device image without zi_writer_put (a codec call placed them): the cursor moves on; returns where they begin */
static zpack_u64 writer_placed(zpack_writer* w, zpack_u64 bytes)
{
    const zpack_u64 at = w->write_offset;
    w->write_offset += (size_t)bytes;
    w->file_size += (size_t)bytes;
    return at;
}

/* ------------------------------------------------------------------ open */

int zpack_init_writer(zpack_writer* writer, const char* path)
{
    zi_writer_dsink_drop(writer);                         /* (a device-sink record left at this address by a writer that was never closed) */
    writer->file = fopen(path, "wb");
    return writer->file ? ZPACK_OK : ZPACK_ERROR_OPEN_FAILED;
}

int zpack_init_writer_cfile(zpack_writer* writer, FILE* fp)
{
    if (!fp) return ZPACK_ERROR_OPEN_FAILED;
    zi_writer_dsink_drop(writer);
    writer->file = fp;
    return ZPACK_OK;
}

int zpack_init_writer_heap(zpack_writer* writer, size_t initial_size)
{
    const size_t least = ZPACK_HEADER_SIZE + ZPACK_SIGNATURE_SIZE;
    zi_writer_dsink_drop(writer);
    writer->buffer_capacity = initial_size > least ? initial_size : least;
    writer->buffer = (zpack_u8*)malloc(writer->buffer_capacity);
    return writer->buffer ? ZPACK_OK : ZPACK_ERROR_MALLOC_FAILED;
}

int zpack_amd_init_writer_device(zpack_writer* writer, void* d_image, size_t capacity)
{
    if (!writer || !d_image) return ZPACK_ERROR_STREAM_INVALID;
    if (zpk_codec_device_count() <= 0) return ZPACK_ERROR_NOT_AVAILABLE;           /* no HIP device: there is no CPU fallback */
    /* the whole range is checked against its allocation before anything is touched */
    const int device = zpk_codec_pointer_device(d_image);
    if (device < 0 || zpk_codec_store_device(d_image, NULL, capacity) != ZPK_OK) return ZPACK_ERROR_STREAM_INVALID;
    if (!zi_writer_dsink_set(writer, d_image, capacity, device)) return ZPACK_ERROR_MALLOC_FAILED;
    writer->buffer = NULL; writer->file = NULL;
    writer->buffer_capacity = capacity;                                            /* (what zi_writer_sink knows the record by) */
    return ZPACK_OK;
}

int zpack_amd_writer_device_image(const zpack_writer* writer, void** d_image, size_t* capacity, int* device)
{
    if (!writer) return ZPACK_ERROR_STREAM_INVALID;
    zpack_u8* p = NULL; size_t cap = 0; int dev = -1;
    if (zi_writer_sink(writer, &p, &cap, &dev) != ZI_SINK_DEVICE) { p = NULL; cap = 0; dev = -1; }
    if (d_image) *d_image = p;
    if (capacity) *capacity = cap;
    if (device) *device = dev;
    return ZPACK_OK;
}

/* ------------------------------------------------------------------ fixed blocks */

int zpack_write_header_ex(zpack_writer* writer, zpack_u16 version)
{
    zpack_u8 b[ZPACK_HEADER_SIZE];
    zi_put32(b, ZPACK_HEADER_SIGNATURE);
    zi_put16(b + 4, version);
    return zi_writer_put(writer, b, sizeof(b));
}

int zpack_write_header(zpack_writer* writer) { return zpack_write_header_ex(writer, ZPACK_ARCHIVE_VERSION_MAX); }

int zpack_write_data_header(zpack_writer* writer)
{
    zpack_u8 b[ZPACK_SIGNATURE_SIZE];
    zi_put32(b, ZPACK_DATA_SIGNATURE);
    return zi_writer_put(writer, b, sizeof(b));
}

int zpack_write_cdr_ex(zpack_writer* writer, zpack_file_entry* entries, zpack_u64 file_count)
{
    if (zi_writer_sink(writer, NULL, NULL, NULL) == ZI_SINK_NONE) return ZPACK_ERROR_WRITER_NOT_OPENED;
    zpack_u64 block = 0;
    for (zpack_u64 i = 0; i < file_count; i++) {
        const size_t n = strlen(entries[i].filename);
        if (n > ZPACK_MAX_FILENAME_LENGTH) return ZPACK_ERROR_FILENAME_TOO_LONG;
        block += ZPACK_FILE_ENTRY_FIXED_SIZE + n;
    }
    const zpack_u64 total = ZPACK_CDR_HEADER_SIZE + block;
    if (total > SIZE_MAX) return ZPACK_ERROR_MALLOC_FAILED;
    zpack_u8* img = (zpack_u8*)malloc((size_t)total);
    if (!img) return ZPACK_ERROR_MALLOC_FAILED;
    zi_put32(img, ZPACK_CDR_SIGNATURE);
    zi_put64(img + 4, file_count);
    zi_put64(img + 12, block);
    zpack_u8* p = img + ZPACK_CDR_HEADER_SIZE;
    for (zpack_u64 i = 0; i < file_count; i++) {
        const zpack_file_entry* e = entries + i;
        const zpack_u16 n = (zpack_u16)strlen(e->filename);
        zi_put16(p, n); memcpy(p + 2, e->filename, n); p += 2 + n;
        zi_put64(p, e->offset); zi_put64(p + 8, e->comp_size); zi_put64(p + 16, e->uncomp_size); zi_put64(p + 24, e->hash);
        p[32] = e->comp_method;
        p += 33;
    }
    const zpack_u64 at = writer->write_offset;
    int rc = zi_writer_put(writer, img, (size_t)total);
    free(img);
    if (rc == ZPACK_OK) writer->cdr_offset = at;
    return rc;
}

int zpack_write_cdr(zpack_writer* writer) { return zpack_write_cdr_ex(writer, writer->file_entries, writer->file_count); }

int zpack_write_eocdr_ex(zpack_writer* writer, zpack_u64 cdr_offset)
{
    zpack_u8 b[ZPACK_EOCDR_SIZE];
    zi_put32(b, ZPACK_EOCDR_SIGNATURE);
    zi_put64(b + 4, cdr_offset);
    const zpack_u64 at = writer->write_offset;
    int rc = zi_writer_put(writer, b, sizeof(b));
    if (rc == ZPACK_OK) writer->eocdr_offset = at;
    return rc;
}

int zpack_write_eocdr(zpack_writer* writer) { return zpack_write_eocdr_ex(writer, writer->cdr_offset); }

/* ------------------------------------------------------------------ the hot path: compress + hash */

typedef struct {
    zi_ctx* ctx; const zpack_u8* const* srcs; const zpk_encode_desc* desc; zpack_u8* const* dsts; zpk_encode_result* res;
    zpack_u64 cut[ZI_MAX_DEVICES + 1]; int rc[ZI_MAX_DEVICES];
} write_job;

static void write_part(void* arg, int k)
{
    write_job* j = (write_job*)arg;
    const zpack_u64 lo = j->cut[k], n = j->cut[k + 1] - lo;
    j->rc[k] = n ? zpk_codec_encode_batch_host(j->ctx->dev[k], j->srcs + lo, j->desc + lo, n, j->dsts + lo, j->res + lo) : ZPK_OK;
}

static zpack_u64 file_weight(const void* files, zpack_u64 i) { return ((const zpack_file*)files)[i].size; }

/* The sink is an image in DEVICE memory: ONE zpk_codec_encode_batch_dsink call on the codec of the sink's device, no shard — the frames
 * are committed to the image on the device under the append rule below (the files in front of the first failing one, where "does not
 * fit" fails too), and only the results and the cut come home: no scratch of compress-bound size on the host. */
static int write_files_dsink(zpack_writer* writer, zi_ctx* ctx, zpack_file* files, zpack_u64 file_count, int on_device,
                             const zpack_u8* const* srcs, const zpk_encode_desc* desc, zpk_encode_result* res, const zpack_u8* elem,
                             const zpack_u8* const* bases)
{
    zpack_u8* d_image; size_t capacity; int device;
    if (zi_writer_sink(writer, &d_image, &capacity, &device) != ZI_SINK_DEVICE) return ZPACK_ERROR_WRITER_NOT_OPENED;
    zpk_codec* codec = zi_ctx_codec_on(ctx, device);
    if (!codec) return ZPACK_ERROR_NOT_AVAILABLE;                                  /* the sink's device is not one of the context's */
    if (on_device) {                                                               /* device plaintext lies on the sink's device */
        int rc = ZPACK_OK;
        zpk_codec* of = zi_ctx_codec_of(ctx, &files[0].buffer, sizeof(files[0]), &files[0].size, sizeof(files[0]), 1, file_count, &rc);
        if (rc == ZPACK_ERROR_NOT_AVAILABLE || (of && zpk_codec_device(of) != device)) return ZPACK_ERROR_STREAM_INVALID;
        if (rc != ZPACK_OK) return rc;
    }
    const zpack_u64 at0 = writer->write_offset;
    const zpack_u64 room = at0 < capacity ? capacity - at0 : 0;
    uint64_t placed = 0, bytes = 0;
    const int crc = zpk_codec_encode_batch_dsink_delta(codec, srcs, on_device, desc, file_count, d_image + (at0 < capacity ? at0 : capacity), room, res, &placed, &bytes, elem, bases);
    if (crc != ZPK_OK) return zi_rc_of_codec(crc);
    for (zpack_u64 i = 0; i < placed; i++) {                                       /* entered as the loop below enters them: at the running sum */
        writer->last_return = (size_t)res[i].comp_size;
        const zpack_u64 at = writer_placed(writer, res[i].comp_size);
        if (zi_writer_enter(writer, files[i].filename, at, res[i].comp_size, files[i].size, res[i].hash, (zpack_u8)files[i].options->method)) return ZPACK_ERROR_MALLOC_FAILED;
    }
    if (placed == file_count) return ZPACK_OK;
    /* the file that stopped the call: its own status, else it did not fit what is left of the image */
    writer->last_return = res[placed].status ? (size_t)0 - res[placed].detail : (size_t)res[placed].comp_size;
    return res[placed].status ? res[placed].status : ZPACK_ERROR_BUFFER_TOO_SMALL;
}

/* on_device: files[i].buffer are DEVICE pointers (zpack_amd_write_files_device) — the plaintext is compressed where it lies, only the
 * compressed bytes cross the bus: one zpk_codec_encode_batch_dsrc call on the codec of the pointers' device (no shard: one call's
 * pointers belong to one device).  Everything behind the codec call is the same code, so the archive is the same bytes.
 * elem (on_device only, else NULL): the files' element sizes — the codec splits the byte planes on the way into its staging.
 * bases (likewise): the files' bases in device memory, NULL for a file that has none — the codec XORs them in on the same way */
static int write_files(zpack_writer* writer, zpack_file* files, zpack_u64 file_count, int on_device, const zpack_u8* elem,
                       const zpack_u8* const* bases)
{
    if (file_count == 0) return ZPACK_OK;
    const zi_sink sink = zi_writer_sink(writer, NULL, NULL, NULL);
    if (sink == ZI_SINK_NONE) return ZPACK_ERROR_WRITER_NOT_OPENED;
    /* contexts: a per-file cctx is honoured when every file names the same one, else the writer's own */
    void* explicit_ctx = files[0].cctx;
    for (zpack_u64 i = 1; i < file_count; i++) if (files[i].cctx != explicit_ctx) explicit_ctx = NULL;
    zi_ctx* ctx = zi_pick_ctx(explicit_ctx, &writer->zstd_cctx);     /* lib/zpack_write.c:20-34: the writer's own, created on first use */
    if (!ctx) return ZPACK_ERROR_NOT_AVAILABLE;              /* no HIP device: there is no CPU fallback */

    zpk_encode_desc* desc = (zpk_encode_desc*)calloc((size_t)file_count, sizeof(*desc));
    zpk_encode_result* res = (zpk_encode_result*)calloc((size_t)file_count, sizeof(*res));
    const zpack_u8** srcs = (const zpack_u8**)calloc((size_t)file_count, sizeof(*srcs));
    zpack_u8** dsts = sink == ZI_SINK_DEVICE ? NULL : (zpack_u8**)calloc((size_t)file_count, sizeof(*dsts));
    int rc = (desc && res && srcs && (dsts || sink == ZI_SINK_DEVICE)) ? ZPACK_OK : ZPACK_ERROR_MALLOC_FAILED;
    zpack_u64 slots = 0;
    for (zpack_u64 i = 0; i < file_count && rc == ZPACK_OK; i++) {
        const zpack_compression_method m = files[i].options->method;
        if (m != ZPACK_COMPRESSION_NONE && m != ZPACK_COMPRESSION_ZSTD && m != ZPACK_COMPRESSION_LZ4) rc = ZPACK_ERROR_COMP_METHOD_INVALID;
        desc[i].size = files[i].size;
        desc[i].method = (uint32_t)m;
        desc[i].level = files[i].options->level;
        desc[i].dst_capacity = zpk_codec_compress_bound((uint32_t)m, (size_t)files[i].size);     /* lib/zpack_write.c:125-150 */
        slots += desc[i].dst_capacity + 16;
        srcs[i] = files[i].buffer;
    }
    if (sink == ZI_SINK_DEVICE) {
        if (rc == ZPACK_OK) rc = write_files_dsink(writer, ctx, files, file_count, on_device, srcs, desc, res, elem, bases);
        free(desc); free(res); free(srcs);
        return rc;
    }
    zpack_u8* scratch = NULL;
    if (rc == ZPACK_OK) {
        scratch = (zpack_u8*)malloc((size_t)slots ? (size_t)slots : 1);
        if (!scratch) rc = ZPACK_ERROR_MALLOC_FAILED;
    }
    if (rc == ZPACK_OK) {
        zpack_u64 pos = 0;
        for (zpack_u64 i = 0; i < file_count; i++) { dsts[i] = scratch + pos; pos += desc[i].dst_capacity + 16; }
    }
    if (rc == ZPACK_OK && on_device) {
        zpk_codec* codec = zi_ctx_codec_of(ctx, &files[0].buffer, sizeof(files[0]), &files[0].size, sizeof(files[0]), 1, file_count, &rc);
        if (!codec && rc == ZPACK_OK) codec = ctx->dev[0];                           /* (nothing has bytes: empty entries only) */
        if (codec) rc = zi_rc_of_codec(zpk_codec_encode_batch_dsrc_delta(codec, srcs, desc, file_count, dsts, res, elem, bases));
    } else if (rc == ZPACK_OK) {
        write_job job = { ctx, srcs, desc, dsts, res, {0}, {0} };
        /* static shard by source bytes: one host thread + one codec per device */
        const int parts = zi_shard(ctx, file_count, file_weight, files, job.cut);
        zi_parallel(parts, write_part, &job);
        for (int k = 0; k < parts; k++) if (job.rc[k] != ZPK_OK) rc = ZPACK_ERROR_NOT_AVAILABLE;
    }
    /* append in order; the first failing file stops the call like the reference loop does (:299-303) */
    for (zpack_u64 i = 0; i < file_count && rc == ZPACK_OK; i++) {
        writer->last_return = res[i].status ? (size_t)0 - res[i].detail : (size_t)res[i].comp_size;
        if (res[i].status != ZPACK_OK) { rc = res[i].status; break; }
        const zpack_u64 at = writer->write_offset;
        if ((rc = zi_writer_put(writer, dsts[i], (size_t)res[i].comp_size))) break;
        if ((rc = zi_writer_enter(writer, files[i].filename, at, res[i].comp_size, files[i].size, res[i].hash, (zpack_u8)files[i].options->method))) break;
    }
    free(scratch); free(desc); free(res); free(srcs); free(dsts);
    return rc;
}

int zpack_write_files(zpack_writer* writer, zpack_file* files, zpack_u64 file_count) { return write_files(writer, files, file_count, 0, NULL, NULL); }

/* DELTA entries: file i is stored as split(plain XOR d_bases[i]); d_bases NULL is the byte-plane call, the same code */
int zpack_amd_write_files_device_delta(zpack_writer* writer, zpack_file* files, zpack_u64 file_count, const zpack_u8* elem_sizes,
                                       const void* const* d_bases)
{
    if (!writer || (file_count && !files)) return ZPACK_ERROR_STREAM_INVALID;
    for (zpack_u64 i = 0; i < file_count; i++) if (!files[i].options || !files[i].filename) return ZPACK_ERROR_STREAM_INVALID;
    if (!zi_elem_sizes_valid(elem_sizes, file_count)) return ZPACK_ERROR_STREAM_INVALID;    /* before any context is created */
    if (zpk_codec_device_count() <= 0) return ZPACK_ERROR_NOT_AVAILABLE;           /* no HIP device: there is no CPU fallback */
    return write_files(writer, files, file_count, 1, elem_sizes, (const zpack_u8* const*)d_bases);
}

int zpack_amd_write_files_device_planes(zpack_writer* writer, zpack_file* files, zpack_u64 file_count, const zpack_u8* elem_sizes)
{
    return zpack_amd_write_files_device_delta(writer, files, file_count, elem_sizes, NULL);
}

int zpack_amd_write_files_device(zpack_writer* writer, zpack_file* files, zpack_u64 file_count)
{
    return zpack_amd_write_files_device_planes(writer, files, file_count, NULL);
}

/* ... from an image in device memory to an image in device memory ON THE SAME DEVICE: the payloads never leave it.  The loop below, in
 * two passes: the entries that pass its guards and fit the image, in order, are rows of ONE zpk_codec_copy_spans_device launch; then they
 * are entered.  *rc = what the first entry that stops the loop returns.  0: no codec of the writer's context is on that device, the
 * caller copies through the host. */
static int from_archive_on_device(zpack_writer* writer, const zpack_reader* reader, const zpack_u8* d_src, zpack_u8* d_image, size_t capacity, int device,
                                  const zpack_file_entry* entries, zpack_u64 file_count, int* rc)
{
    zi_ctx* ctx = zi_pick_ctx(NULL, &writer->zstd_cctx);
    zpk_codec* codec = ctx ? zi_ctx_codec_on(ctx, device) : NULL;
    if (!codec) return 0;
    zpk_span_copy* rows = (zpk_span_copy*)malloc(sizeof(*rows) * (size_t)(file_count ? file_count : 1));
    if (!rows) { *rc = ZPACK_ERROR_MALLOC_FAILED; return 1; }
    zpack_u64 k = 0, at = writer->write_offset;
    *rc = ZPACK_OK;
    for (; k < file_count; k++) {
        const zpack_file_entry* src = entries + k;
        if (!zi_entry_in_image(src, reader->file_size)) { *rc = ZPACK_ERROR_FILE_OFFSET_INVALID; break; }
        if (at > capacity || src->comp_size > capacity - at) { *rc = ZPACK_ERROR_BUFFER_TOO_SMALL; break; }
        rows[k].src = (uint64_t)(uintptr_t)(d_src + src->offset); rows[k].dst = (uint64_t)(uintptr_t)(d_image + at); rows[k].len = src->comp_size;
        at += src->comp_size;
    }
    if (k && (zpk_codec_copy_spans_device(codec, rows, k, NULL) != ZPK_OK || zpk_codec_stream_sync(codec) != ZPK_OK)) { free(rows); *rc = ZPACK_ERROR_WRITE_FAILED; return 1; }
    free(rows);
    for (zpack_u64 i = 0; i < k; i++)
        if (writer_enter_copy(writer, entries + i, writer_placed(writer, entries[i].comp_size))) { *rc = ZPACK_ERROR_MALLOC_FAILED; return 1; }
    return 1;
}

/* raw entry copy between archives: no codec involved (lib/zpack_write.c:345-428) */
int zpack_write_files_from_archive(zpack_writer* writer, zpack_reader* reader, zpack_file_entry* entries, zpack_u64 file_count)
{
    zpack_u8* d_sink; size_t sink_capacity; int sink_device;
    if (zi_writer_sink(writer, &d_sink, &sink_capacity, &sink_device) == ZI_SINK_NONE) return ZPACK_ERROR_WRITER_NOT_OPENED;
    zpack_u8* tmp = NULL; size_t tmp_cap = 0;
    int rc = ZPACK_OK;
    const zpack_u8* d_from; int from_device;
    const zi_source from = zi_reader_source(reader, &d_from, &from_device);
    if (d_sink && from == ZI_SRC_DEVICE && from_device == sink_device &&
        from_archive_on_device(writer, reader, d_from, d_sink, sink_capacity, sink_device, entries, file_count, &rc)) return rc;
    for (zpack_u64 i = 0; i < file_count && rc == ZPACK_OK; i++) {
        const zpack_file_entry* src = entries + i;
        const zpack_u8* payload = NULL;
        if (from == ZI_SRC_FILE || from == ZI_SRC_DEVICE) {
            /* (an image in device memory: the guard of the host image below, then the payload comes home through zpack_read_raw_file) */
            if (from == ZI_SRC_DEVICE && !zi_entry_in_image(src, reader->file_size)) { rc = ZPACK_ERROR_FILE_OFFSET_INVALID; break; }
            if (src->comp_size > SIZE_MAX) { rc = ZPACK_ERROR_MALLOC_FAILED; break; }
            if (tmp_cap < src->comp_size) {
                zpack_u8* nb = (zpack_u8*)realloc(tmp, (size_t)src->comp_size);
                if (!nb) { rc = ZPACK_ERROR_MALLOC_FAILED; break; }
                tmp = nb; tmp_cap = (size_t)src->comp_size;
            }
            if ((rc = zpack_read_raw_file(reader, (zpack_file_entry*)src, tmp, tmp_cap))) break;
            payload = tmp;
        } else if (reader->buffer) {
            if (!zi_entry_in_image(src, reader->file_size)) { rc = ZPACK_ERROR_FILE_OFFSET_INVALID; break; }
            payload = reader->buffer + src->offset;
        } else { rc = ZPACK_ERROR_ARCHIVE_NOT_LOADED; break; }
        const zpack_u64 at = writer->write_offset;
        if ((rc = zi_writer_put(writer, payload, (size_t)src->comp_size))) break;
        if ((rc = writer_enter_copy(writer, src, at))) break;
    }
    free(tmp);
    return rc;
}

/* streaming write (lib/zpack_write.c:461-685): the plaintext goes to the device chunk by chunk and is compressed there as it comes —
 * every call hands what has been compressed so far to the archive through the caller's output window, as the reference does with
 * its library buffers (:541-571); the entry is one frame, its blocks compressed piece by piece (zpk_stream.inc). */
static int stream_drain(zpack_writer* writer, zpack_stream* stream, zi_stream_state* st)
{
    for (;;) {
        size_t n = zpk_cstream_drain(st->c, stream->next_out, stream->avail_out);
        if (n == 0) return ZPACK_OK;
        int rc = zi_writer_put(writer, stream->next_out, n);
        if (rc) return rc;
        stream->total_out += n;
    }
}

int zpack_write_file_stream(zpack_writer* writer, zpack_compress_options* options, zpack_stream* stream, void* cctx)
{
    if (!stream->next_in || !stream->next_out || !stream->avail_out) return ZPACK_ERROR_STREAM_INVALID;
    const zpack_compression_method m = options->method;
    if (m != ZPACK_COMPRESSION_NONE && m != ZPACK_COMPRESSION_ZSTD && m != ZPACK_COMPRESSION_LZ4) return ZPACK_ERROR_COMP_METHOD_INVALID;
    if (zi_writer_sink(writer, NULL, NULL, NULL) == ZI_SINK_NONE) return ZPACK_ERROR_WRITER_NOT_OPENED;
    zi_stream_state* st = (zi_stream_state*)stream->xxh3_state;
    if (!st) return ZPACK_ERROR_STREAM_INVALID;
    zi_ctx* ctx = zi_pick_ctx(cctx, &writer->zstd_cctx);
    if (!ctx) return ZPACK_ERROR_NOT_AVAILABLE;
    if (!st->c && zpk_cstream_create(ctx->dev[0], &st->c) != ZPK_OK) return ZPACK_ERROR_MALLOC_FAILED;
    zpk_cstream_bind(st->c, ctx->dev[0]);
    if (stream->total_in == 0) {
        zpk_cstream_reset(st->c); st->c_active = 1;
        st->entry_offset = writer->write_offset;                  /* where this entry's first byte goes */
        int rc0 = zpk_cstream_configure(st->c, (uint32_t)m, options->level);
        if (rc0) return rc0;
    }
    int rc = zpk_cstream_update(st->c, stream->next_in, stream->avail_in);
    if (rc) return rc;
    stream->next_in += stream->avail_in;
    stream->total_in += stream->avail_in;
    stream->avail_in = 0;
    return stream_drain(writer, stream, st);
}

int zpack_write_file_stream_end(zpack_writer* writer, char* filename, zpack_compress_options* options, zpack_stream* stream, void* cctx)
{
    if (!stream->next_out || !stream->avail_out) return ZPACK_ERROR_STREAM_INVALID;
    const zpack_compression_method m = options->method;
    if (m != ZPACK_COMPRESSION_NONE && m != ZPACK_COMPRESSION_ZSTD && m != ZPACK_COMPRESSION_LZ4) return ZPACK_ERROR_COMP_METHOD_INVALID;
    if (zi_writer_sink(writer, NULL, NULL, NULL) == ZI_SINK_NONE) return ZPACK_ERROR_WRITER_NOT_OPENED;
    zi_stream_state* st = (zi_stream_state*)stream->xxh3_state;
    if (!st) return ZPACK_ERROR_STREAM_INVALID;
    zi_ctx* ctx = zi_pick_ctx(cctx, &writer->zstd_cctx);
    if (!ctx) return ZPACK_ERROR_NOT_AVAILABLE;
    if (!st->c && zpk_cstream_create(ctx->dev[0], &st->c) != ZPK_OK) return ZPACK_ERROR_MALLOC_FAILED;   /* an empty entry: end without update */
    zpk_cstream_bind(st->c, ctx->dev[0]);
    if (stream->total_in == 0 && !st->c_active) { zpk_cstream_reset(st->c); st->entry_offset = writer->write_offset; }
    uint64_t csize = 0, usize = 0, hash = 0;
    int rc = zpk_cstream_finish(st->c, (uint32_t)m, options->level, &csize, &usize, &hash);
    if (rc) return rc;
    if ((rc = stream_drain(writer, stream, st))) return rc;
    if ((rc = zi_writer_enter(writer, filename, st->entry_offset, csize, usize, hash, (zpack_u8)m))) return rc;
    zpk_cstream_reset(st->c);
    st->c_active = 0;
    return ZPACK_OK;
}

int zpack_write_archive(zpack_writer* writer, zpack_file* files, zpack_u64 file_count)
{
    int rc;
    if ((rc = zpack_write_header(writer))) return rc;
    if ((rc = zpack_write_data_header(writer))) return rc;
    if ((rc = zpack_write_files(writer, files, file_count))) return rc;
    if ((rc = zpack_write_cdr(writer))) return rc;
    return zpack_write_eocdr(writer);
}

void zpack_close_writer(zpack_writer* writer)
{
    zi_writer_dsink_drop(writer);                         /* (the image is the caller's: left alone) */
    if (writer->file) fclose(writer->file);
    free(writer->buffer);
    if (writer->file_entries) {
        for (zpack_u64 i = 0; i < writer->file_count; i++) free(writer->file_entries[i].filename);
        free(writer->file_entries);
    }
    zi_ctx_destroy((zi_ctx*)writer->zstd_cctx);
    memset(writer, 0, sizeof(*writer));
}
