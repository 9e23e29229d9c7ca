/* internal.h — shared by the host-side zpack.h implementation (reader.c, writer.c, readahead.c, stream.c, util.c).
 * Nothing here is part of the public API.  util.c holds what more than one file needs: the contexts and their codec lookup
 * (zi_ctx_codec_on, zi_ctx_codec_of), the mapping of a codec's return (zi_rc_of_codec), the static shard (zi_shard) and the one
 * side-table implementation (zi_side_*) behind the readers' and the writers' records; writer.c holds the one way a file is entered
 * (zi_writer_enter). */
#ifndef ZPACK_AMD_INTERNAL_H
#define ZPACK_AMD_INTERNAL_H

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/types.h>
#include <pthread.h>
#include "zpack.h"
#include "zpack_codec.h"

/* little-endian field access (the format is LE everywhere: docs/specs.md) */
static inline zpack_u16 zi_get16(const zpack_u8* p) { return (zpack_u16)(p[0] | (p[1] << 8)); }
static inline zpack_u32 zi_get32(const zpack_u8* p) { return (zpack_u32)p[0] | ((zpack_u32)p[1] << 8) | ((zpack_u32)p[2] << 16) | ((zpack_u32)p[3] << 24); }
static inline zpack_u64 zi_get64(const zpack_u8* p) { return (zpack_u64)zi_get32(p) | ((zpack_u64)zi_get32(p + 4) << 32); }
static inline void zi_put16(zpack_u8* p, zpack_u16 v) { p[0] = (zpack_u8)v; p[1] = (zpack_u8)(v >> 8); }
static inline void zi_put32(zpack_u8* p, zpack_u32 v) { for (int i = 0; i < 4; i++) p[i] = (zpack_u8)(v >> (8 * i)); }
static inline void zi_put64(zpack_u8* p, zpack_u64 v) { for (int i = 0; i < 8; i++) p[i] = (zpack_u8)(v >> (8 * i)); }

/* 64-bit clean file positioning (the reference maps these per platform, lib/zpack_common.h:37-78) */
#define zi_fseek(fp, off, whence) fseeko((fp), (off_t)(off), (whence))
#define zi_ftell(fp) ((zpack_u64)ftello(fp))

/* a context = the device codecs a reader / writer / explicit dctx / cctx works with (util.c), and the read-ahead window of the
 * in-order zpack_read_file callers that use it (readahead.c) */
#define ZI_MAX_DEVICES 16
struct zi_ra_s;
typedef struct zi_ctx_s { int n; zpk_codec* dev[ZI_MAX_DEVICES]; struct zi_ra_s* ra; } zi_ctx;
zi_ctx* zi_ctx_create(void);                 /* NULL when no HIP device is usable: there is no CPU fallback */
void    zi_ctx_destroy(zi_ctx* x);
void    zi_ctx_reset(zi_ctx* x);
/* resolve the context of a call: the explicit one, else the owner's (created on first use, freed by zpack_close_*) */
zi_ctx* zi_pick_ctx(void* explicit_ctx, void** owner_slot);
/* the static shard of a batch over the context's codecs: contiguous ranges of about equal weight(items, i), at most one
 * per codec and per item, cut[k] .. cut[k + 1] for k in [0, parts); returns parts (1: one codec, one item, or no memory for the weights) */
int zi_shard(zi_ctx* ctx, zpack_u64 count, zpack_u64 (*weight)(const void* items, zpack_u64 i), const void* items, zpack_u64* cut);
void zi_parallel(int parts, void (*fn)(void*, int), void* arg);
/* name index of reader-owned entry tables (zpack_get_file_entry) */
void zi_index_register(const zpack_file_entry* table, zpack_u64 count);
void zi_index_drop(const zpack_file_entry* table);

/* decode entries in one device batch on context `ctx` (reader.c): per-entry verdicts in res[], reader->last_return untouched.
 * span != NULL: the payloads come from there — archive bytes [span_lo, span_lo + span_size - 1) and one pad byte, covering
 * entries that all pass the host guards — instead of the reader's memory image or file */
int zi_decode_entries(zpack_reader* reader, zi_ctx* ctx, zpack_file_entry* const* entries, zpack_u64 count,
                      zpack_u8* const* buffers, const size_t* max_sizes, zpk_decode_result* res,
                      const zpack_u8* span, zpack_u64 span_lo, zpack_u64 span_size);
/* ... with the PLAINTEXT IN DEVICE MEMORY (zpack_amd.h: zpack_amd_read_files_device): buffers[i] are device pointers, the batch runs on
 * the one codec of `ctx` whose device they belong to (ZPACK_ERROR_NOT_AVAILABLE when it has none; ZPACK_ERROR_STREAM_INVALID when
 * the codec's pointer check turns a buffer down) */
int zi_decode_entries_device(zpack_reader* reader, zi_ctx* ctx, zpack_file_entry* const* entries, zpack_u64 count,
                             zpack_u8* const* d_buffers, const size_t* max_sizes, zpk_decode_result* res);
/* the codec of `ctx` on the device that the first device pointer among ptrs[0, n) with sizes[i] != 0 belongs to (stride: bytes from one
 * pointer / size to the next, the arrays may be fields of structs).  *rc = ZPACK_OK with NULL: no entry has bytes, any codec serves;
 * ZPACK_ERROR_STREAM_INVALID: bytes, but no device pointer; ZPACK_ERROR_NOT_AVAILABLE: a device the context does not hold */
zpk_codec* zi_ctx_codec_of(zi_ctx* ctx, const void* ptrs, size_t ptr_stride, const void* sizes, size_t size_stride, int size_is_u64, zpack_u64 n, int* rc);
/* the codec of `ctx` on HIP device `device`, NULL when the context holds none */
zpk_codec* zi_ctx_codec_on(zi_ctx* ctx, int device);
/* what a batch call of the codec returned, as the library reports it: ZPK_E_INVALID (the pointer rule turned something down) is
 * ZPACK_ERROR_STREAM_INVALID, any other failure ZPACK_ERROR_NOT_AVAILABLE */
int zi_rc_of_codec(int crc);
/* the element sizes of a byte-plane call (zpack_amd.h): 1 when there are none (NULL) or every one of the n is 1, 2, 4 or 8 */
int zi_elem_sizes_valid(const zpack_u8* elem_sizes, zpack_u64 n);

/* side tables (util.c): records kept beside structs of fixed layout, keyed by the struct's address.  One implementation, two instances —
 * the readers' (readahead.c: word = the generation) and the writers' (writer.c: word = the image's capacity) — and never one table for
 * both: a closed reader's address may become a writer's.  find -> 1 and *out, 0 when there is no record; set creates or replaces -> 1,
 * 0 when there is no memory for the record; drop forgets (a missing key: nothing). */
typedef struct { const void* image; zpack_u64 word; int device; } zi_side_rec;
typedef struct zi_side_node_s { const void* key; zi_side_rec rec; struct zi_side_node_s* next; } zi_side_node;
#define ZI_SIDE_BUCKETS 64
typedef struct { pthread_rwlock_t mu; zi_side_node* bucket[ZI_SIDE_BUCKETS]; } zi_side_table;
#define ZI_SIDE_TABLE_INIT { PTHREAD_RWLOCK_INITIALIZER, { NULL } }
int  zi_side_find(zi_side_table* t, const void* key, zi_side_rec* out);
int  zi_side_set(zi_side_table* t, const void* key, const zi_side_rec* rec);
void zi_side_drop(zi_side_table* t, const void* key);

/* read-ahead for in-order zpack_read_file callers (readahead.c) */
struct zi_ra_s* zi_ra_create(void);          /* reads ZPACK_AMD_READ_AHEAD; NULL when out of memory (read-ahead is then off) */
void zi_ra_destroy(struct zi_ra_s* ra);
void zi_ra_drop(struct zi_ra_s* ra);         /* forget the window and free its memory */
/* 1 when the call was answered from a window (buffer filled, last_return set), 0 when the caller decodes the entry on its own;
 * called once the host guards of zpack_read_file have passed */
int  zi_ra_read(zi_ctx* ctx, zpack_reader* reader, const zpack_file_entry* entry, zpack_u8* buffer);
/* an entry answered before any decode (comp_size 0): still a step of an in-order run of this context */
void zi_ra_step(zi_ctx* ctx, zpack_reader* reader, const zpack_file_entry* entry);
/* reader generations: a new one at every parse of a reader, dropped by zpack_close_reader; 0 = a reader never parsed here */
void      zi_reader_gen_new(const zpack_reader* reader);
void      zi_reader_gen_drop(const zpack_reader* reader);
zpack_u64 zi_reader_gen(const zpack_reader* reader);
/* ... and, in the same record of the readers' side table, the image of a reader opened by zpack_amd_init_reader_device (zpack_reader has a fixed layout and no field
 * for it): set -> 1, 0 when there is no memory for the record; get -> the image (*device: its HIP ordinal), NULL for any other reader.
 * zi_reader_gen_drop forgets it with the record. */
int         zi_reader_dimage_set(const zpack_reader* reader, const void* d_image, int device);
const void* zi_reader_dimage(const zpack_reader* reader, int* device);

/* Is a reader loaded, and from where: its FILE, its host image, or an image in device memory (*d_image, *device; both may be NULL).
 * The side table is only asked when the reader has neither a file nor a buffer. */
typedef enum { ZI_SRC_NONE = 0, ZI_SRC_FILE, ZI_SRC_MEMORY, ZI_SRC_DEVICE } zi_source;
zi_source zi_reader_source(const zpack_reader* reader, const zpack_u8** d_image, int* device);
/* bytes [at, at + n) of a device image brought home (zpk_codec_fetch_device): ZPACK_OK, or ZPACK_ERROR_READ_FAILED */
int zi_dimage_fetch(const zpack_u8* d_image, zpack_u64 at, zpack_u8* dst, size_t n);

/* per-stream aggregation state hung off zpack_stream.xxh3_state */
typedef struct zi_stream_state_s {
    zpk_dstream* d;
    zpk_cstream* c;
    int          d_active, c_active;
    zpack_u64    entry_offset;       /* streaming write: archive offset of the entry being written */
} zi_stream_state;

/* Is a writer opened, and on what: its FILE, its growing heap buffer, or a bounded image in device memory (zpack_amd_init_writer_device:
 * *d_image, *capacity, *device; each may be NULL).  zpack_writer has a fixed layout and no field for the image: it is kept in the writers' side
 * table (zi_side_table, above), which is only asked when the writer has neither a file nor a buffer.  A record that outlived
 * its writer (a struct never closed whose address serves again) is replaced by the next zpack_amd_init_writer_device there, dropped by the
 * other inits and by zpack_close_writer, and does not answer for a struct whose buffer_capacity is not the record's capacity — a zeroed
 * struct is ZPACK_ERROR_WRITER_NOT_OPENED. */
typedef enum { ZI_SINK_NONE = 0, ZI_SINK_FILE, ZI_SINK_HEAP, ZI_SINK_DEVICE } zi_sink;
zi_sink zi_writer_sink(const zpack_writer* w, zpack_u8** d_image, size_t* capacity, int* device);
int  zi_writer_dsink_set(const zpack_writer* w, void* d_image, size_t capacity, int device);   /* 1, or 0 when there is no memory for the record */
void zi_writer_dsink_drop(const zpack_writer* w);

/* the writer's unified sink: file, growing heap buffer or bounded device image, at the writer's cursor.  A block that does not fit a
 * device image writes nothing: ZPACK_ERROR_BUFFER_TOO_SMALL, the offsets do not move. */
int zi_writer_put(zpack_writer* w, const zpack_u8* data, size_t size);
zpack_file_entry* zi_writer_push_entry(zpack_writer* w);
/* a file entered into the writer's table under a copy of `name`: ZPACK_OK, or ZPACK_ERROR_MALLOC_FAILED */
int zi_writer_enter(zpack_writer* w, const char* name, zpack_u64 offset, zpack_u64 comp_size, zpack_u64 uncomp_size, zpack_u64 hash, zpack_u8 method);
/* the offset guard of a raw entry against its image (lib/zpack_write.c:345-428): the payload lies inside file_size bytes */
static inline int zi_entry_in_image(const zpack_file_entry* e, zpack_u64 file_size) { return e->offset < file_size && e->comp_size <= file_size - e->offset; }

#endif
