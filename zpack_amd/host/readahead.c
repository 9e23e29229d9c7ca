/* readahead.c — read-ahead for callers that read one entry per zpack_read_file call, in CDR order.
 *
 * The reference's own read loop (tests/read_archive.c:21-35) and every program written against zpack.h read an archive one
 * entry per call; served as a device batch of one entry each, such a loop runs at the speed of a single wave.  A context
 * watches the entries its zpack_read_file calls ask for: once a call asks for entry i of a reader right after entry i - 1 of
 * the same reader, the run of entries from i on is decoded as ONE batch (the machinery of zpack_read_files) into host slots
 * the context owns, and the calls that follow are answered from there with a memcpy.  The first window of a run is small;
 * every refill in the same run doubles it, up to ZPACK_AMD_READ_AHEAD bytes of output (read when the context is created;
 * 0 = off) and ZI_RA_MAX_ENTRIES entries.  Any out-of-order call ends the run: random access decodes nothing it does not use.
 *
 * A call is answered from a window only when the window's decode of that entry (with one byte of room to spare) ended
 * ZPACK_OK with exactly uncomp_size bytes and the entry's fields are still the ones the window decoded.  Every other verdict — and every short decode, whose hash
 * covers the caller's own buffer bytes (lib/zpack_read.c:466) — comes from the per-call path, as before.  Windows are keyed
 * by (reader, generation): a reader that was closed or parsed again never sees a window of its earlier life, even at the
 * same address with the same CDR.  The window state is guarded by a mutex of its own: two threads that share one context
 * (legal here; the codec serialises them) still get the right bytes. */
#define _GNU_SOURCE                                        /* MAP_ANONYMOUS, MADV_HUGEPAGE */
#include "internal.h"
#include "zpack_amd.h"
#include <pthread.h>
#include <stdint.h>
#include <sys/mman.h>
#include <unistd.h>

/* defaults: a window of 256 MiB output / 16 384 entries keeps the chip busy for Zstandard entries of 256 KiB
 * (one wave each, milliseconds per entry) as well as for LZ4 entries of 64 KiB */
#define ZI_RA_DEFAULT_CAP   (256ull << 20)
#define ZI_RA_MAX_ENTRIES   16384ull
#define ZI_RA_FIRST_ENTRIES 8ull
#define ZI_RA_FIRST_BYTES   (1ull << 20)

typedef struct {
    zpack_u64 offset, comp_size, uncomp_size, hash;   /* the entry's fields when the window decoded it */
    zpack_u64 produced, at;                           /* bytes decoded; slot offset in the window's buffer */
    int       status;
    zpack_u8  method, served;
} zi_ra_slot;

typedef struct zi_ra_s {
    pthread_mutex_t mu;
    zpack_u64 cap;                                    /* bytes of output per window, 0 = off */
    /* the previous call, and the size of the next window of the run it belongs to */
    const zpack_reader* last_reader; zpack_u64 last_gen, last_idx;
    zpack_u64 next_bytes, next_entries;
    /* the window: entries [w_lo, w_lo + w_n) of (w_reader, w_gen) */
    const zpack_reader* w_reader; zpack_u64 w_gen, w_lo, w_n;
    zi_ra_slot* slots; zpack_u64 slots_cap;
    zpack_u8* buf; zpack_u64 buf_cap;                 /* output slots: one mapping for the whole cap, faulted in once */
    zpack_u8* span; zpack_u64 span_cap;               /* file-backed readers: the compressed span of a window, read in one piece */
    /* zpack_amd_read_ahead_stats */
    zpack_u64 served, own, windows, unused;
} zi_ra;

/* ------------------------------------------------------------------ reader generations
 * zpack_reader has the reference's fixed layout: the generation of a reader lives in a side table keyed by its address. */

static zi_side_table g_readers = ZI_SIDE_TABLE_INIT;     /* image: zpack_amd_init_reader_device's; word: the generation */
static zpack_u64 g_gen_next = 1;
/* zi_reader_gen_new and zi_reader_dimage_set read a record and write it back in two steps of the table, so they are not atomic per record:
 * both run while a reader is opened or parsed, which one thread does; the finds of other threads see the old record or the new one whole. */

void zi_reader_gen_new(const zpack_reader* reader)
{
    zi_side_rec r = { NULL, 0, -1 };
    (void)zi_side_find(&g_readers, reader, &r);             /* (a record at this address keeps its image) */
    r.word = __atomic_fetch_add(&g_gen_next, 1, __ATOMIC_RELAXED);
    (void)zi_side_set(&g_readers, reader, &r);              /* (out of memory: no generation, so this reader never reads ahead) */
}

void zi_reader_gen_drop(const zpack_reader* reader) { zi_side_drop(&g_readers, reader); }

zpack_u64 zi_reader_gen(const zpack_reader* reader)
{
    zi_side_rec r;
    return zi_side_find(&g_readers, reader, &r) ? r.word : 0;
}

int zi_reader_dimage_set(const zpack_reader* reader, const void* d_image, int device)
{
    zi_side_rec r = { NULL, 0, -1 };
    (void)zi_side_find(&g_readers, reader, &r);             /* (... and its generation) */
    r.image = d_image; r.device = device;
    return zi_side_set(&g_readers, reader, &r);
}

const void* zi_reader_dimage(const zpack_reader* reader, int* device)
{
    zi_side_rec r = { NULL, 0, -1 };
    (void)zi_side_find(&g_readers, reader, &r);
    if (device) *device = r.image ? r.device : -1;
    return r.image;
}

/* ------------------------------------------------------------------ the window */

zi_ra* zi_ra_create(void)
{
    zi_ra* ra = (zi_ra*)calloc(1, sizeof(*ra));
    if (!ra) return NULL;
    pthread_mutex_init(&ra->mu, NULL);
    ra->cap = ZI_RA_DEFAULT_CAP;
    const char* v = getenv("ZPACK_AMD_READ_AHEAD");
    if (v && *v) { char* end = NULL; unsigned long long q = strtoull(v, &end, 10); if (end && *end == 0 && v[0] != '-') ra->cap = q; }
    ra->next_bytes = ZI_RA_FIRST_BYTES; ra->next_entries = ZI_RA_FIRST_ENTRIES;
    return ra;
}

/* host buffers are mappings of their largest size: pages are faulted in once, as windows grow into them, and never again
 * (a buffer allocated anew at every doubling of the window took its page faults again each time) */
static zpack_u8* map_bytes(zpack_u64 size)
{
    void* p = mmap(NULL, (size_t)size, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (p == MAP_FAILED) return NULL;
    (void)madvise(p, (size_t)size, MADV_HUGEPAGE);              /* (advice only: fewer, larger faults where the kernel allows) */
    return (zpack_u8*)p;
}

static void forget_window(zi_ra* ra)
{
    for (zpack_u64 k = 0; k < ra->w_n; k++) if (!ra->slots[k].served) ra->unused++;
    ra->w_reader = NULL; ra->w_gen = 0; ra->w_lo = 0; ra->w_n = 0;
}

void zi_ra_drop(zi_ra* ra)
{
    if (!ra) return;
    pthread_mutex_lock(&ra->mu);
    forget_window(ra);
    if (ra->buf) munmap(ra->buf, (size_t)ra->buf_cap);
    if (ra->span) munmap(ra->span, (size_t)ra->span_cap);
    free(ra->slots);
    ra->buf = NULL; ra->buf_cap = 0; ra->span = NULL; ra->span_cap = 0; ra->slots = NULL; ra->slots_cap = 0;
    ra->last_reader = NULL; ra->last_gen = 0; ra->last_idx = 0;
    ra->next_bytes = ZI_RA_FIRST_BYTES; ra->next_entries = ZI_RA_FIRST_ENTRIES;
    pthread_mutex_unlock(&ra->mu);
}

void zi_ra_destroy(zi_ra* ra)
{
    if (!ra) return;
    zi_ra_drop(ra);
    pthread_mutex_destroy(&ra->mu);
    free(ra);
}

/* index of `entry` in the reader's own table, or 0 when it points anywhere else (a caller's copy takes the per-call path) */
static int entry_index(const zpack_reader* reader, const zpack_file_entry* entry, zpack_u64* idx)
{
    const uintptr_t base = (uintptr_t)reader->file_entries, at = (uintptr_t)entry;
    if (!reader->file_entries || at < base || (at - base) % sizeof(zpack_file_entry)) return 0;
    const zpack_u64 i = (zpack_u64)((at - base) / sizeof(zpack_file_entry));
    if (i >= reader->file_count) return 0;
    *idx = i;
    return 1;
}

/* may entry e join a window: it passes the host guards of zpack_read_file that do not depend on the caller's max_size, and
 * it is not large (those keep the block- and frame-parallel routes of the per-call path).  An empty entry (comp_size 0) joins
 * as a step of the run: zpack_read_file answers it before any decode. */
static int joins(const zpack_reader* reader, const zpack_file_entry* e, zpack_u64 cap)
{
    if (e->comp_size == 0) return 1;
    return e->offset < reader->file_size && e->comp_size < reader->file_size - e->offset && e->uncomp_size <= cap / 4;
}

static int pread_all(FILE* fp, zpack_u8* dst, zpack_u64 off, zpack_u64 n)
{
    const int fd = fileno(fp);
    if (fd < 0) return 0;
    while (n) {
        const ssize_t got = pread(fd, dst, (size_t)(n < (1ull << 30) ? n : (1ull << 30)), (off_t)off);
        if (got <= 0) return 0;
        dst += got; off += (zpack_u64)got; n -= (zpack_u64)got;
    }
    return 1;
}

/* decode the run of entries from index i as one batch; 1 when a window of at least two entries is in place */
static int fill_window(zi_ra* ra, zi_ctx* ctx, zpack_reader* reader, zpack_u64 gen, zpack_u64 i)
{
    const zpack_u64 max_n = ra->next_entries < ZI_RA_MAX_ENTRIES ? ra->next_entries : ZI_RA_MAX_ENTRIES;
    const zpack_u64 max_b = ra->next_bytes < ra->cap ? ra->next_bytes : ra->cap;
    zpack_u64 n = 0, nd = 0, bytes = 0, lo = 0, hi = 0;
    for (zpack_u64 j = i; j < reader->file_count && n < max_n; j++, n++) {
        const zpack_file_entry* e = reader->file_entries + j;
        if (!joins(reader, e, ra->cap)) break;
        if (e->comp_size == 0) continue;
        if (n && bytes + e->uncomp_size > max_b) break;
        /* the compressed span of the window is staged whole (by the codec, or read in one piece for a file-backed reader) */
        const zpack_u64 end = e->offset + e->comp_size, nlo = nd && lo < e->offset ? lo : e->offset, nhi = nd && hi > end ? hi : end;
        if (nhi - nlo > 2 * ra->cap) break;
        lo = nlo; hi = nhi;
        bytes += e->uncomp_size;
        nd++;
    }
    forget_window(ra);
    if (n < 2 || nd == 0) return 0;
    int ok = 1;
    if (n > ra->slots_cap) {
        zi_ra_slot* s = (zi_ra_slot*)realloc(ra->slots, sizeof(zi_ra_slot) * (size_t)n);
        if (s) { ra->slots = s; ra->slots_cap = n; }
        else ok = 0;
    }
    if (ok && !ra->buf) {                                      /* every window fits: bytes <= cap, plus one byte per slot */
        ra->buf = map_bytes(ra->cap + ZI_RA_MAX_ENTRIES);
        ra->buf_cap = ra->buf ? ra->cap + ZI_RA_MAX_ENTRIES : 0;
        ok = ra->buf != NULL;
    }
    const zpack_u8* span = NULL;
    if (ok && reader->file) {
        /* a file-backed window reads its compressed span in one piece into a buffer of its own, plus the 1-byte pad behind it;
         * the device then sees the same image as for the per-entry gather of zi_decode_entries, at one read instead of one per
         * entry.  (pread: the FILE's position and buffer are not touched) */
        if (!ra->span) {
            ra->span = map_bytes(2 * ra->cap + 1);
            ra->span_cap = ra->span ? 2 * ra->cap + 1 : 0;
        }
        ok = ra->span && pread_all(reader->file, ra->span, lo, hi - lo);
        if (ok) { ra->span[hi - lo] = 0; span = ra->span; }
    }
    zpack_file_entry** ents = (zpack_file_entry**)malloc(sizeof(*ents) * (size_t)nd);
    zpack_u8** outs = (zpack_u8**)malloc(sizeof(*outs) * (size_t)nd);
    size_t* caps = (size_t*)malloc(sizeof(*caps) * (size_t)nd);
    zpk_decode_result* res = (zpk_decode_result*)calloc((size_t)nd, sizeof(*res));
    ok = ok && ents && outs && caps && res;
    if (ok) {
        zpack_u64 at = 0, d = 0;
        for (zpack_u64 k = 0; k < n; k++) {
            zpack_file_entry* e = reader->file_entries + i + k;
            zi_ra_slot* s = &ra->slots[k];
            s->offset = e->offset; s->comp_size = e->comp_size; s->uncomp_size = e->uncomp_size; s->hash = e->hash; s->method = e->comp_method;
            s->at = at; s->produced = 0;
            if (e->comp_size == 0) { s->status = -1; s->served = 1; continue; }      /* never decoded, never served, not "unused" */
            s->served = 0;
            /* a slot of uncomp_size + 1 bytes.  A decode that ends ZPACK_OK with exactly uncomp_size bytes there stopped on its own,
             * never at the end of the room it had, so every max_size >= uncomp_size gets that verdict and those bytes.  With no room
             * to spare the verdict can differ: lib/zpack_read.c:414-439 stops at a full buffer and ignores what follows the frame,
             * with room it reads on (tests/golden/foreign_frames.json, "frame_then_5_bytes" with and without "_capacity_full"). */
            ents[d] = e; outs[d] = ra->buf + at; caps[d] = (size_t)e->uncomp_size + 1;
            at += e->uncomp_size + 1;
            d++;
        }
        ok = zi_decode_entries(reader, ctx, ents, nd, outs, caps, res, span, lo, hi - lo + 1) == ZPACK_OK;
        if (ok)
            for (zpack_u64 k = 0, q = 0; k < n; k++)
                if (ra->slots[k].comp_size) { ra->slots[k].status = res[q].status; ra->slots[k].produced = res[q].produced; q++; }
    }
    if (ok) {
        ra->w_reader = reader; ra->w_gen = gen; ra->w_lo = i; ra->w_n = n;
        ra->windows++;
        ra->next_bytes = ra->next_bytes < ra->cap / 2 ? ra->next_bytes * 2 : ra->cap;
        ra->next_entries = ra->next_entries < ZI_RA_MAX_ENTRIES / 2 ? ra->next_entries * 2 : ZI_RA_MAX_ENTRIES;
    } else {
        /* out of host or device memory for a window: the run ends, so the next calls do not try a window of that size again */
        ra->next_bytes = ZI_RA_FIRST_BYTES; ra->next_entries = ZI_RA_FIRST_ENTRIES;
        ra->last_reader = NULL;
    }
    free(ents); free(outs); free(caps); free(res);
    return ok;
}

/* record call i of this reader: 1 when it continues an in-order run.  A call out of order ends the run. */
static int step(zi_ra* ra, const zpack_reader* reader, zpack_u64 gen, zpack_u64 i)
{
    const int in_order = ra->last_reader == reader && ra->last_gen == gen && ra->last_idx + 1 == i;
    if (!in_order) { ra->next_bytes = ZI_RA_FIRST_BYTES; ra->next_entries = ZI_RA_FIRST_ENTRIES; }
    ra->last_reader = reader; ra->last_gen = gen; ra->last_idx = i;
    return in_order;
}

static int serve(zi_ra* ra, zi_ctx* ctx, zpack_reader* reader, const zpack_file_entry* entry, zpack_u8* buffer)
{
    zpack_u64 i = 0, gen = 0;
    if (!ra->cap || !entry_index(reader, entry, &i) || !(gen = zi_reader_gen(reader))) return 0;
    const int in_order = step(ra, reader, gen, i);
    int have = ra->w_n && ra->w_reader == reader && ra->w_gen == gen && i >= ra->w_lo && i - ra->w_lo < ra->w_n;
    if (!have && in_order) have = fill_window(ra, ctx, reader, gen, i);
    if (!have) return 0;
    zi_ra_slot* s = &ra->slots[i - ra->w_lo];
    if (s->status != ZPACK_OK || s->produced != s->uncomp_size || s->offset != entry->offset || s->comp_size != entry->comp_size ||
        s->uncomp_size != entry->uncomp_size || s->hash != entry->hash || s->method != entry->comp_method) return 0;
    memcpy(buffer, ra->buf + s->at, (size_t)s->uncomp_size);
    s->served = 1;
    reader->last_return = 0;                                    /* what the per-call path leaves on ZPACK_OK */
    return 1;
}

int zi_ra_read(zi_ctx* ctx, zpack_reader* reader, const zpack_file_entry* entry, zpack_u8* buffer)
{
    zi_ra* ra = ctx->ra;
    if (!ra) return 0;
    pthread_mutex_lock(&ra->mu);
    const int done = serve(ra, ctx, reader, entry, buffer);
    if (done) ra->served++;
    else ra->own++;
    pthread_mutex_unlock(&ra->mu);
    return done;
}

void zi_ra_step(zi_ctx* ctx, zpack_reader* reader, const zpack_file_entry* entry)
{
    zi_ra* ra = ctx->ra;
    zpack_u64 i = 0, gen = 0;
    if (!ra || !ra->cap || !entry_index(reader, entry, &i) || !(gen = zi_reader_gen(reader))) return;
    pthread_mutex_lock(&ra->mu);
    (void)step(ra, reader, gen, i);
    pthread_mutex_unlock(&ra->mu);
}

int zpack_amd_read_ahead_stats(const zpack_reader* reader, void* dctx, zpack_u64 out[6])
{
    if (!out) return ZPACK_ERROR_STREAM_INVALID;
    memset(out, 0, sizeof(zpack_u64) * 6);
    const zi_ctx* x = (const zi_ctx*)(dctx ? dctx : reader ? reader->zstd_dctx : NULL);
    if (!x || !x->ra) return ZPACK_OK;
    zi_ra* ra = x->ra;
    pthread_mutex_lock(&ra->mu);
    out[0] = ra->served; out[1] = ra->own; out[2] = ra->windows; out[3] = ra->unused;
    out[4] = ra->buf_cap + ra->span_cap + ra->slots_cap * sizeof(zi_ra_slot);
    out[5] = ra->cap;
    pthread_mutex_unlock(&ra->mu);
    return ZPACK_OK;
}
