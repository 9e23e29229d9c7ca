/* per_entry_rate.c — the reference's read loop (tests/read_archive.c:21-35) against any zpack.h library, timed.
 *
 *   per_entry_rate LIB ARCHIVE mem|file seq|rand CALLS
 *
 * dlopen()s LIB (libzpack_amd.so or the compiled reference), opens ARCHIVE memory-backed (zpack_init_reader_memory_shared
 * over the file's bytes) or file-backed (zpack_init_reader), then calls zpack_read_file(reader, reader->file_entries + i,
 * buffer, max_size, NULL) CALLS times: entries 0, 1, 2, ... in CDR order (seq) or in a fixed pseudo-random order (rand), one
 * buffer for every call.  Prints one JSON line; the exit status is non-zero when any call fails. */
#define _POSIX_C_SOURCE 200809L
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <sys/resource.h>
#include "zpack.h"

typedef int  (*init_mem_fn)(zpack_reader*, zpack_u8*, size_t);
typedef int  (*init_file_fn)(zpack_reader*, const char*);
typedef int  (*read_fn)(zpack_reader*, zpack_file_entry*, zpack_u8*, size_t, void*);
typedef void (*close_fn)(zpack_reader*);

static double now(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

int main(int argc, char** argv)
{
    if (argc != 6) { fprintf(stderr, "usage: %s LIB ARCHIVE mem|file seq|rand CALLS\n", argv[0]); return 2; }
    const int mem = strcmp(argv[3], "mem") == 0, rnd = strcmp(argv[4], "rand") == 0;
    const unsigned long long want = strtoull(argv[5], NULL, 10);
    void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!lib) { fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    init_mem_fn init_mem = (init_mem_fn)dlsym(lib, "zpack_init_reader_memory_shared");
    init_file_fn init_file = (init_file_fn)dlsym(lib, "zpack_init_reader");
    read_fn read_file = (read_fn)dlsym(lib, "zpack_read_file");
    close_fn close_reader = (close_fn)dlsym(lib, "zpack_close_reader");
    if (!init_mem || !init_file || !read_file || !close_reader) { fprintf(stderr, "missing zpack.h symbols\n"); return 2; }

    zpack_reader reader;
    memset(&reader, 0, sizeof(reader));
    zpack_u8* image = NULL;
    int rc;
    if (mem) {
        FILE* fp = fopen(argv[2], "rb");
        if (!fp) { perror(argv[2]); return 2; }
        fseeko(fp, 0, SEEK_END);
        const size_t size = (size_t)ftello(fp);
        fseeko(fp, 0, SEEK_SET);
        image = (zpack_u8*)malloc(size);
        if (!image || fread(image, size, 1, fp) != 1) { fprintf(stderr, "read %s failed\n", argv[2]); return 2; }
        fclose(fp);
        rc = init_mem(&reader, image, size);
    } else {
        rc = init_file(&reader, argv[2]);
    }
    if (rc) { fprintf(stderr, "open -> %d\n", rc); return 2; }
    const zpack_u64 n = reader.file_count;
    zpack_u64 calls = want && want < n ? want : n;
    zpack_u64* order = (zpack_u64*)malloc(sizeof(zpack_u64) * (size_t)(n ? n : 1));
    size_t max_size = 1;
    for (zpack_u64 i = 0; i < n; i++) {
        order[i] = i;
        if (reader.file_entries[i].uncomp_size > max_size) max_size = (size_t)reader.file_entries[i].uncomp_size;
    }
    if (rnd) {                                          /* Fisher-Yates with a fixed 64-bit LCG: the same order every run */
        zpack_u64 s = 0x9E3779B97F4A7C15ull;
        for (zpack_u64 i = n; i > 1; i--) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            const zpack_u64 j = (s >> 33) % i, t = order[i - 1];
            order[i - 1] = order[j]; order[j] = t;
        }
    }
    zpack_u8* buffer = (zpack_u8*)malloc(max_size);
    memset(buffer, 0, max_size);                         /* (touch the pages before the clock starts) */
    zpack_u64 bytes = 0, failed = 0;
    struct rusage ru0, ru1;
    getrusage(RUSAGE_SELF, &ru0);
    const double t0 = now();
    double t1 = t0;                                      /* end of the first call: it also creates the library's context */
    for (zpack_u64 k = 0; k < calls; k++) {
        zpack_file_entry* e = reader.file_entries + order[k];
        if (read_file(&reader, e, buffer, max_size, NULL) != ZPACK_OK) failed++;
        bytes += e->uncomp_size;
        if (k == 0) t1 = now();
    }
    const double dt = now() - t0;
    getrusage(RUSAGE_SELF, &ru1);
    printf("{\"mode\": \"%s\", \"order\": \"%s\", \"calls\": %llu, \"bytes\": %llu, \"seconds\": %.6f, \"gib_s\": %.4f, "
           "\"us_per_call\": %.2f, \"first_call_ms\": %.3f, \"minflt\": %ld, \"failed\": %llu}\n", argv[3], argv[4], (unsigned long long)calls,
           (unsigned long long)bytes, dt, dt > 0 ? (double)bytes / dt / (1024.0 * 1024.0 * 1024.0) : 0.0, calls ? dt * 1e6 / (double)calls : 0.0,
           (t1 - t0) * 1e3, ru1.ru_minflt - ru0.ru_minflt, (unsigned long long)failed);
    close_reader(&reader);
    free(buffer); free(order); free(image);
    return failed ? 1 : 0;
}
