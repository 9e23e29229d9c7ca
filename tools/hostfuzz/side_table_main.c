/* side_table_main.c — the side tables of the host library (zpack_amd/host/util.c: zi_side_find / _set / _drop, internal.h) driven on the
 * CPU: this program is linked with the very util.c the library compiles, once under AddressSanitizer + UBSan and once under
 * ThreadSanitizer (tools/hostfuzz/run_side_table.sh).  The keys are addresses that are never read through.  One summary line per case;
 * tests/test_side_table_cpu.py asserts them. */
#include "internal.h"
#include <stdint.h>

/* what the rest of util.c refers to and this program never calls: no device, no read-ahead */
int  zpk_codec_device_count(void) { return 0; }
int  zpk_codec_create(zpk_codec** out, int device) { (void)device; *out = NULL; return ZPK_E_NO_DEVICE; }
void zpk_codec_destroy(zpk_codec* c) { (void)c; }
void zpk_codec_reset(zpk_codec* c) { (void)c; }
int  zpk_codec_device(const zpk_codec* c) { (void)c; return -1; }
int  zpk_codec_set_option(zpk_codec* c, int option, int value) { (void)c; (void)option; (void)value; return ZPK_E_INVALID; }
int  zpk_codec_pointer_device(const void* ptr) { (void)ptr; return -1; }
struct zi_ra_s* zi_ra_create(void) { return NULL; }
void zi_ra_destroy(struct zi_ra_s* ra) { (void)ra; }

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static zi_side_table g_a = ZI_SIDE_TABLE_INIT, g_b = ZI_SIDE_TABLE_INIT;

/* key i of a family: 16 x 64 bytes apart, so every key of a family falls into one bucket */
#define STRIDE (16u * ZI_SIDE_BUCKETS)
static const void* key_of(uintptr_t family, uintptr_t i) { return (const void*)(family + i * STRIDE); }
static zi_side_rec rec_of(const void* key, zpack_u64 salt)
{
    zi_side_rec r = { (const char*)key + 1, (zpack_u64)(uintptr_t)key * 3 + salt, (int)(((uintptr_t)key / STRIDE) & 7) };
    return r;
}
static int rec_is(const zi_side_rec* r, const void* key, zpack_u64 salt)
{
    const zi_side_rec w = rec_of(key, salt);
    return r->image == w.image && r->word == w.word && r->device == w.device;
}

static void chain_case(void)
{
    enum { N = 1000 };
    const uintptr_t fam = 0x10000;
    zi_side_rec r;
    for (uintptr_t i = 0; i < N; i++) { r = rec_of(key_of(fam, i), 0); CHECK(zi_side_set(&g_a, key_of(fam, i), &r) == 1); }
    for (uintptr_t i = 0; i < N; i++) CHECK(zi_side_find(&g_a, key_of(fam, i), &r) && rec_is(&r, key_of(fam, i), 0));
    /* the chain grows at its tail: key 0 is the head, key N - 1 the tail */
    const uintptr_t gone[] = { N / 2, 0, N - 1, N / 2 + 1, 1, N - 2 };
    unsigned dropped = 0;
    for (size_t g = 0; g < sizeof(gone) / sizeof(gone[0]); g++) {
        zi_side_drop(&g_a, key_of(fam, gone[g]));
        dropped++;
        for (uintptr_t i = 0; i < N; i++) {
            int is_gone = 0;
            for (size_t h = 0; h <= g; h++) is_gone |= gone[h] == i;
            const int found = zi_side_find(&g_a, key_of(fam, i), &r);
            CHECK(found == !is_gone && (!found || rec_is(&r, key_of(fam, i), 0)));
        }
    }
    unsigned left = 0;
    for (uintptr_t i = 0; i < N; i++) if (zi_side_find(&g_a, key_of(fam, i), &r)) { left++; zi_side_drop(&g_a, key_of(fam, i)); }
    for (uintptr_t i = 0; i < N; i++) CHECK(!zi_side_find(&g_a, key_of(fam, i), &r));
    printf("chain: %d keys in one bucket, %u dropped from the middle, the head and the tail, %u found and dropped after\n", N, dropped, left);
}

/* ---- eight threads find while two set and drop disjoint keys */
enum { OPS = 10000, FINDERS = 8, WRITERS = 2, LIVE = 64 };
static const uintptr_t FAM_STABLE = 0x4000000, FAM_W[WRITERS] = { 0x8000000, 0xC000000 };
static unsigned long g_hits[FINDERS], g_bad[FINDERS + WRITERS];

static void* finder(void* arg)
{
    const int id = (int)(intptr_t)arg;
    zi_side_rec r;
    unsigned x = 12345u + (unsigned)id;
    for (int op = 0; op < OPS; op++) {
        x = x * 1664525u + 1013904223u;
        const unsigned pick = (x >> 8) % 3, i = (x >> 16) % LIVE;
        const void* key = key_of(pick == 0 ? FAM_STABLE : FAM_W[pick - 1], i);
        const int found = zi_side_find(&g_a, key, &r);
        if (found) g_hits[id]++;
        if (found && !rec_is(&r, key, pick)) g_bad[id]++;                 /* a record is whole, or it is not there */
        if (pick == 0 && !found) g_bad[id]++;                             /* the stable keys are never dropped */
    }
    return NULL;
}

static void* writer(void* arg)
{
    const int id = (int)(intptr_t)arg;
    zi_side_rec r;
    for (int op = 0; op < OPS; op++) {
        const void* key = key_of(FAM_W[id], (uintptr_t)(op / 2) % LIVE);
        if (op % 2 == 0) { r = rec_of(key, (zpack_u64)id + 1); if (!zi_side_set(&g_a, key, &r)) g_bad[FINDERS + id]++; }
        else {
            if (!zi_side_find(&g_a, key, &r) || !rec_is(&r, key, (zpack_u64)id + 1)) g_bad[FINDERS + id]++;     /* its own key: nobody else touches it */
            zi_side_drop(&g_a, key);
        }
    }
    return NULL;
}

static void threads_case(void)
{
    zi_side_rec r;
    for (uintptr_t i = 0; i < LIVE; i++) { r = rec_of(key_of(FAM_STABLE, i), 0); CHECK(zi_side_set(&g_a, key_of(FAM_STABLE, i), &r)); }
    pthread_t th[FINDERS + WRITERS];
    for (int k = 0; k < FINDERS + WRITERS; k++)
        CHECK(pthread_create(&th[k], NULL, k < FINDERS ? finder : writer, (void*)(intptr_t)(k < FINDERS ? k : k - FINDERS)) == 0);
    for (int k = 0; k < FINDERS + WRITERS; k++) pthread_join(th[k], NULL);
    unsigned long bad = 0, hits = 0;
    for (int k = 0; k < FINDERS + WRITERS; k++) bad += g_bad[k];
    for (int k = 0; k < FINDERS; k++) hits += g_hits[k];
    CHECK(hits > 0);
    for (int w = 0; w < WRITERS; w++) for (uintptr_t i = 0; i < LIVE; i++) CHECK(!zi_side_find(&g_a, key_of(FAM_W[w], i), &r));
    for (uintptr_t i = 0; i < LIVE; i++) zi_side_drop(&g_a, key_of(FAM_STABLE, i));
    printf("threads: %d finders and %d writers, %d operations each, %lu torn or missing records\n", FINDERS, WRITERS, OPS, bad);
    CHECK(bad == 0);
}

int main(void)
{
    zi_side_rec r = { NULL, 77, 5 };
    const void* k1 = key_of(0x1000, 1);
    CHECK(!zi_side_find(&g_a, k1, &r) && r.word == 77 && r.device == 5);
    printf("empty: nothing found, the caller's record untouched\n");

    zi_side_rec a = rec_of(k1, 0);
    CHECK(zi_side_set(&g_a, k1, &a) == 1 && zi_side_find(&g_a, k1, &r) && rec_is(&r, k1, 0));
    printf("set: found with its three fields\n");

    a = rec_of(k1, 9);
    CHECK(zi_side_set(&g_a, k1, &a) == 1 && zi_side_find(&g_a, k1, &r) && rec_is(&r, k1, 9));
    zi_side_drop(&g_a, k1);
    CHECK(!zi_side_find(&g_a, k1, &r));                                   /* one record, not two: the first is not behind it */
    printf("replace: a second set at the key replaced the record, one drop forgot it\n");

    chain_case();

    a = rec_of(k1, 1);
    CHECK(zi_side_set(&g_a, k1, &a));
    zi_side_drop(&g_a, key_of(0x1000, 2));                                /* same bucket, not there */
    zi_side_drop(&g_a, (const void*)0x2010);                              /* an empty bucket */
    CHECK(zi_side_find(&g_a, k1, &r) && rec_is(&r, k1, 1));
    zi_side_drop(&g_a, k1);
    zi_side_drop(&g_a, k1);
    CHECK(!zi_side_find(&g_a, k1, &r));
    printf("missing: dropping a key that is not there changes nothing\n");

    a = rec_of(k1, 2);
    zi_side_rec b = rec_of(k1, 3);
    CHECK(zi_side_set(&g_a, k1, &a) && zi_side_set(&g_b, k1, &b));
    CHECK(zi_side_find(&g_a, k1, &r) && rec_is(&r, k1, 2) && zi_side_find(&g_b, k1, &r) && rec_is(&r, k1, 3));
    zi_side_drop(&g_a, k1);
    CHECK(!zi_side_find(&g_a, k1, &r) && zi_side_find(&g_b, k1, &r) && rec_is(&r, k1, 3));
    zi_side_drop(&g_b, k1);
    CHECK(!zi_side_find(&g_b, k1, &r));
    printf("instances: one key in two tables, two records, dropped one by one\n");

    threads_case();
    printf("ok\n");
    return 0;
}
