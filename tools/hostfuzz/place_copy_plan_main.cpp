// zpack_amd/csrc/place_copy_plan.h, the header the codec compiles, under ASan + UBSan: the pitch of a placed read, its rule, the extent,
// the row table of k_place_copy and the placed offset of a place in an item.  Every item is walked the way the kernel walks it (wc_item
// with PITCHED, row_copy.h) — the groups and the loose bytes of window_piece, each at place_dst_of — against a byte-by-byte model:
//   place_valid and place_extent against the model's own arithmetic in 128 bits, at pitches and row counts whose products need more
//     than 32 bits and at the wrap;
//   the items of a row write every placed byte once, no gap byte, nothing outside the extent, and every byte is the map of the header;
//   in place, with the items in either order, no item reads a base byte that another item has written;
//   the overlap rule: base == dst, or the two extents disjoint.
// Built and run by tools/hostfuzz/run_place_copy_plan.sh
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "place_copy_plan.h"
using namespace zpk;

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static u8 pattern(u64 i) { return (u8)(i * 131 + (i >> 8) * 7 + (i >> 16) * 3 + 1); }
static u8 base_pattern(u64 i) { return (u8)(i * 29 + (i >> 7) * 13 + 101); }
static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// ---- the model of the rule: the extent in 128 bits ----
typedef unsigned __int128 u128m;
static bool model_valid(u64 n, u32 k, const Window& w, u64 p, u64* extent)
{
    if (p == 0 || !window_valid(n, k, w) || p < w.cols) return false;
    u128m e = 0;
    if (w.rows != 0 && w.cols != 0) e = (u128m)(w.rows - 1) * p + w.cols;
    if (e > (u128m)~0ull) return false;
    *extent = (u64)e;
    return true;
}
static void rule_case(u64 n, u32 k, const Window& w, u64 p)
{
    u64 e = 0;
    const bool want = model_valid(n, k, w, p, &e);
    CHECK(place_valid(n, k, w, p) == want);
    if (want) CHECK(place_extent(w, p) == e);
}

struct Walk { u64 items = 0, bytes = 0; };
// One row walked item by item: `stored` the n stored bytes, dst and base of extent bytes (base may BE dst, or NULL).
static Walk run_row(u64 n, u32 k, const Window& w, u64 pitch, const u8* stored, u8* dst, const u8* base, bool reverse_items)
{
    PlaceCopyRow rows[1];
    CopyPlan p = { 0, 0 };
    CHECK(place_copy_emit((u64)stored, (u64)dst, (u64)base, n, w, pitch, k, rows, p));
    const u64 len = window_bytes(w), ext = place_extent(w, pitch);
    CHECK(p.nrows == (len ? 1u : 0u) && p.items == copy_items(len));
    Walk out;
    out.items = p.items; out.bytes = len;
    std::vector<long long> written_by(ext, -1);
    const u64 m = n / k;
    u64 covered = 0;
    for (u64 tt = 0; tt < p.items; tt++) {
        const u64 t = reverse_items ? p.items - 1 - tt : tt;
        CHECK(copy_row_of(rows, p.nrows, t) == 0);
        const PlaceCopyRow& r = rows[0];
        CHECK(r.src == (u64)stored && r.dst == (u64)dst && r.base == (u64)base && r.n == n && r.len == len && r.elem == k && r.item_base == 0 && r.pitch == pitch);
        CHECK(r.row_bytes == w.row_bytes && r.row0 == w.row0 && r.col0 == w.col0 && r.cols == w.cols);
        const WindowPiece P = window_piece(len, w.cols, k, t);
        CHECK((u64)P.groups * 16u * k + P.loose == P.to - P.from);
        covered += P.to - P.from;
        auto one = [&](u64 o, u64 d, u64 i) {
            CHECK(d >= P.from && d < P.to);                                                                     // the window byte is the item's own
            CHECK(o == place_offset(w, pitch, d) && o < ext && o % pitch < w.cols);                             // the map as the header states it; inside the extent; no gap byte
            CHECK(i == window_plain_index(w, d) && i < n);
            CHECK(written_by[o] < 0);                                                                           // once — and, in place, nobody has written base[o] when it is read
            dst[o] = delta_byte(stored[plane_stored_index(n, k, i)], base ? base[o] : 0);
            written_by[o] = (long long)t;
        };
        for (u32 G = 0; G < P.groups; G++) {
            const WindowAt a = window_group_at(P, k, G);
            const u64 o = place_dst_of(P, pitch, a), d = window_dst_of(P, w.cols, a), i = window_plain_of(P, w.row_bytes, w.row0, w.col0, a);
            CHECK(a.col + 16u * k <= w.cols && i % k == 0);                                                     // a group lies in ONE window row: its 16 * k placed bytes are contiguous
            const u64 e = i / k;
            for (u32 pl = 0; pl < k; pl++) {
                CHECK(pl * m + e + 16 <= n);
                for (u32 x = 0; x < 16; x++) one(o + x * k + pl, d + x * k + pl, i + x * k + pl);
            }
        }
        for (u32 B = 0; B < P.loose; B++) {
            const WindowAt a = window_loose_at(P, k, B);
            CHECK(a.col < w.cols);
            one(place_dst_of(P, pitch, a), window_dst_of(P, w.cols, a), window_plain_of(P, w.row_bytes, w.row0, w.col0, a));
        }
    }
    CHECK(covered == len);
    for (u64 o = 0; o < ext; o++) CHECK((written_by[o] >= 0) == (o % pitch < w.cols));                          // every placed byte, no gap byte
    return out;
}

static Walk totals;
static u64 cases = 0;
static void geometry(u32 k, u64 nrows, u64 row_elems, u64 row0, u64 rows, u64 col0e, u64 colse, u64 gap)
{
    const Window w = { row_elems * k, row0, rows, col0e * k, colse * k };
    const u64 n = nrows * w.row_bytes, len = window_bytes(w), pitch = w.cols + gap;
    if (pitch == 0) return;
    CHECK(place_valid(n, k, w, pitch));
    const u64 ext = place_extent(w, pitch);
    CHECK(ext >= len && (len == 0) == (ext == 0));
    std::vector<u8> stored(n), base(ext), expect(ext, 0xEE), got(ext, 0xEE);
    for (u64 j = 0; j < n; j++) stored[j] = pattern(j);
    for (u64 o = 0; o < ext; o++) base[o] = base_pattern(o);
    // the byte-by-byte model: window byte d at (d / cols) * pitch + d % cols
    for (u64 d = 0; d < len; d++) expect[(d / w.cols) * pitch + d % w.cols] = stored[plane_stored_index(n, k, (w.row0 + d / w.cols) * w.row_bytes + w.col0 + d % w.cols)];
    const Walk a = run_row(n, k, w, pitch, stored.data(), got.data(), nullptr, false);
    CHECK(got == expect);                                                                                       // the gaps kept their canaries
    std::vector<u8> xored = base, ckpt;
    for (u64 d = 0; d < len; d++) { const u64 o = (d / w.cols) * pitch + d % w.cols; xored[o] = expect[o] ^ base[o]; }
    got = base;
    for (u64 o = 0; o < ext; o++) if (o % pitch >= w.cols) got[o] = 0xDD, xored[o] = 0xDD;                       // (a destination apart from the base: its gaps are its own)
    run_row(n, k, w, pitch, stored.data(), got.data(), base.data(), true);
    CHECK(got == xored);
    for (u64 o = 0; o < ext; o++) if (o % pitch >= w.cols) xored[o] = base[o];                                  // in place the gaps are the base's, untouched
    for (int rev = 0; rev < 2; rev++) { ckpt = base; run_row(n, k, w, pitch, stored.data(), ckpt.data(), ckpt.data(), rev != 0); CHECK(ckpt == xored); }
    cases++; totals.items += a.items; totals.bytes += a.bytes;
}

int main()
{
    // ---- the rule ----
    {
        const Window ok = { 64, 1, 2, 8, 16 };
        CHECK(place_valid(256, 4, ok, 16) && place_extent(ok, 16) == 32 && place_valid(256, 4, ok, 17) && place_extent(ok, 17) == 33);
        CHECK(!place_valid(256, 4, ok, 15) && !place_valid(256, 4, ok, 0));                                     // rows that run into each other; no pitch
        CHECK(!place_valid(256, 4, Window{ 64, 3, 2, 8, 16 }, 64) && !place_valid(256, 4, Window{ 0, 0, 0, 0, 0 }, 64));      // the window's own rule
        CHECK(place_valid(256, 4, Window{ 64, 1, 0, 8, 16 }, 16) && place_extent(Window{ 64, 1, 0, 8, 16 }, 16) == 0);        // no rows
        CHECK(place_valid(256, 4, Window{ 64, 1, 2, 8, 0 }, 1) && place_extent(Window{ 64, 1, 2, 8, 0 }, ~0ull) == 0);        // no columns: any pitch but 0
        CHECK(place_valid(256, 4, Window{ 64, 1, 2, 8, 0 }, ~0ull) && !place_valid(256, 4, Window{ 64, 1, 2, 8, 0 }, 0));
        CHECK(place_valid(256, 4, Window{ 64, 1, 1, 8, 16 }, ~0ull) && place_extent(Window{ 64, 1, 1, 8, 16 }, ~0ull) == 16); // one row: the pitch multiplies nothing
        // products past 32 bits, and the wrap: 2^33 rows of 8 bytes in an entry of 2^36 (nothing is allocated: the rule alone)
        const Window tall = { 8, 0, 1ull << 33, 0, 8 };
        const u64 n36 = 1ull << 36;
        CHECK(place_valid(n36, 8, tall, 1ull << 20) && place_extent(tall, 1ull << 20) == ((1ull << 33) - 1) * (1ull << 20) + 8);
        const u64 edge = (~0ull - 8) / ((1ull << 33) - 1);                                                      // the largest pitch whose extent fits
        CHECK(edge == 1ull << 31 && place_valid(n36, 8, tall, edge) && place_extent(tall, edge) == ~0ull - (1ull << 31) + 9 && !place_valid(n36, 8, tall, edge + 1));
        CHECK(!place_valid(n36, 8, tall, ~0ull) && !place_valid(n36, 8, tall, 1ull << 40));
        const Window two = { 8, 0, 2, 0, 8 };
        CHECK(place_valid(16, 8, two, ~0ull - 8) && place_extent(two, ~0ull - 8) == ~0ull && !place_valid(16, 8, two, ~0ull - 7) && !place_valid(16, 8, two, ~0ull));
        for (int it = 0; it < 200000; it++) {
            const u32 k = 1u << (rnd() % 4);
            const u64 colse = rnd() % 5, rows = it % 3 ? rnd() >> (rnd() % 64) : rnd() % 4;
            const u64 row_bytes = (colse + rnd() % 3) * k;
            if (row_bytes == 0 || rows > ~0ull / row_bytes) continue;
            const Window w = { row_bytes, 0, rows, 0, colse * k };
            const u64 p = it % 5 == 0 ? w.cols + rnd() % 3 - 1 : rnd() >> (rnd() % 64);
            rule_case(rows * row_bytes, k, w, p);
            if (rows > 1 && w.cols) {                                                                           // ... and right at the wrap of this window
                const u64 e = (~0ull - w.cols) / (rows - 1);
                rule_case(rows * row_bytes, k, w, e); rule_case(rows * row_bytes, k, w, e + 1); rule_case(rows * row_bytes, k, w, e - 1);
            }
        }
        PlaceCopyRow one[1]; memset(one, 0xA5, sizeof(one));
        const PlaceCopyRow before = one[0];
        CopyPlan p = { 0, 0 };
        CHECK(!place_copy_emit(1, 2, 3, 256, ok, 15, 4, one, p) && !place_copy_emit(1, 2, 3, 256, ok, 0, 4, one, p) && place_copy_emit(1, 2, 3, 256, Window{ 64, 1, 0, 8, 16 }, 16, 4, one, p));
        CHECK(p.nrows == 0 && p.items == 0 && memcmp(one, &before, sizeof(before)) == 0);
        CopyPlan full = { ZPK_COPY_MAX_ROWS, 5 };
        CHECK(!place_copy_emit(1, 2, 3, 256, ok, 16, 4, one, full) && memcmp(one, &before, sizeof(before)) == 0);
        PlaceCopyRow tworows[2];
        CopyPlan q = { 0, 0 };
        CHECK(place_copy_emit(1, 2, 0, 1 << 20, Window{ 1 << 10, 0, 1 << 10, 0, 32 }, 1ull << 34, 2, tworows, q) && place_copy_emit(4, 5, 6, 256, ok, 24, 4, tworows, q));
        CHECK(q.nrows == 2 && q.items == 3 && tworows[1].item_base == 2 && tworows[0].pitch == 1ull << 34 && tworows[1].pitch == 24 && tworows[1].len == 32);
        // the placed offset in 64 bits: row 2^22 of an item's rows at a pitch of 2^34 lies past 2^56
        WindowPiece P = window_piece(1ull << 15, 32, 2, 0); P.r0 = (1ull << 22) - 1;
        CHECK(place_dst_of(P, 1ull << 34, WindowAt{ 1u, 7 }) == (1ull << 56) + 7);
        // the overlap rule: over the EXTENT (ok at pitch 24: 40 bytes), not over the window's 32 bytes
        CHECK(place_overlap_ok(100, 100, ok, 24) && place_overlap_ok(100, 140, ok, 24) && place_overlap_ok(140, 100, ok, 24));
        CHECK(!place_overlap_ok(100, 139, ok, 24) && !place_overlap_ok(139, 100, ok, 24) && !place_overlap_ok(100, 132, ok, 24) && !place_overlap_ok(100, 101, ok, 24));
        CHECK(place_overlap_ok(100, 101, Window{ 64, 1, 0, 8, 16 }, 24));                                       // no bytes: anywhere
        printf("rule: every clause of place_valid against a 128-bit model, products past 32 bits and pitches at the wrap; rows as given, none for no bytes; overlap over the extent\n");
    }
    // ---- the edges ----
    for (u32 k : { 1u, 2u, 4u, 8u }) {
        const u64 pe = 16384 / k;                                                                               // elements per item
        for (u64 colse : { (u64)1, (u64)15, (u64)16, (u64)17, (u64)64 * 16, (u64)65 * 16, pe - 1, pe, pe + 1 })
            for (u64 rows : { 1, 2, 3, 70 }) {
                if (rows == 70 && colse > 65 * 16) rows = 5;
                for (u64 gap : { (u64)0, (u64)1, (u64)k, (u64)16 * k, colse * k, (u64)4099 })
                    for (u64 col0e : { 0, 15 }) geometry(k, rows + 1, col0e + colse + (col0e ? 3 : 0), 1, rows, col0e, colse, gap);
            }
        geometry(k, 4, 32, 4, 0, 0, 32, 5); geometry(k, 4, 32, 1, 2, 32, 0, 7);                                 // placements of no bytes
    }
    const u64 edge_cases = cases;
    // ---- randomized ----
    for (int it = 0; it < 500; it++) {
        const u32 k = 1u << (rnd() % 4);
        const u64 row_elems = 1 + rnd() % (it % 8 == 0 ? 40000 : 700), nrows = 1 + rnd() % (it % 8 == 0 ? 6 : 90);
        const u64 col0e = rnd() % row_elems, colse = rnd() % (row_elems - col0e + 1), row0 = rnd() % nrows, rows = rnd() % (nrows - row0 + 1);
        geometry(k, nrows, row_elems, row0, rows, col0e, colse, it % 4 == 0 ? 0 : rnd() % (it % 3 ? 40 : 5000));
    }
    printf("items: %llu edge and %llu random geometries (k in 1, 2, 4, 8; gaps of 0, 1, k, 16k, cols, 4099 and random), each without a base, with one, and in place with the "
           "items in either order: every placed byte written once, no gap byte, nothing outside the extent, every byte the map (%llu items, %llu bytes)\n",
           (unsigned long long)edge_cases, (unsigned long long)(cases - edge_cases), (unsigned long long)totals.items, (unsigned long long)totals.bytes);
    return 0;
}
