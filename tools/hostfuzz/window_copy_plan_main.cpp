// zpack_amd/csrc/window_copy_plan.h, the header the codec compiles, under ASan + UBSan: the window, its rule, the row table of
// k_window_copy and what an item covers.  Every item is walked the way the kernel walks it (wc_item, row_copy.h) — the groups of 16
// elements inside one window row against 16 bytes in each plane, the loose bytes through the map, both numbered through the whole item —
// over edge and randomized geometries:
//   the items tile [0, window_bytes) exactly once;
//   every source index lies in [0, n), and no two destination bytes read the same stored byte;
//   every byte is the map of the header, and the window whole is join_k;
//   in place, with the items in either order, no item reads a base byte that another item has written.
// Built and run by tools/hostfuzz/run_window_copy_plan.sh
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "window_copy_plan.h"
using namespace zpk;

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static u8 pattern(u64 i) { return (u8)(i * 131 + (i >> 8) * 7 + (i >> 16) * 3 + 1); }
static u8 base_pattern(u64 i) { return (u8)(i * 29 + (i >> 7) * 13 + 101); }
static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

struct Walk { u64 items = 0, wide = 0, bytes = 0; };
// One row walked item by item: `stored` the n stored bytes, dst and base of window size (base may BE dst, or NULL).
static Walk run_row(u64 n, u32 k, const Window& w, const u8* stored, u8* dst, const u8* base, bool reverse_items)
{
    WindowCopyRow rows[1];
    CopyPlan p = { 0, 0 };
    CHECK(window_copy_emit((u64)stored, (u64)dst, (u64)base, n, w, k, rows, p));
    const u64 len = window_bytes(w);
    CHECK(p.nrows == (len ? 1u : 0u) && p.items == copy_items(len));
    Walk out;
    out.items = p.items; out.bytes = len;
    const bool inplace = base && base == dst;
    std::vector<long long> written_by(len, -1);
    std::vector<u8> src_seen(n, 0);
    const u64 m = n / k;
    u64 covered = 0;
    for (u64 tt = 0; tt < p.items; tt++) {
        const u64 t = reverse_items ? p.items - 1 - tt : tt;
        CHECK(copy_row_of(rows, p.nrows, t) == 0);
        const WindowCopyRow& r = rows[0];
        CHECK(r.src == (u64)stored && r.dst == (u64)dst && r.base == (u64)base && r.n == n && r.len == len && r.elem == k && r.item_base == 0);
        CHECK(r.row_bytes == w.row_bytes && r.row0 == w.row0 && r.col0 == w.col0 && r.cols == w.cols);
        const WindowPiece P = window_piece(len, w.cols, k, t);
        CHECK(P.from < P.to && P.to <= len && P.from % ZPK_COPY_PIECE == 0 && P.to - P.from <= ZPK_COPY_PIECE);
        CHECK((u64)P.groups * 16u * k + P.loose == P.to - P.from);                                              // groups and loose bytes make up the item
        covered += P.to - P.from;
        auto one = [&](u64 d, u64 i) {
            CHECK(d >= P.from && d < P.to);                                                                     // the item stays inside its own destination range, base included
            CHECK(i == window_plain_index(w, d) && i < n);                                                      // the map as the header states it
            const u64 j = plane_stored_index(n, k, i);
            CHECK(j < n && !src_seen[j] && written_by[d] < 0);                                                  // inside the entry; no stored byte twice; no destination byte twice
            if (inplace) CHECK(written_by[d] < 0);                                                              // nobody has written base[d] when it is read
            src_seen[j] = 1;
            dst[d] = delta_byte(stored[j], base ? base[d] : 0);
            written_by[d] = (long long)t;
        };
        for (u32 G = 0; G < P.groups; G++) {
            const WindowAt a = window_group_at(P, k, G);
            const u64 d = window_dst_of(P, w.cols, a), i = window_plain_of(P, w.row_bytes, w.row0, w.col0, a);
            CHECK(a.col + 16u * k <= w.cols && i % k == 0);                                                     // a group lies in ONE window row and begins on an element
            const u64 e = i / k;
            for (u32 pl = 0; pl < k; pl++) {
                CHECK(pl * m + e + 16 <= n);                                                                    // the 16-byte load of plane pl
                for (u32 x = 0; x < 16; x++) { CHECK(plane_stored_index(n, k, i + x * k + pl) == pl * m + e + x); one(d + x * k + pl, i + x * k + pl); }
            }
        }
        out.wide += (u64)P.groups * 16u * k;
        for (u32 B = 0; B < P.loose; B++) {
            const WindowAt a = window_loose_at(P, k, B);
            CHECK(a.col < w.cols);
            one(window_dst_of(P, w.cols, a), window_plain_of(P, w.row_bytes, w.row0, w.col0, a));
        }
    }
    CHECK(covered == len);
    for (u64 d = 0; d < len; d++) CHECK(written_by[d] >= 0);                                                    // the items tile [0, window_bytes)
    return out;
}

static Walk totals;
static u64 cases = 0;
static void geometry(u32 k, u64 nrows, u64 row_elems, u64 row0, u64 rows, u64 col0e, u64 colse)
{
    const Window w = { row_elems * k, row0, rows, col0e * k, colse * k };
    const u64 n = nrows * w.row_bytes, len = window_bytes(w);
    CHECK(window_valid(n, k, w));
    std::vector<u8> stored(n), base(len), expect(len), got(len, 0xEE);
    for (u64 j = 0; j < n; j++) stored[j] = pattern(j);
    for (u64 d = 0; d < len; d++) { base[d] = base_pattern(d); expect[d] = stored[plane_stored_index(n, k, window_plain_index(w, d))]; }
    const Walk a = run_row(n, k, w, stored.data(), got.data(), nullptr, false);
    CHECK(got == expect);
    std::vector<u8> xored(len), ckpt;
    for (u64 d = 0; d < len; d++) xored[d] = expect[d] ^ base[d];
    std::fill(got.begin(), got.end(), 0xDD);
    run_row(n, k, w, stored.data(), got.data(), base.data(), true);
    CHECK(got == xored);
    for (int rev = 0; rev < 2; rev++) { ckpt = base; run_row(n, k, w, stored.data(), ckpt.data(), ckpt.data(), rev != 0); CHECK(ckpt == xored); }
    cases++; totals.items += a.items; totals.wide += a.wide; totals.bytes += a.bytes;
}

int main()
{
    // ---- the rule ----
    {
        const Window ok = { 64, 1, 2, 8, 16 };
        CHECK(window_valid(256, 4, ok) && window_bytes(ok) == 32);
        CHECK(!window_valid(256, 4, Window{ 0, 0, 0, 0, 0 }));                                                  // no window is no valid window
        CHECK(!window_valid(250, 1, Window{ 64, 0, 1, 0, 8 }));                                                 // a tail
        CHECK(!window_valid(256, 4, Window{ 64, 1, 2, 6, 16 }) && !window_valid(256, 4, Window{ 64, 1, 2, 8, 18 }) && !window_valid(252, 4, Window{ 42, 0, 1, 0, 8 }));
        CHECK(!window_valid(256, 4, Window{ 64, 1, 2, 52, 16 }) && window_valid(256, 4, Window{ 64, 1, 2, 48, 16 }));
        CHECK(!window_valid(256, 4, Window{ 64, 3, 2, 8, 16 }) && window_valid(256, 4, Window{ 64, 2, 2, 8, 16 }) && !window_valid(256, 4, Window{ 64, 5, 0, 8, 16 }));
        CHECK(!window_valid(256, 4, Window{ 64, 1, 2, ~0ull - 3, 8 }) && !window_valid(256, 4, Window{ 64, ~0ull, 2, 8, 16 }) && !window_valid(256, 4, Window{ 64, 2, ~0ull, 8, 16 }));
        CHECK(!window_valid(256, 4, Window{ 64, 1, 2, 8, ~0ull - 3 }));
        for (u32 k : { 0u, 3u, 5u, 16u }) CHECK(!window_valid(240, k, Window{ 240, 0, 1, 0, 240 }));
        CHECK(window_valid(256, 4, Window{ 64, 4, 0, 64, 0 }) && window_bytes(Window{ 64, 4, 0, 64, 0 }) == 0); // the empty window at the far corner
        CHECK(window_valid(0, 2, Window{ 64, 0, 0, 0, 64 }));                                                   // an entry of no bytes: no rows
        WindowCopyRow one[1]; memset(one, 0xA5, sizeof(one));
        const WindowCopyRow before = one[0];
        CopyPlan p = { 0, 0 };
        CHECK(!window_copy_emit(1, 2, 3, 256, Window{ 64, 3, 2, 8, 16 }, 4, one, p) && window_copy_emit(1, 2, 3, 256, Window{ 64, 1, 0, 8, 16 }, 4, one, p));
        CHECK(p.nrows == 0 && p.items == 0 && memcmp(one, &before, sizeof(before)) == 0);
        CopyPlan full = { ZPK_COPY_MAX_ROWS, 5 };
        CHECK(!window_copy_emit(1, 2, 3, 256, ok, 4, one, full) && memcmp(one, &before, sizeof(before)) == 0);
        WindowCopyRow two[2];
        CopyPlan q = { 0, 0 };
        CHECK(window_copy_emit(1, 2, 0, 1 << 20, Window{ 1 << 10, 0, 1 << 10, 0, 32 }, 2, two, q) && window_copy_emit(4, 5, 6, 256, ok, 4, two, q));
        CHECK(q.nrows == 2 && q.items == 3 && two[1].item_base == 2 && two[0].base == 0 && two[1].len == 32);
        CHECK(copy_row_of(two, 2, 1) == 0 && copy_row_of(two, 2, 2) == 1);
        CHECK(window_overlap_ok(100, 100, ok) && window_overlap_ok(100, 132, ok) && !window_overlap_ok(100, 131, ok) && !window_overlap_ok(131, 100, ok));
        printf("rule: every clause of window_valid, wrap-around included; rows as given, none for the empty window; overlap over window_bytes\n");
    }
    // ---- the edges ----
    for (u32 k : { 1u, 2u, 4u, 8u }) {
        const u64 pe = 16384 / k;                                                                               // elements per item
        for (u64 colse : { (u64)1, (u64)15, (u64)16, (u64)17, (u64)63 * 16, (u64)64 * 16, (u64)65 * 16, pe - 1, pe, pe + 1 })
            for (u64 rows : { 1, 2, 3, 70 }) {
                if (rows == 70 && colse > 65 * 16) rows = 5;                                                    // (70 rows of an item each: no new path, a megabyte per walk)
                for (u64 col0e : { 0, 1, 15, 16 })
                    for (int wider = 0; wider < 2; wider++) {
                        if (!wider && col0e) continue;
                        const u64 row_elems = wider ? col0e + colse + 3 : colse;
                        for (u64 row0 : { 0, 1 }) geometry(k, rows + row0 + (wider ? 1 : 0), row_elems, row0, rows, col0e, colse);
                    }
            }
        geometry(k, 4, 32, 4, 0, 0, 32); geometry(k, 4, 32, 1, 2, 32, 0);                                       // windows of no bytes
    }
    const u64 edge_cases = cases;
    // ---- the window whole is join_k ----
    for (u32 k : { 1u, 2u, 4u, 8u })
        for (u64 elems : { (u64)1, (u64)16, (u64)1025, (u64)16384 / k + 17, (u64)3 * 16384 + 5 })
            for (u64 nrows : { 1, 3 }) {
                const u64 n = elems * k * nrows;
                const Window w = { elems * k, 0, nrows, 0, elems * k };
                std::vector<u8> stored(n), got(n, 0xEE);
                for (u64 j = 0; j < n; j++) stored[j] = pattern(j);
                run_row(n, k, w, stored.data(), got.data(), nullptr, false);
                for (u64 i = 0; i < n; i++) CHECK(got[i] == stored[plane_stored_index(n, k, i)]);
            }
    // ---- randomized ----
    for (int it = 0; it < 600; it++) {
        const u32 k = 1u << (rnd() % 4);
        const u64 row_elems = 1 + rnd() % (it % 8 == 0 ? 40000 : 700), nrows = 1 + rnd() % (it % 8 == 0 ? 6 : 90);
        const u64 col0e = rnd() % row_elems, colse = rnd() % (row_elems - col0e + 1), row0 = rnd() % nrows, rows = rnd() % (nrows - row0 + 1);
        geometry(k, nrows, row_elems, row0, rows, col0e, colse);
    }
    printf("items: %llu edge and %llu random geometries (k in 1, 2, 4, 8), each without a base, with one, and in place with the items in either order: "
           "the items tile the window once, every source index lies inside the entry, no stored byte is read twice, every byte is the map, the window whole is the join\n",
           (unsigned long long)edge_cases, (unsigned long long)(cases - edge_cases));
    CHECK(totals.wide * 2 > totals.bytes);
    printf("wide path: more than half of the window bytes walked\n");
    return 0;
}
