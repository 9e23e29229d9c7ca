// zpack_amd/csrc/plane_copy_plan.h, the header the codec compiles, under ASan + UBSan: the layout of a byte-plane entry, the row table of
// k_plane_copy, its work items and the launches of a table that exceeds one grid.  Every item is walked the way the kernel walks it —
// whole groups of 16 elements against 16 bytes in each plane, the rest byte by byte through the index map —: split is a permutation of
// [0, n), join inverts it, and the items tile the bytes once.
// `dump`: prints "k n <hex of the stored side>" for plain[i] = (i * 131 + (i >> 8) * 7 + 1) & 255 and every (k, n) of the list, for a
// model of the layout to compare with (tests/test_plane_copy_plan_cpu.py).
// Built and run by tools/hostfuzz/run_plane_copy_plan.sh
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "plane_copy_plan.h"
using namespace zpk;

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static std::vector<u64> sizes_of(u32 k)
{
    return { 0, 1, (u64)k - 1, k, (u64)k + 1, 16ull * k - 1, 16ull * k + 1, 1024ull * k - 1, 1024ull * k + 1, 16383, 16385, 3ull * 16384 + 5 };
}
static u8 pattern(u64 i) { return (u8)(i * 131 + (i >> 8) * 7 + 1); }

// One row of n bytes with element size k, its items walked as k_plane_copy walks them (pc_item, row_copy.h).  to_stored[i] = where plain
// byte i goes; every plain and every stored byte is touched exactly once.
static std::vector<u64> walk_row(u64 n, u32 k, u64* wide_bytes)
{
    PlaneCopyRow rows[3];
    CopyPlan p = { 0, 0 };
    CHECK(plane_copy_emit(0x1000, 0x2000, 0, k, PLANE_SPLIT, rows, p) && p.nrows == 0 && p.items == 0);      // no bytes: no row, no item
    CHECK(plane_copy_emit(0x7f0000000003ull, 0x7e000000000dull, n, k, PLANE_SPLIT, rows, p));
    CHECK(p.nrows == (n ? 1u : 0u) && p.items == copy_items(n));
    std::vector<u64> to_stored(n, ~0ull);
    std::vector<u8> plain_seen(n, 0), stored_seen(n, 0);
    const u64 m = n / k;
    u64 next_from = 0;
    for (u64 t = 0; t < p.items; t++) {
        CHECK(copy_row_of(rows, p.nrows, t) == 0);
        const PlanePiece P = plane_piece(n, k, t - rows[0].item_base);
        CHECK(P.from == next_from && P.from < P.to && P.to <= n && P.to - P.from <= ZPK_COPY_PIECE);         // the items tile [0, n) in order
        CHECK(P.from % (16u * k) == 0 && P.from <= P.wide_end && P.wide_end <= P.to && (P.wide_end - P.from) % (16u * k) == 0);
        CHECK(P.wide_end <= m * k && P.to - P.wide_end < 16u * k + k);                                     // whole elements only; the rest is short
        CHECK(t + 1 == p.items ? P.to == n : P.to == P.from + ZPK_COPY_PIECE);
        next_from = P.to;
        const u64 groups = (P.wide_end - P.from) / (16u * k), e0 = P.from / k;
        for (u64 g = 0; g < groups; g++)                                                                   // the wide path: 16 * k plain bytes, 16 bytes per plane
            for (u32 pl = 0; pl < k; pl++)
                for (u32 e = 0; e < 16; e++) {
                    const u64 i = P.from + (g * 16 + e) * k + pl, j = pl * m + e0 + g * 16 + e;
                    CHECK(i < P.wide_end && j < n && j == plane_stored_index(n, k, i));
                    CHECK(!plain_seen[i] && !stored_seen[j]);
                    plain_seen[i] = stored_seen[j] = 1; to_stored[i] = j;
                }
        *wide_bytes += P.wide_end - P.from;
        for (u64 i = P.wide_end; i < P.to; i++) {                                                          // byte by byte
            const u64 j = plane_stored_index(n, k, i);
            CHECK(j < n && !plain_seen[i] && !stored_seen[j]);
            plain_seen[i] = stored_seen[j] = 1; to_stored[i] = j;
        }
    }
    CHECK(next_from == n);
    for (u64 i = 0; i < n; i++) CHECK(plain_seen[i] && stored_seen[i]);                                    // a permutation of [0, n)
    return to_stored;
}

int main(int argc, char** argv)
{
    const bool dump = argc > 1 && strcmp(argv[1], "dump") == 0;
    // ---- the element sizes ----
    for (u32 k = 0; k < 300; k++) CHECK(plane_elem_valid(k) == (k == 1 || k == 2 || k == 4 || k == 8));
    {
        PlaneCopyRow one[1]; memset(one, 0xA5, sizeof(one));
        const PlaneCopyRow before = one[0];
        CopyPlan p = { 0, 0 };
        for (u32 k : { 0u, 3u, 5u, 6u, 7u, 9u, 16u }) CHECK(!plane_copy_emit(1, 2, 64, k, 0, one, p) && !plane_copy_emit(1, 2, 0, k, 0, one, p));
        CHECK(p.nrows == 0 && p.items == 0 && memcmp(one, &before, sizeof(before)) == 0);
        CopyPlan full = { ZPK_COPY_MAX_ROWS, 77 };
        CHECK(!plane_copy_emit(1, 2, 3, 2, 0, one, full) && full.nrows == ZPK_COPY_MAX_ROWS && full.items == 77 && memcmp(one, &before, sizeof(before)) == 0);
    }
    // ---- the layout, item by item ----
    u64 cases = 0, wide = 0, bytes = 0;
    for (u32 k : { 1u, 2u, 4u, 8u })
        for (u64 n : sizes_of(k)) {
            const std::vector<u64> to_stored = walk_row(n, k, &wide);
            const u64 m = n / k;
            std::vector<u8> plain(n), stored(n), back(n);
            for (u64 i = 0; i < n; i++) plain[i] = pattern(i);
            for (u64 i = 0; i < n; i++) stored[to_stored[i]] = plain[i];                                   // split
            for (u64 i = 0; i < n; i++) back[i] = stored[to_stored[i]];                                    // join
            CHECK(back == plain);
            for (u32 p = 0; p < k; p++) for (u64 j = 0; j < m; j++) CHECK(stored[p * m + j] == plain[j * k + p]);      // the layout as the header states it
            for (u64 t = k * m; t < n; t++) CHECK(stored[t] == plain[t]);
            if (k == 1) CHECK(stored == plain);
            if (dump) { printf("%u %llu ", k, (unsigned long long)n); for (u64 i = 0; i < n; i++) printf("%02x", stored[i]); printf("\n"); }
            cases++; bytes += n;
        }
    if (dump) return 0;
    printf("layout: %llu rows (k in 1, 2, 4, 8; n around k, 16 k, 1024 k, one piece and three): split is a permutation, join inverts it, the items tile the bytes once; %llu of %llu bytes take the wide path\n",
           (unsigned long long)cases, (unsigned long long)wide, (unsigned long long)bytes);

    // ---- rows and item_base ----
    {
        const u64 lens[] = { 0, 1, 16383, 16384, 16385, (1ull << 32) + 5 };
        const u64 want_items[] = { 0, 1, 1, 1, 2, (1ull << 18) + 1 };
        std::vector<PlaneCopyRow> rows(7);
        memset(rows.data(), 0xA5, rows.size() * sizeof(PlaneCopyRow));
        const PlaneCopyRow guard = rows[6];
        CopyPlan p = { 0, 0 };
        u64 next = 0, searched = 0;
        for (u64 q = 0; q < 6; q++) { CHECK(copy_items(lens[q]) == want_items[q]); CHECK(plane_copy_emit(100 + q, 200 + q, lens[q], 1u << (q % 4), q & 1, rows.data(), p)); }
        CHECK(p.nrows == 5 && p.items == 1 + 1 + 1 + 2 + (1ull << 18) + 1 && memcmp(&rows[5], &guard, sizeof(guard)) == 0);
        for (u64 r = 0; r < p.nrows; r++) {
            CHECK(rows[r].item_base == next && rows[r].src == 101 + r && rows[r].dst == 201 + r && rows[r].len == lens[r + 1]);
            CHECK(rows[r].elem == (1u << ((r + 1) % 4)) && rows[r].join == ((r + 1) & 1));
            const u64 n = copy_items(rows[r].len);
            next += n;
            for (u64 t : { rows[r].item_base, rows[r].item_base + n / 2, next - 1 }) { CHECK(copy_row_of(rows.data(), p.nrows, t) == r); searched++; }
        }
        CHECK(next == p.items && copy_items(~0ull) == (1ull << 50));
        // the last piece of a long row: its tail stays, whatever lies in front is whole groups
        const PlanePiece last = plane_piece((1ull << 32) + 5, 8, 1ull << 18);
        CHECK(last.from == (1ull << 32) && last.wide_end == last.from && last.to == last.from + 5);
        printf("rows: as given with element size and direction, none for the empty row; item_base ascending without a gap, %llu items searched for land in their rows\n", (unsigned long long)searched);
    }

    // ---- the launches ----
    {
        CHECK(copy_launches(0) == 0 && copy_launches(1) == 1 && copy_launches(ZPK_COPY_MAX_ITEMS) == 1 && copy_launches(ZPK_COPY_MAX_ITEMS + 1) == 2);
        CopyLaunch L = copy_launch(ZPK_COPY_MAX_ITEMS + 1, 0);
        CHECK(L.item0 == 0 && L.items == ZPK_COPY_MAX_ITEMS && L.grid == 0x7FFFFFFFu);
        L = copy_launch(ZPK_COPY_MAX_ITEMS + 1, 1);
        CHECK(L.item0 == ZPK_COPY_MAX_ITEMS && L.items == 1 && L.grid == 1);
        const u64 total = 262150, cap = 1000;
        u64 at = 0;
        const u64 nl = copy_launches(total, cap);
        for (u64 j = 0; j < nl; j++) {
            L = copy_launch(total, j, cap);
            CHECK(L.item0 == at && L.items >= 1 && L.items <= cap && (u64)L.grid * 4 >= L.items && (u64)L.grid * 4 < L.items + 4);
            at += L.items;
        }
        CHECK(at == total && nl == (total + cap - 1) / cap);
        printf("launches: one grid holds %llu items, one more is a second launch of 1; %llu items at 1000 a grid are %llu launches that tile them\n",
               (unsigned long long)ZPK_COPY_MAX_ITEMS, (unsigned long long)total, (unsigned long long)nl);
    }
    return 0;
}
