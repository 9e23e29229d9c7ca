// zpack_amd/csrc/delta_copy_plan.h, the header the codec compiles, under ASan + UBSan: the layout of a delta entry and the row table of
// k_delta_copy.  Every item is walked the way the kernel walks it (pc_item, row_copy.h) — whole groups of 16 elements against 16 bytes
// in each plane with the base beside the plain side, the rest byte by byte through the index map —:
//   split then join with the same base is the identity, and the stored side is split_k(plain XOR base) as the header states it;
//   the items tile the bytes of all three sides once;
//   for a join with base == dst no item reads a base byte that another item writes, so the join IN PLACE gives the same bytes.
// Built and run by tools/hostfuzz/run_delta_copy_plan.sh
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "delta_copy_plan.h"
using namespace zpk;

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static std::vector<u64> sizes_of(u32 k)
{
    return { 0, 1, (u64)k - 1, k, (u64)k + 1, 16ull * k - 1, 16ull * k + 1, 1024ull * k - 1, 1024ull * k + 1, 16383, 16385, 3ull * 16384 + 5 };
}
static u8 pattern(u64 i) { return (u8)(i * 131 + (i >> 8) * 7 + 1); }
static u8 base_pattern(u64 i) { return (u8)(i * 29 + (i >> 7) * 13 + 101); }

// One row walked item by item.  src / dst / base are the three buffers of the row (base may BE dst); owner[i] = the item that has written
// dst[i] so far (-1: none).  Every read of the base is checked against the writes of OTHER items, whichever order the items ran in.
struct Walk { u64 items = 0, wide = 0; };
static Walk run_row(u64 n, u32 k, u32 join, const u8* src, u8* dst, const u8* base, bool reverse_items)
{
    DeltaCopyRow rows[2];
    CopyPlan p = { 0, 0 };
    CHECK(delta_copy_emit(0x1000, 0x2000, 0x3000, 0, k, join, rows, p) && p.nrows == 0 && p.items == 0);       // no bytes: no row, no item
    CHECK(delta_copy_emit((u64)src, (u64)dst, (u64)base, n, k, join, rows, p));
    CHECK(p.nrows == (n ? 1u : 0u) && p.items == copy_items(n));
    Walk w;
    w.items = p.items;
    const bool inplace = base == dst;
    std::vector<long long> written_by(n, -1);                                                                 // dst byte -> item
    std::vector<u8> src_seen(n, 0), base_seen(n, 0);
    const u64 m = n / k;
    u64 covered = 0;
    for (u64 tt = 0; tt < p.items; tt++) {
        const u64 t = reverse_items ? p.items - 1 - tt : tt;
        CHECK(copy_row_of(rows, p.nrows, t) == 0);
        const DeltaCopyRow& r = rows[0];
        CHECK(r.src == (u64)src && r.dst == (u64)dst && r.base == (u64)base && r.len == n && r.elem == k && r.join == (join ? PLANE_JOIN : PLANE_SPLIT));
        const PlanePiece P = plane_piece(n, k, t - r.item_base);
        CHECK(P.from < P.to && P.to <= n && P.from % ZPK_COPY_PIECE == 0 && P.wide_end <= m * k);
        covered += P.to - P.from;
        // what the item does to plain byte i / stored byte j: reads src, reads base[i], writes dst
        auto one = [&](u64 i, u64 j) {
            CHECK(i >= P.from && i < P.to && j < n);                                                           // the base is read inside the item's own plain range
            const u64 s_at = join ? j : i, d_at = join ? i : j;
            CHECK(!src_seen[s_at] && !base_seen[i] && written_by[d_at] < 0);                                   // every byte of the three sides once
            if (inplace) CHECK(join && d_at == i);                                                             // ... and in place it is read before ITS OWN store, by no other item:
            if (inplace) CHECK(written_by[i] < 0);                                                             // nobody has written base[i] when it is read
            src_seen[s_at] = base_seen[i] = 1;
            const u8 b = base[i];
            dst[d_at] = delta_byte(src[s_at], b);
            written_by[d_at] = (long long)t;
        };
        const u64 groups = (P.wide_end - P.from) / (16u * k), e0 = P.from / k;
        for (u64 g = 0; g < groups; g++)
            for (u32 pl = 0; pl < k; pl++)
                for (u32 e = 0; e < 16; e++) {
                    const u64 i = P.from + (g * 16 + e) * k + pl, j = pl * m + e0 + g * 16 + e;
                    CHECK(i < P.wide_end && j == plane_stored_index(n, k, i));
                    one(i, j);
                }
        w.wide += P.wide_end - P.from;
        for (u64 i = P.wide_end; i < P.to; i++) one(i, plane_stored_index(n, k, i));
    }
    CHECK(covered == n);
    for (u64 i = 0; i < n; i++) CHECK(src_seen[i] && base_seen[i] && written_by[i] >= 0);                     // the items tile all three sides
    return w;
}

int main()
{
    // ---- rows ----
    {
        DeltaCopyRow one[1]; memset(one, 0xA5, sizeof(one));
        const DeltaCopyRow before = one[0];
        CopyPlan p = { 0, 0 };
        for (u32 k : { 0u, 3u, 5u, 6u, 7u, 9u, 16u }) CHECK(!delta_copy_emit(1, 2, 3, 64, k, 0, one, p) && !delta_copy_emit(1, 2, 3, 0, k, 0, one, p));
        CHECK(!delta_copy_emit(1, 2, 0, 64, 2, 0, one, p));                                                    // bytes and no base: not a row of this table
        CHECK(delta_copy_emit(1, 2, 0, 0, 2, 0, one, p));                                                      // (no bytes pass)
        CHECK(p.nrows == 0 && p.items == 0 && memcmp(one, &before, sizeof(before)) == 0);
        CopyPlan full = { ZPK_COPY_MAX_ROWS, 77 };
        CHECK(!delta_copy_emit(1, 2, 3, 4, 2, 0, one, full) && full.nrows == ZPK_COPY_MAX_ROWS && full.items == 77 && memcmp(one, &before, sizeof(before)) == 0);
        DeltaCopyRow three[3];
        CopyPlan q = { 0, 0 };
        CHECK(delta_copy_emit(10, 20, 30, 16385, 4, 1, three, q) && delta_copy_emit(11, 21, 31, 0, 4, 1, three, q) && delta_copy_emit(12, 22, 32, 5, 1, 0, three, q));
        CHECK(q.nrows == 2 && q.items == 3 && three[0].item_base == 0 && three[1].item_base == 2 && three[1].base == 32 && three[0].join == PLANE_JOIN && three[1].join == PLANE_SPLIT);
        CHECK(copy_row_of(three, 2, 0) == 0 && copy_row_of(three, 2, 1) == 0 && copy_row_of(three, 2, 2) == 1);
        printf("rows: as given with base, element size and direction; none for the empty row, none without a base; item_base ascending\n");
    }
    // ---- base against destination ----
    {
        CHECK(delta_overlap_ok(100, 100, 50) && delta_overlap_ok(100, 150, 50) && delta_overlap_ok(150, 100, 50) && delta_overlap_ok(7, 8, 0));
        CHECK(!delta_overlap_ok(100, 149, 50) && !delta_overlap_ok(149, 100, 50) && !delta_overlap_ok(100, 101, 50) && !delta_overlap_ok(101, 100, 50));
        CHECK(delta_overlap_ok(~0ull - 10, 5, 6) && !delta_overlap_ok(~0ull - 10, ~0ull - 5, 6));             // (differences, no sum that could wrap)
        printf("overlap: the same address passes, disjoint ranges pass, every partial overlap is refused\n");
    }
    // ---- the layout, item by item ----
    u64 cases = 0, wide = 0, bytes = 0;
    for (u32 k : { 1u, 2u, 4u, 8u })
        for (u64 n : sizes_of(k)) {
            const u64 m = n / k;
            std::vector<u8> plain(n), base(n), stored(n, 0xEE), back(n, 0xDD);
            for (u64 i = 0; i < n; i++) { plain[i] = pattern(i); base[i] = base_pattern(i); }
            const std::vector<u8> plain0 = plain, base0 = base;
            const Walk ws = run_row(n, k, PLANE_SPLIT, plain.data(), stored.data(), base.data(), false);
            CHECK(plain == plain0 && base == base0);                                                           // a split reads its source and its base only
            for (u32 p = 0; p < k; p++) for (u64 j = 0; j < m; j++) CHECK(stored[p * m + j] == (u8)(plain[j * k + p] ^ base[j * k + p]));     // the layout as the header states it
            for (u64 t = k * m; t < n; t++) CHECK(stored[t] == (u8)(plain[t] ^ base[t]));                     // the tail is XORed like the rest
            run_row(n, k, PLANE_JOIN, stored.data(), back.data(), base.data(), true);
            CHECK(back == plain);                                                                              // split then join with the same base: the identity
            // in place: the base buffer is the destination; items in either order
            for (int rev = 0; rev < 2; rev++) {
                std::vector<u8> ckpt = base0;
                run_row(n, k, PLANE_JOIN, stored.data(), ckpt.data(), ckpt.data(), rev != 0);
                CHECK(ckpt == plain);
            }
            if (n) { std::vector<u8> same(n); run_row(n, k, PLANE_SPLIT, plain.data(), same.data(), plain.data(), false); for (u64 i = 0; i < n; i++) CHECK(same[i] == 0); }     // base == source: all zero
            cases++; bytes += n; wide += ws.wide;
        }
    printf("layout: %llu rows (k in 1, 2, 4, 8; n around k, 16 k, 1024 k, one piece and three): stored = split(plain ^ base), join inverts it, in place too and with the items in either order; "
           "the items tile source, base and destination once; %llu of %llu bytes take the wide path\n", (unsigned long long)cases, (unsigned long long)wide, (unsigned long long)bytes);
    return 0;
}
