// zpack_amd/csrc/span_copy_plan.h, the header the codec compiles, under ASan + UBSan: the row table of k_span_copy (rows as given, a span
// of no bytes takes none, item_base ascending and disjoint, every item found by the kernel's search), the launches of a table that
// exceeds one grid, the staging slots of a sub-batch, the offsets of the packed read and the pointer test.
// Built and run by tools/hostfuzz/run_span_copy_plan.sh
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "span_copy_plan.h"
using namespace zpk;

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

int main()
{
    // ---- the rows ----
    const u64 lens[] = { 0, 1, 16383, 16384, 16385, (1ull << 32) + 5 };
    const u64 want_items[] = { 0, 1, 1, 1, 2, (1ull << 18) + 1 };
    const u64 nlens = sizeof(lens) / sizeof(lens[0]);
    std::vector<SpanCopyRow> rows(nlens + 1);
    memset(rows.data(), 0xA5, rows.size() * sizeof(SpanCopyRow));
    const SpanCopyRow guard = rows[nlens];
    CopyPlan p = { 0, 0 };
    std::vector<u64> in_src, in_dst, in_len;
    u64 src_at = 0x7f0000000003ull, dst_at = 0x7e000000000dull, items = 0;
    for (u64 k = 0; k < nlens; k++) {
        CHECK(copy_items(lens[k]) == want_items[k]);
        const CopyPlan before = p;
        CHECK(span_copy_emit(src_at, dst_at, lens[k], rows.data(), p));
        if (lens[k] == 0) CHECK(p.nrows == before.nrows && p.items == before.items);               // no row, no item
        else { in_src.push_back(src_at); in_dst.push_back(dst_at); in_len.push_back(lens[k]); items += want_items[k]; }
        CHECK(p.nrows == in_len.size() && p.items == items);
        src_at += lens[k] + 1; dst_at += lens[k] + 64;
    }
    CHECK(p.nrows == nlens - 1 && p.items == 1 + 1 + 1 + 2 + (1ull << 18) + 1);
    CHECK(memcmp(&rows[p.nrows], &guard, sizeof(guard)) == 0 && memcmp(&rows[nlens], &guard, sizeof(guard)) == 0);      // nothing behind the last row
    for (u64 k = 0; k < p.nrows; k++) CHECK(rows[k].src == in_src[k] && rows[k].dst == in_dst[k] && rows[k].len == in_len[k]);
    CHECK(copy_items(~0ull) == (1ull << 50));                                                 // (nothing wraps)
    printf("rows: %llu spans of the lengths 0, 1, 16383, 16384, 16385, 2^32 + 5 are %llu rows and %llu items: rows as given, none for the empty span\n",
           (unsigned long long)nlens, (unsigned long long)p.nrows, (unsigned long long)p.items);

    // ---- item_base ----
    u64 next = 0, searched = 0;
    for (u64 k = 0; k < p.nrows; k++) {
        CHECK(rows[k].item_base == next);                                                          // ascending, disjoint, no gap
        const u64 n = copy_items(rows[k].len);
        CHECK(n >= 1 && (n - 1) * ZPK_COPY_PIECE < rows[k].len && rows[k].len <= n * ZPK_COPY_PIECE);  // the last item holds 1..16384 bytes
        next += n;
        for (u64 t : { rows[k].item_base, rows[k].item_base + n / 2, next - 1 }) { CHECK(copy_row_of(rows.data(), p.nrows, t) == k); searched++; }
    }
    CHECK(next == p.items);
    {   // a full table takes no further row
        SpanCopyRow one[1]; memset(one, 0xA5, sizeof(one));
        const SpanCopyRow before = one[0];
        CopyPlan full = { ZPK_COPY_MAX_ROWS, 77 };
        CHECK(!span_copy_emit(1, 2, 3, one, full) && full.nrows == ZPK_COPY_MAX_ROWS && full.items == 77 && memcmp(one, &before, sizeof(before)) == 0);
        CHECK(span_copy_emit(1, 2, 0, one, full));
    }
    printf("item_base: ascending and disjoint without a gap, %llu items searched for land in their own rows\n", (unsigned long long)searched);

    // ---- the launches ----
    {
        CHECK(copy_launches(0) == 0 && copy_launches(1) == 1 && copy_launches(ZPK_COPY_MAX_ITEMS) == 1 && copy_launches(ZPK_COPY_MAX_ITEMS + 1) == 2);
        CopyLaunch L = copy_launch(ZPK_COPY_MAX_ITEMS, 0);
        CHECK(L.item0 == 0 && L.items == ZPK_COPY_MAX_ITEMS && L.grid == 0x7FFFFFFFu);
        L = copy_launch(ZPK_COPY_MAX_ITEMS + 1, 0);
        CHECK(L.item0 == 0 && L.items == ZPK_COPY_MAX_ITEMS && L.grid == 0x7FFFFFFFu);
        L = copy_launch(ZPK_COPY_MAX_ITEMS + 1, 1);
        CHECK(L.item0 == ZPK_COPY_MAX_ITEMS && L.items == 1 && L.grid == 1);
        L = copy_launch(5, 0);
        CHECK(L.item0 == 0 && L.items == 5 && L.grid == 2);
        // a small grid limit: the launches tile the items exactly, each grid holds its items and fewer than four to spare
        const u64 total = p.items, cap = 1000;
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

    // ---- the staging slots ----
    CHECK(span_copy_read_slot(true, 100, 300) == 256 && span_copy_read_slot(false, 100, 300) == 512 && span_copy_read_slot(true, 300, 100) == 256 &&
          span_copy_read_slot(false, 0, 0) == 0 && span_copy_read_slot_bytes(true, 256, 256) == 256 && span_copy_read_slot(false, 1, 257) == 512);
    CHECK(span_copy_write_slot(0) == 256 && span_copy_write_slot(240) == 256 && span_copy_write_slot(241) == 512 && span_copy_write_slot(65536) == 65536 + 256);
    for (u64 n : { 0ull, 1ull, 239ull, 240ull, 241ull, 65535ull, 65536ull, (2ull << 20) + 17 }) CHECK(span_copy_write_slot(n) >= n + 16 && span_copy_write_slot(n) % 256 == 0 && span_copy_write_slot(n) < n + 16 + 256);
    printf("slots: read slots hold what the entry may produce, write slots the source and 16 bytes, both at multiples of 256\n");

    // ---- the descriptor of a staged entry ----
    {
        struct Desc { u64 src_offset, comp_size, uncomp_size, expect_hash, dst_offset, dst_capacity; uint32_t method, flags; };   // (the fields of zpk_decode_desc)
        const Desc d = { 11, 22, 100, 0x1234, 999, 300, 2, 1 };
        auto same_but = [&](const Desc& s, u64 off, u64 cap) {
            return s.src_offset == d.src_offset && s.comp_size == d.comp_size && s.uncomp_size == d.uncomp_size && s.expect_hash == d.expect_hash &&
                   s.method == d.method && s.flags == d.flags && s.dst_offset == off && s.dst_capacity == cap;
        };
        CHECK(same_but(span_copy_staged_desc(d, false, 512), 512, 300));                           // a compressed entry: the caller's capacity
        CHECK(same_but(span_copy_staged_desc(d, true, 0), 0, 100));                                // a stored entry that fits: cut to uncomp_size, its slot
        Desc e = d; e.dst_capacity = 100;
        CHECK(span_copy_staged_desc(e, true, 256).dst_capacity == 100 && span_copy_staged_desc(e, true, 256).dst_offset == 256);      // exactly as large
        e.dst_capacity = 99;
        CHECK(span_copy_staged_desc(e, true, 256).dst_capacity == 99 && span_copy_staged_desc(e, false, 256).dst_capacity == 99);     // too small: as given, the device's guard judges it
        e.uncomp_size = 0; e.dst_capacity = 0;
        CHECK(span_copy_staged_desc(e, true, 768).dst_capacity == 0 && span_copy_staged_desc(e, true, 768).dst_offset == 768);
        for (u64 cap : { 0ull, 99ull, 100ull, 101ull, ~0ull })                                     // what is kept never exceeds the slot's bytes
            { Desc f = d; f.dst_capacity = cap; if (cap >= f.uncomp_size) CHECK(span_copy_staged_desc(f, true, 0).dst_capacity == span_copy_read_slot_bytes(true, f.uncomp_size, cap)); }
        printf("staged: the caller's descriptor at its slot's offset; a stored entry that fits is cut to uncomp_size, every other capacity stays\n");
    }

    // ---- the packed read ----
    {
        const u64 sizes[] = { 0, 1, 255, 256, 257 };
        const u64 want[] = { 0, 0, 256, 512, 768 }, end = 1280;
        u64 pos = 0;
        for (u64 k = 0; k < 5; k++) { CHECK(pos == want[k]); pos = span_copy_packed_next(pos, sizes[k]); }
        CHECK(pos == end);
        CHECK(span_copy_packed_stride(0) == 0 && span_copy_packed_stride(1) == 256 && span_copy_packed_stride(256) == 256 && span_copy_packed_stride(257) == 512);
        CHECK(span_copy_packed_next(~0ull - 300, 1024) == (~0ull & ~255ull) && span_copy_packed_next(512, ~0ull) == (~0ull & ~255ull) &&
              span_copy_packed_next(~0ull & ~255ull, 0) == (~0ull & ~255ull));                     // saturates, never wraps
        printf("packed: uncomp_size 0, 1, 255, 256, 257 land at 0, 0, 256, 512, 768 and end at 1280\n");
    }

    // ---- the pointer test ----
    {
        const u64 base = 0x7f1200000000ull, size = 1u << 20;
        CHECK(span_copy_in_range(base, 1, base, size) && span_copy_in_range(base, size, base, size) && !span_copy_in_range(base, size + 1, base, size));
        CHECK(!span_copy_in_range(base - 1, 1, base, size) && !span_copy_in_range(base - 1, 2, base, size));
        CHECK(span_copy_in_range(base + size - 1, 1, base, size) && !span_copy_in_range(base + size - 1, 2, base, size));
        CHECK(!span_copy_in_range(base + size, 1, base, size) && !span_copy_in_range(base + size + 1, 1, base, size));
        CHECK(!span_copy_in_range(base + 16, ~0ull, base, size) && !span_copy_in_range(base + 16, ~0ull - base - 15, base, size));     // ptr + len wraps to 0 / past it
        CHECK(!span_copy_in_range(~0ull, 2, base, size) && !span_copy_in_range(0, 1, base, size));
        CHECK(span_copy_in_range(0, 0, base, size) && span_copy_in_range(base + size + 5, 0, base, size));                              // no bytes: nothing is touched
        CHECK(span_copy_in_range(~0ull - 7, 8, ~0ull - 15, 16) && !span_copy_in_range(~0ull - 7, 9, ~0ull - 15, 16));                    // an allocation at the top of the address space
        printf("range: the first and the last byte of an allocation pass, one before and one behind do not, ptr + len that wraps does not\n");
    }
    return 0;
}
