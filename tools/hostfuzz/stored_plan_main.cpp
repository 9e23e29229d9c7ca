// zpack_amd/csrc/stored_plan.h, the header the codec compiles, under ASan + UBSan: which stored entries of a device-resident call go
// chip-wide (every guard failed once, the lengths at which the block and group counts change), the span table (rows, destination
// offsets, part_base, the group count, a launch that is full) and the verdict as a table.  Built and run by tools/hostfuzz/run_stored_plan.sh
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "stored_plan.h"
using namespace zpk;

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static const u64 ARCHIVE = (1ull << 33) + 4096, DST = (1ull << 33) + 8192;

static zpk_decode_desc good(u64 len)
{
    zpk_decode_desc d; memset(&d, 0, sizeof(d));
    d.src_offset = 10; d.comp_size = len; d.uncomp_size = len; d.expect_hash = 0x1122334455667788ull;
    d.dst_offset = 257; d.dst_capacity = len; d.method = ZPK_METHOD_NONE;
    return d;
}
// the rule, stated once more
static bool want(const zpk_decode_desc& d, u64 archive, u64 dst, u64 threshold)
{
    const u64 least = threshold > 1025 ? threshold : 1025;
    return d.method == 0 && d.comp_size != 0 && d.dst_capacity >= d.uncomp_size && d.src_offset <= archive && d.comp_size < archive - d.src_offset &&
           d.uncomp_size <= d.comp_size && d.dst_offset <= dst && d.uncomp_size <= dst - d.dst_offset && d.uncomp_size >= least;
}

int main()
{
    const u64 lens[] = { 1024, 1025, 2048, 2049, 65536, 65537, 66560, 66561, 0xFFFFFFFFull, (1ull << 32) + 1025 };
    const u64 nlens = sizeof(lens) / sizeof(lens[0]);

    // ---- the rule ----
    u64 taken = 0, asked = 0;
    const u64 thresholds[] = { 1, 1025, 1026, 65537, 256u << 10, ~0ull };
    for (u64 th : thresholds) for (u64 len : lens) {
        const zpk_decode_desc d = good(len);
        const bool t = stored_span_takes(d, ARCHIVE, DST, th);
        CHECK(t == want(d, ARCHIVE, DST, th));
        CHECK(t == (len >= 1025 && len >= th));
        asked++; taken += t;
    }
    CHECK(!stored_span_takes(good(1024), ARCHIVE, DST, 1) && stored_span_takes(good(1025), ARCHIVE, DST, 1));       // no full block: no group to carry the tail
    CHECK(!stored_span_takes(good(1000), ARCHIVE, DST, 0) && stored_span_takes(good(1025), ARCHIVE, DST, 0));
    u64 failed = 0;
    {   // every guard failed once, and the last value that passes it
        const u64 L = 300u << 10, TH = 256u << 10;
        zpk_decode_desc d = good(L);
        CHECK(stored_span_takes(d, ARCHIVE, DST, TH));
        d = good(L); d.method = ZPK_METHOD_LZ4; CHECK(!stored_span_takes(d, ARCHIVE, DST, TH)); failed++;
        d = good(L); d.method = ZPK_METHOD_ZSTD; CHECK(!stored_span_takes(d, ARCHIVE, DST, TH));
        d = good(L); d.method = 3; CHECK(!stored_span_takes(d, ARCHIVE, DST, TH));
        d = good(L); d.comp_size = 0; d.uncomp_size = 0; d.dst_capacity = 0; CHECK(!stored_span_takes(d, ARCHIVE, DST, 1)); failed++;
        d = good(L); d.comp_size = 0; CHECK(!stored_span_takes(d, ARCHIVE, DST, TH));
        d = good(L); d.dst_capacity = L - 1; CHECK(!stored_span_takes(d, ARCHIVE, DST, TH)); failed++;
        d = good(L); d.dst_capacity = L + 1; CHECK(stored_span_takes(d, ARCHIVE, DST, TH));
        d = good(L); d.src_offset = ARCHIVE + 1; CHECK(!stored_span_takes(d, ARCHIVE, DST, TH)); failed++;
        d = good(L); d.src_offset = ~0ull - 5; CHECK(!stored_span_takes(d, ARCHIVE, DST, TH));                      // (no wrap)
        d = good(L); d.src_offset = ARCHIVE; CHECK(!stored_span_takes(d, ARCHIVE, DST, TH));
        d = good(L); d.src_offset = ARCHIVE - L; CHECK(!stored_span_takes(d, ARCHIVE, DST, TH)); failed++;          // ends where the archive ends
        d = good(L); d.src_offset = ARCHIVE - L - 1; CHECK(stored_span_takes(d, ARCHIVE, DST, TH));
        d = good(L); d.comp_size = ~0ull; CHECK(!stored_span_takes(d, ARCHIVE, DST, TH));
        d = good(L); d.uncomp_size = L + 1; d.dst_capacity = L + 1; CHECK(!stored_span_takes(d, ARCHIVE, DST, TH)); failed++;
        d = good(L); d.comp_size = L + 5; CHECK(stored_span_takes(d, ARCHIVE, DST, TH));                             // trailing bytes in the archive are not copied
        d = good(L); d.dst_offset = DST - L + 1; CHECK(!stored_span_takes(d, ARCHIVE, DST, TH)); failed++;           // the slot reaches past dst_size
        d = good(L); d.dst_offset = DST - L; CHECK(stored_span_takes(d, ARCHIVE, DST, TH));
        d = good(L); d.dst_offset = DST + 1; CHECK(!stored_span_takes(d, ARCHIVE, DST, TH));
        d = good(L); d.dst_offset = ~0ull; CHECK(!stored_span_takes(d, ARCHIVE, DST, TH));
        d = good(L); CHECK(!stored_span_takes(d, ARCHIVE, DST, L + 1)); failed++;                                    // below the threshold
        d = good(L); CHECK(stored_span_takes(d, ARCHIVE, DST, L) && !stored_span_takes(d, ARCHIVE, DST, ~0ull));
        d = good(L); d.flags = ZPK_DF_SKIP_HASH | ZPK_DF_GENERAL; CHECK(stored_span_takes(d, ARCHIVE, DST, TH));     // the flags do not matter
    }
    printf("rule: %llu of %llu entries taken over the lengths and thresholds, %llu guards failed once each: exactly by the rule\n",
           (unsigned long long)taken, (unsigned long long)asked, (unsigned long long)failed);

    // ---- the table ----
    CHECK(xxh3_span_blocks(1025) == 64 && xxh3_span_blocks(65536) == 64 && xxh3_span_blocks(65537) == 64 && xxh3_span_blocks(66560) == 64 &&
          xxh3_span_blocks(66561) == 128 && xxh3_span_blocks(0xFFFFFFFFull) == (1u << 22) && xxh3_span_blocks((1ull << 32) + 1025) == (1u << 22) + 64);
    {
        std::vector<StoredSpanRow> rows(nlens + 1);
        std::vector<u64> dst(nlens + 1);
        memset(&rows[nlens - 1], 0xA5, 2 * sizeof(StoredSpanRow)); dst[nlens - 1] = dst[nlens] = 0xA5A5A5A5A5A5A5A5ull;   // (1024 is not taken: nlens - 1 rows are written)
        const StoredSpanRow guard = rows[nlens];
        StoredPlan p = { 0, 0, 0 };
        u64 src_at = 10, dst_at = 3, want_groups = 0, n = 0;
        std::vector<zpk_decode_desc> in;
        for (u64 len : lens) {
            zpk_decode_desc d = good(len); d.src_offset = src_at; d.dst_offset = dst_at;
            src_at += len + 1; dst_at += len + 7;
            if (!stored_span_takes(d, ~0ull, ~0ull, 1)) { CHECK(len == 1024); continue; }
            const u64 nblocks = (len - 1) >> 10;
            CHECK(nblocks >= 1);
            want_groups += (nblocks + 63) / 64;
            CHECK(stored_span_emit(d, rows.data(), dst.data(), p));
            in.push_back(d); n++;
            CHECK(p.nspans == n && p.groups == want_groups && p.part_blocks == 64 * want_groups);
        }
        CHECK(n == nlens - 1);
        CHECK(memcmp(&rows[n], &guard, sizeof(guard)) == 0 && dst[n] == 0xA5A5A5A5A5A5A5A5ull);                     // nothing behind the last row
        u64 next = 0;
        for (u64 k = 0; k < n; k++) {
            CHECK(rows[k].off == in[k].src_offset && rows[k].len == in[k].uncomp_size && dst[k] == in[k].dst_offset);
            CHECK(rows[k].part_base == next && rows[k].part_base % 64 == 0);                                         // ascending, multiples of 64, disjoint, no gap
            const u64 nblocks = (rows[k].len - 1) >> 10;
            next = rows[k].part_base + xxh3_span_blocks(rows[k].len);
            CHECK(next >= rows[k].part_base + nblocks && next - rows[k].part_base - nblocks < 64);                   // room for every block, less than a group to spare
            // group g of the launch belongs to the LAST span with part_base / 64 <= g (the search of k_stored_span): the span's own groups, no other
            for (u64 g : { rows[k].part_base / 64, next / 64 - 1 }) {
                u64 lo = 0, hi = n;
                while (hi - lo > 1) { const u64 mid = (lo + hi) >> 1; if (rows[mid].part_base / 64 <= g) lo = mid; else hi = mid; }
                CHECK(lo == k && (g - rows[k].part_base / 64) * 64 < nblocks);
            }
        }
        CHECK(next == p.part_blocks && p.groups == want_groups && p.groups == 6 * 1 + 2 + 65536 + 65537);
        printf("table: %llu spans, %llu groups: rows and destination offsets as given, part_base ascending in multiples of 64 and disjoint\n",
               (unsigned long long)p.nspans, (unsigned long long)p.groups);
    }
    {   // a launch that is full: the entry is not written, the plan stays as it was
        StoredSpanRow rows[4]; u64 dst[4];
        memset(rows, 0xA5, sizeof(rows));
        StoredPlan p = { 0, 0, 0 };
        CHECK(stored_span_emit(good(66561), rows, dst, p, 3) && p.groups == 2);
        const StoredSpanRow before = rows[1];
        CHECK(!stored_span_emit(good(66561), rows, dst, p, 3) && p.nspans == 1 && p.groups == 2 && p.part_blocks == 128);
        CHECK(memcmp(&rows[1], &before, sizeof(before)) == 0);
        CHECK(stored_span_emit(good(65537), rows, dst, p, 3) && p.nspans == 2 && p.groups == 3 && rows[1].part_base == 128);
        CHECK(!stored_span_emit(good(1025), rows, dst, p, 3) && p.nspans == 2);
        StoredPlan q = { 0, 0, 0 };
        CHECK(!stored_span_emit(good(66561), rows, dst, q, 1) && q.nspans == 0 && q.groups == 0);
        StoredPlan full = { ZPK_STORED_MAX_SPANS, 0, 0 };
        CHECK(!stored_span_emit(good(1025), rows, dst, full));
        StoredPlan brim = { 1, (ZPK_STORED_MAX_GROUPS - 1) * 64, ZPK_STORED_MAX_GROUPS - 1 };
        CHECK(stored_span_emit(good(1025), rows, dst, brim) && brim.groups == ZPK_STORED_MAX_GROUPS && !stored_span_emit(good(1025), rows, dst, brim));
        printf("full: an entry whose groups do not fit the launch is left out, nothing written, the plan unchanged\n");
    }

    // ---- the verdict ----
    {
        zpk_decode_desc d = good(300u << 10);
        zpk_decode_result r = stored_span_verdict(d, d.expect_hash);
        CHECK(r.status == 0 && r.detail == 0 && r.produced == d.uncomp_size && r.hash == d.expect_hash);
        r = stored_span_verdict(d, d.expect_hash ^ 1);
        CHECK(r.status == 15 && r.detail == 0 && r.produced == d.uncomp_size && r.hash == (d.expect_hash ^ 1));
        d.flags = ZPK_DF_SKIP_HASH;
        r = stored_span_verdict(d, d.expect_hash ^ 1);
        CHECK(r.status == 0 && r.detail == 0 && r.produced == d.uncomp_size && r.hash == (d.expect_hash ^ 1));
        d.flags = ZPK_DF_GENERAL; d.comp_size += 5;
        r = stored_span_verdict(d, d.expect_hash ^ 1);
        CHECK(r.status == 15 && r.produced == d.uncomp_size);
        printf("verdict: OK, hash mismatch, hash mismatch skipped; detail 0, produced = uncomp_size, the hash as computed\n");
    }
    return 0;
}
