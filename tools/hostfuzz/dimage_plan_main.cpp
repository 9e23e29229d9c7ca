// zpack_amd/csrc/dimage_plan.h, the header the codec compiles, under ASan + UBSan: the sub-batches of a batch read out of an archive image
// in device memory (zpk_codec_decode_batch_dimage) — the slot of an entry, where the slots of a sub-batch lie, where a sub-batch ends —
// on fixed cases whose lines tests/test_device_image_cpu.py asserts, and on random batches against a restatement in 128-bit sums.
// Built and run by tools/hostfuzz/run_dimage_plan.sh
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "dimage_plan.h"
using namespace zpk;

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)
typedef unsigned __int128 u128;

struct Sub { u64 first, count, total; };

// every sub-batch of slots[0, n) at `chunk`, with the properties that hold for each: the offsets ascend in multiples of 256 without a
// gap, the total is their sum, it fits the chunk unless the sub-batch is ONE entry, and the entry behind it would not have fitted
static std::vector<Sub> cut_all(const std::vector<u64>& slots, u64 chunk, u64 max_entries = ZPK_DIMAGE_MAX_ENTRIES)
{
    const u64 n = slots.size();
    auto slot = [&](u64 i) { return slots[i]; };
    std::vector<Sub> out;
    std::vector<u64> at(n + 1, 0xA5A5A5A5A5A5A5A5ull);
    for (u64 first = 0; first < n; ) {
        const DimageCut c = dimage_cut(first, n, chunk, slot, at.data() + first, max_entries);
        const DimageCut again = dimage_cut(first, n, chunk, slot, nullptr, max_entries);      // at = nullptr: the same cut
        CHECK(c.count >= 1 && c.count <= max_entries && first + c.count <= n && again.count == c.count && again.out_total == c.out_total);
        u128 sum = 0;
        for (u64 k = 0; k < c.count; k++) { CHECK(at[first + k] == (u64)sum && at[first + k] % 256 == 0); sum += slots[first + k]; }
        CHECK(sum == (u128)c.out_total);
        CHECK(c.count == 1 || sum <= (u128)chunk);
        if (first + c.count < n && c.count < max_entries) CHECK(sum + slots[first + c.count] > (u128)chunk);
        if (first + c.count < n) CHECK(at[first + c.count] == 0xA5A5A5A5A5A5A5A5ull);        // nothing written behind the sub-batch
        out.push_back(Sub{ first, c.count, c.out_total });
        first += c.count;
    }
    CHECK(at[n] == 0xA5A5A5A5A5A5A5A5ull);
    return out;
}

static std::string list_of(const std::vector<Sub>& s, int what)
{
    std::string t;
    for (size_t k = 0; k < s.size(); k++) { char b[40]; snprintf(b, sizeof(b), "%s%llu", k ? ", " : "", (unsigned long long)(what ? s[k].total : s[k].count)); t += b; }
    return t;
}

int main()
{
    // ---- the slots ----
    const u64 caps[] = { 0, 1, 255, 256, 257, 65536, 300u << 10 };
    std::vector<u64> slots;
    std::string slot_list;
    for (u64 cap : caps) {
        const u64 s = dimage_slot(false, cap, cap);
        CHECK(s == span_copy_read_slot(false, cap, cap) && s >= cap && s < cap + 256 && s % 256 == 0);
        slots.push_back(s);
        char b[40]; snprintf(b, sizeof(b), "%s%llu", slot_list.empty() ? "" : ", ", (unsigned long long)s); slot_list += b;
    }
    CHECK(dimage_slot(true, 100, 300) == 256 && dimage_slot(false, 100, 300) == 512 && dimage_slot(true, 300, 100) == 256);      // a stored entry: uncomp_size, when it fits
    printf("slots: capacities 0, 1, 255, 256, 257, 65536, 307200 take %s bytes of staging\n", slot_list.c_str());

    // ---- the cuts ----
    CHECK(dimage_chunk(0) == ZPK_HOST_CHUNK_BYTES && dimage_chunk(1) == 1 && dimage_chunk(1u << 20) == (1u << 20));
    {
        const std::vector<Sub> a = cut_all(slots, 64u << 10), b = cut_all(slots, 1u << 20), d = cut_all(slots, dimage_chunk(0));
        printf("cuts: at a chunk of 65536 they are %llu sub-batches of %s entries and %s bytes\n", (unsigned long long)a.size(), list_of(a, 0).c_str(), list_of(a, 1).c_str());
        printf("cuts: at a chunk of 1048576 they are %llu of %s entries and %s bytes, at the default of %llu bytes %llu of %s entries and %s bytes\n",
               (unsigned long long)b.size(), list_of(b, 0).c_str(), list_of(b, 1).c_str(), (unsigned long long)dimage_chunk(0),
               (unsigned long long)d.size(), list_of(d, 0).c_str(), list_of(d, 1).c_str());
    }
    {   // an entry above the chunk goes alone, wherever it stands; one that fills the chunk exactly does not close it early
        const std::vector<u64> s = { 256, 70000 * 256ull, 256, 256, 65536 - 512, 256 };
        const std::vector<Sub> a = cut_all(s, 64u << 10);
        CHECK(a.size() == 4 && a[0].count == 1 && a[1].count == 1 && a[1].total == 70000 * 256ull && a[2].count == 3 && a[2].total == 65536 && a[3].count == 1);
        printf("alone: a slot of %llu bytes at a chunk of 65536 is a sub-batch of its own between its neighbours (%s entries)\n", (unsigned long long)s[1], list_of(a, 0).c_str());
    }
    {   // no entries, entries without bytes, the cap on the entries of one sub-batch
        auto none = [](u64) -> u64 { abort(); };
        const DimageCut c = dimage_cut(0, 0, 65536, none);
        CHECK(c.count == 0 && c.out_total == 0);
        const std::vector<u64> zeros(1000, 0);
        const std::vector<Sub> a = cut_all(zeros, 0), b = cut_all(zeros, 65536, 300);
        CHECK(a.size() == 1 && a[0].count == 1000 && a[0].total == 0);
        CHECK(b.size() == 4 && b[0].count == 300 && b[3].count == 100);
        printf("empty: a batch of no entries is no sub-batch; 1000 entries without bytes are one, at 300 entries a sub-batch %llu\n", (unsigned long long)b.size());
    }
    {   // sums that would wrap
        CHECK(dimage_slot(false, 0, ~0ull) == ZPK_DIMAGE_SLOT_MAX && dimage_slot(false, 0, ~0ull - 254) == ZPK_DIMAGE_SLOT_MAX &&
              dimage_slot(false, 0, ~0ull - 255) == ZPK_DIMAGE_SLOT_MAX && dimage_slot(false, 0, ~0ull - 256) == ZPK_DIMAGE_SLOT_MAX &&
              dimage_slot(false, 0, ~0ull - 511) == ZPK_DIMAGE_SLOT_MAX - 256);
        CHECK(dimage_slot(true, ~0ull, ~0ull) == ZPK_DIMAGE_SLOT_MAX && dimage_slot(true, 5, ~0ull) == 256);
        const std::vector<u64> s = { ZPK_DIMAGE_SLOT_MAX, ZPK_DIMAGE_SLOT_MAX, 256, 1ull << 63, 1ull << 63, 256 };
        const std::vector<Sub> a = cut_all(s, dimage_chunk(0)), b = cut_all(s, ~0ull);
        CHECK(a.size() == 6 && a[3].count == 1 && a[3].total == (1ull << 63));                                                       // (each above the chunk: alone)
        CHECK(b.size() == 4 && b[0].count == 1 && b[1].count == 1 && b[2].count == 2 && b[2].total == (1ull << 63) + 256 && b[3].count == 2);
        printf("wrap: capacities within 255 bytes of 2^64 take the largest slot, %llu; slots of that size and of 2^63 never share a sub-batch whose sum would wrap\n",
               (unsigned long long)ZPK_DIMAGE_SLOT_MAX);
    }

    // ---- random batches against the properties of cut_all ----
    u64 x = 0x9E3779B97F4A7C15ull, batches = 0, subs = 0;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int it = 0; it < 2000; it++) {
        const u64 n = rnd() % 200;
        std::vector<u64> s(n);
        const int kind = (int)(rnd() % 4);
        for (u64 i = 0; i < n; i++) {
            const u64 r = rnd();
            const u64 cap = kind == 0 ? r % 6000 : kind == 1 ? r % (400u << 10) : kind == 2 ? (r % 8 ? r % 70000 : r) : (r % 16 ? r % 300 : ~0ull - r % 600);
            s[i] = dimage_slot(r & (1ull << 40), cap, cap + (r >> 60));
        }
        const u64 chunks[] = { 0, 1, 255, 256, 65536, 1u << 20, rnd() % (2u << 20), dimage_chunk(0), ~0ull };
        for (u64 chunk : chunks) subs += cut_all(s, chunk, it % 7 == 0 ? 1 + rnd() % 50 : ZPK_DIMAGE_MAX_ENTRIES).size();
        batches++;
    }
    printf("random: %llu batches at 9 chunks each, %llu sub-batches: offsets ascend without gaps, totals are the sums, only a single entry exceeds its chunk\n",
           (unsigned long long)batches, (unsigned long long)subs);
    return 0;
}
