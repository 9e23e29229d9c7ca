// zpack_amd/csrc/dsink_plan.h, the header the codec and the commit kernels compile, under ASan + UBSan: a batch compressed into a bounded
// sink in device memory (zpk_codec_encode_batch_dsink) — the cut, the span table and what a persistent grid copies from it, the room and
// the chaining of sub-batches, the staging slots — on fixed cases whose lines tests/test_dsink_plan_cpu.py asserts, on batches that test hands
// over (`cut ROOM STATUS:SIZE ...`), and on random batches against a restatement that walks the offsets as k_sink_cut and k_sink_place do.
// Built and run by tools/hostfuzz/run_dsink_plan.sh
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "dsink_plan.h"
using namespace zpk;

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

struct Batch { std::vector<int32_t> status; std::vector<u64> size; };

// what the pack scan leaves: offsets[0, n] over the sizes of the entries with status 0, span_first[0, n] over their spans
static void scan(const Batch& b, std::vector<u64>& offsets, std::vector<u64>& span_first)
{
    const u64 n = b.status.size();
    offsets.assign(n + 1, 0); span_first.assign(n + 1, 0);
    for (u64 i = 0; i < n; i++) {
        const u64 sz = b.status[i] == 0 ? b.size[i] : 0;
        offsets[i + 1] = offsets[i] + sz; span_first[i + 1] = span_first[i] + sink_spans(sz);
    }
}

// the cut as k_sink_cut takes it: the min over the entries that stop (sink_stops on the scanned offsets), in any order
static SinkCut kernel_cut(const Batch& b, const std::vector<u64>& offsets, u64 room)
{
    const u64 n = b.status.size();
    u64 f = n;
    for (u64 i = n; i-- > 0; ) if (sink_stops(b.status[i], offsets[i + 1], room)) f = i < f ? i : f;
    return SinkCut{ f, offsets[f] };
}

// every item of [0, span_first[f]) as k_sink_place handles it, into a sink of `room` bytes with guard bytes behind it: each byte in front
// of the cut is written exactly once with its entry's byte, nothing at or behind it
static void place_all(const Batch& b, const std::vector<u64>& offsets, const std::vector<u64>& span_first, SinkCut cut, u64 room)
{
    const u64 f = cut.placed;
    std::vector<u8> sink(room + 64, 0xA5), hits(room + 64, 0);
    const u64 items = f ? span_first[f] : 0;
    for (u64 slot = 0; slot < sink_slots(items); slot++) {                            // a wave's walk through its slot of items
    u64 t = slot * ZPK_SINK_SLOT_ITEMS;
    const u64 t_end = t + ZPK_SINK_SLOT_ITEMS < items ? t + ZPK_SINK_SLOT_ITEMS : items;
    u64 e = sink_entry_of(span_first.data(), f, t), next = span_first[e + 1];
    for (; t < t_end; t++) {
        while (t >= next) { e++; CHECK(e < f); next = span_first[e + 1]; }
        CHECK(e == sink_entry_of(span_first.data(), f, t));
        CHECK(e < f && span_first[e] <= t && t < span_first[e + 1] && b.status[e] == 0);
        const SinkSpan sp = sink_span(b.size[e], span_first[e], t);
        CHECK(sp.len > 0 && sp.len <= ZPK_SINK_SPAN && sp.from + sp.len <= b.size[e]);
        CHECK(offsets[e] + sp.from + sp.len <= cut.bytes && cut.bytes <= room);
        for (u64 k = 0; k < sp.len; k++) { sink[offsets[e] + sp.from + k] = (u8)(e * 131 + (sp.from + k) * 7); hits[offsets[e] + sp.from + k]++; }
    }
    }
    for (u64 e = 0; e < f; e++) for (u64 k = 0; k < b.size[e]; k++) CHECK(sink[offsets[e] + k] == (u8)(e * 131 + k * 7));
    for (u64 k = 0; k < cut.bytes; k++) CHECK(hits[k] == 1);
    for (u64 k = cut.bytes; k < sink.size(); k++) CHECK(hits[k] == 0 && sink[k] == 0xA5);
}

static SinkCut check_cut(const Batch& b, u64 room, bool place)
{
    std::vector<u64> offsets, span_first;
    scan(b, offsets, span_first);
    const SinkCut a = sink_cut(b.status.data(), b.size.data(), b.status.size(), room), k = kernel_cut(b, offsets, room);
    CHECK(a.placed == k.placed && a.bytes == k.bytes && a.bytes <= room && a.placed <= b.status.size());
    if (place) place_all(b, offsets, span_first, a, room);
    return a;
}

int main(int argc, char** argv)
{
    // `cut ROOM STATUS:SIZE ...`: the cut of one batch, "placed bytes" (what tests/test_dsink_plan_cpu.py compares its own model with)
    if (argc >= 3 && strcmp(argv[1], "cut") == 0) {
        Batch b;
        const u64 room = strtoull(argv[2], nullptr, 10);
        for (int i = 3; i < argc; i++) {
            char* colon = nullptr;
            b.status.push_back((int32_t)strtol(argv[i], &colon, 10));
            CHECK(colon && *colon == ':');
            b.size.push_back(strtoull(colon + 1, nullptr, 10));
        }
        const SinkCut c = check_cut(b, room, room <= (1u << 22));
        printf("%llu %llu\n", (unsigned long long)c.placed, (unsigned long long)c.bytes);
        return 0;
    }
    // ---- the cut: the fixed list tests/test_dsink_plan_cpu.py restates ----
    {
        const Batch ok = { { 0, 0, 0, 0, 0 }, { 100, 0, 16384, 16385, 7 } };                 // 32876 bytes in all
        const Batch bad0 = { { 14, 0, 0 }, { 0, 5, 6 } }, bad_last = { { 0, 0, 12 }, { 5, 6, 0 } }, bad_mid = { { 0, 19, 0, 0 }, { 9, 0, 9, 9 } };
        const u64 rooms[] = { 32876, 32875, 0, 100, 99, 16484, 16483, 1u << 20 };
        printf("cut:");
        for (u64 room : rooms) { const SinkCut c = check_cut(ok, room, true); printf(" %llu:%llu/%llu", (unsigned long long)room, (unsigned long long)c.placed, (unsigned long long)c.bytes); }
        printf("\n");
        const SinkCut a = check_cut(bad0, 1000, true), b = check_cut(bad_last, 1000, true), c = check_cut(bad_last, 10, true), d = check_cut(bad_mid, 1000, true), e = check_cut(bad_mid, 8, true);
        printf("failed: at 0 %llu/%llu, at the last %llu/%llu, at the last with room for one %llu/%llu, in the middle %llu/%llu, behind a file that does not fit %llu/%llu\n",
               (unsigned long long)a.placed, (unsigned long long)a.bytes, (unsigned long long)b.placed, (unsigned long long)b.bytes, (unsigned long long)c.placed, (unsigned long long)c.bytes,
               (unsigned long long)d.placed, (unsigned long long)d.bytes, (unsigned long long)e.placed, (unsigned long long)e.bytes);
        const Batch none = { {}, {} };
        const SinkCut z = check_cut(none, 0, true);
        CHECK(z.placed == 0 && z.bytes == 0);
        // sizes whose sum would wrap never pass a room
        const Batch wrap = { { 0, 0, 0 }, { ~0ull - 5, 10, 3 } };
        const SinkCut w = sink_cut(wrap.status.data(), wrap.size.data(), 3, ~0ull);
        CHECK(w.placed == 1 && w.bytes == ~0ull - 5);
        printf("wrap: two sizes whose sum passes 2^64 stop at the second, whatever the room\n");
    }

    // ---- the span table ----
    {
        CHECK(sink_spans(0) == 0 && sink_spans(1) == 1 && sink_spans(16384) == 1 && sink_spans(16385) == 2 && sink_spans(~0ull) == (~0ull >> 14) + 1);
        const SinkSpan a = sink_span(16385, 10, 11), b = sink_span(16385, 10, 12), c = sink_span(16385, 10, 9), d = sink_span(0, 4, 4);
        CHECK(a.from == 16384 && a.len == 1 && b.len == 0 && c.len == 0 && d.len == 0);
        u64 bound = 0;
        for (u64 cap : { 0ull, 1ull, 16384ull, 16385ull, 1ull << 28 }) bound = sink_items_bound(bound, cap);
        CHECK(bound == 0 + 1 + 1 + 2 + 16384 && sink_items_bound(~0ull - 1, 1u << 20) == ~0ull);
        CHECK(sink_slots(0) == 0 && sink_slots(1) == 1 && sink_slots(4) == 1 && sink_slots(5) == 2 && sink_slots(~0ull) == (~0ull >> 2) + 1);
        CHECK(sink_grid(0, 2048) == 1 && sink_grid(1, 2048) == 1 && sink_grid(16, 2048) == 1 && sink_grid(17, 2048) == 2 && sink_grid(32768, 2048) == 2048 && sink_grid(~0ull, 2048) == 2048);
        printf("spans: sizes 0, 1, 16384, 16385 are 0, 1, 1, 2 items; a ragged batch of one 256 MiB entry and 30000 of 100 bytes is %llu items in %llu slots and a grid of %u\n",
               (unsigned long long)(sink_spans(256ull << 20) + 30000), (unsigned long long)sink_slots(sink_spans(256ull << 20) + 30000), sink_grid(sink_spans(256ull << 20) + 30000, 2048));
    }

    // ---- room, chaining, staging ----
    {
        CHECK(sink_room(100, 0) == 100 && sink_room(100, 100) == 0 && sink_room(100, 101) == 0 && sink_room(~0ull, 1) == ~0ull - 1);
        SinkChain ch = { 0, 0, true };
        sink_chain(ch, 5, SinkCut{ 5, 1000 }); CHECK(ch.open && ch.placed == 5 && ch.bytes == 1000);
        sink_chain(ch, 3, SinkCut{ 3, 0 }); CHECK(ch.open && ch.placed == 8 && ch.bytes == 1000);
        sink_chain(ch, 4, SinkCut{ 1, 17 }); CHECK(!ch.open && ch.placed == 9 && ch.bytes == 1017);
        CHECK(sink_slot(0) == 0 && sink_slot(1) == 256 && sink_slot(256) == 256 && sink_slot(257) == 512 && sink_slot(~0ull) == ZPK_DIMAGE_SLOT_MAX && sink_slot(~0ull - 255) == ZPK_DIMAGE_SLOT_MAX);
        CHECK(sink_src_slot(0) == 256 && sink_src_slot(240) == 256 && sink_src_slot(241) == 512 && sink_src_slot(~0ull) == ZPK_DIMAGE_SLOT_MAX && sink_src_slot(ZPK_DIMAGE_SLOT_MAX - 256) == ZPK_DIMAGE_SLOT_MAX - 256 + 256);
        printf("chain: sub-batches of 5, 3 and 4 entries of which the last places 1 end the call at 9 entries and 1017 bytes\n");
    }

    // ---- random batches: the two cuts agree, the items tile the bytes in front of the cut, sub-batches chained give the whole batch's cut ----
    u64 x = 0x9E3779B97F4A7C15ull, batches = 0, items = 0, chained = 0;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int it = 0; it < 3000; it++) {
        const u64 n = rnd() % 60;
        Batch b; b.status.resize(n); b.size.resize(n);
        const int kind = (int)(rnd() % 4);
        u64 total = 0;
        for (u64 i = 0; i < n; i++) {
            const u64 r = rnd();
            b.status[i] = (kind == 3 && r % 11 == 0) ? (int32_t)(12 + r % 8) : 0;
            b.size[i] = kind == 0 ? r % 300 : kind == 1 ? r % 40000 : (r % 9 ? r % 50 : 16384 * (r % 5) + (r >> 60));
            if (b.status[i]) b.size[i] = 0;                                            // (a failed entry reports no size)
            total += b.size[i];
        }
        const u64 rooms[] = { 0, 1, total, total ? total - 1 : 0, total + 1, total / 2, rnd() % (total + 2), ~0ull };
        for (u64 room : rooms) {
            const bool place = room <= total + 1;
            const SinkCut whole = check_cut(b, room, place);
            std::vector<u64> off, sf; scan(b, off, sf);
            items += whole.placed ? sf[whole.placed] : 0;
            // the same batch in sub-batches of 1 + r entries, each against the room the ones before it left
            SinkChain ch = { 0, 0, true };
            for (u64 first = 0; first < n && ch.open; ) {
                const u64 m = 1 + rnd() % 7 < n - first ? 1 + rnd() % 7 : n - first;
                const u64 cnt = m < n - first ? m : n - first;
                const SinkCut c = sink_cut(b.status.data() + first, b.size.data() + first, cnt, sink_room(room, ch.bytes));
                sink_chain(ch, cnt, c);
                first += cnt; chained++;
            }
            CHECK(ch.placed == whole.placed && ch.bytes == whole.bytes && (ch.open == (whole.placed == n)));
        }
        batches++;
    }
    printf("random: %llu batches at 8 rooms each, %llu items, %llu sub-batches: both cuts agree, the items tile the bytes in front of the cut and nothing behind it, chained sub-batches give the batch's cut\n",
           (unsigned long long)batches, (unsigned long long)items, (unsigned long long)chained);
    return 0;
}
