// zpk_layout.h — the one place that says what every word of the device counter block and every slot of the work-list storage
// is (plain C++: host code and kernels read the same names).  A batch starts by zeroing the whole counter block; the list storage
// is N_LIST_SLOTS arrays of `stride` entry indices each.
#pragma once

#define ORD_CLASSES 16                           // k_order_* / k_enc_order_*: size classes of the counting sort
#define N_ORDERED 3                              // k_order_*: grid.y = 0 Zstandard, 1 LZ4 (plain), 2 LZ4 (general)
#define N_ENC_CLASSES 3                          // k_encode<12> / <13> / <14>

namespace zpk {

// ---- list storage: which entries a kernel works on (entry indices, u32) ----
enum ListSlot : int {
    S_NONE, S_ZSTD, S_LZ4,                       // k_classify: one list per method (LZ4: plain frames that are not mostly runs)
    S_RETRY_LZ4, S_RETRY_ZSTD,                   // entries whose decoder ran out of its time budget: decoded again by the retry launches
    S_LZ4_RUNS,                                  // k_classify: LZ4 entries that are mostly runs (compressed to less than 1/8): k_lz4_left's
    S_ZSTD_ORDERED, S_LZ4_ORDERED,               // k_order_fill: S_ZSTD / S_LZ4 largest entries first
    S_LZ4_HANDED,                                // LZ4 entries k_lz4_wave handed over WITHOUT judging them (a plain header, but no clean end)
    S_LZ4_GEN, S_LZ4_GEN_ORDERED,                // k_classify: LZ4 entries whose frame header is not a plain one (k_lz4_general's), and their ordered copy
    N_LIST_SLOTS
};

// ---- counter block (u32 words) ----
enum CounterWord : int {
    // length of each list (the four k_classify fills first are brought home behind every batch: struct SeenCounts)
    C_NONE, C_ZSTD, C_LZ4, C_LZ4_GEN, C_LZ4_RUNS, C_LZ4_HANDED, C_RETRY_LZ4, C_RETRY_ZSTD,
    C_ZSTD_LEFT,                                 // Zstandard entries k_zstd_exec left to the full decoder (their list lives behind zstate)
    // dequeue heads of the persistent grids
    C_ZSTD_HEAD,                                 // k_zstd, first launch (the Zstandard list, or what k_zstd_exec left over)
    C_ZSTD_RETRY_HEAD,                           // k_zstd, retry launch
    C_FSE_HEAD, C_EXEC_HEAD,                     // k_zstd_fse, k_zstd_exec
    C_LZ4_RUNS_HEAD, C_LZ4_GEN_HEAD,             // k_lz4_left, k_lz4_general
    C_LZ4_HANDED_HEAD, C_LZ4_RETRY_HEAD,         // k_lz4_retry on the hand-over list and on the LZ4 retry list
    // the Zstandard stages' own words
    C_ZSTD_TWO_STAGE, C_ZSTD_FUSED,              // entries finished on pre-decoded sequences / by the full decoder
    C_FSE_WATCHDOG, C_FSE_BUDGET, C_FSE_MARKED,  // k_zstd_fse: rows given up by the watchdog, header-loop budget hits, entries whose sequences are in the arena
    C_EXEC_FAILED, C_EXEC_LAST_RC,               // k_zstd_exec: pre-decoded entries it could not finish, the last one's decoder code
    // largest entries first
    C_ORDER_SPAN, C_ORDER_SPAN_INV,              // largest size class and largest 15 - class among the entries that go to a decoder
    // encode batches
    C_ENC_HEAD,                                  // (N_ENC_CLASSES words) ticket queue of k_encode<12> / <13> / <14>
    C_ENC_CLASS = C_ENC_HEAD + N_ENC_CLASSES,    // (N_ENC_CLASSES words) does the batch hold entries for that instantiation at all
    C_ORDER_HIST = C_ENC_CLASS + N_ENC_CLASSES,  // [N_ORDERED lists][ORD_CLASSES] entry counts (encode batches: one list)
    C_ORDER_FILL = C_ORDER_HIST + N_ORDERED * ORD_CLASSES,   // the same again as fill cursors
    N_COUNTERS = C_ORDER_FILL + N_ORDERED * ORD_CLASSES
};

// Every owner of counter words, in order: the block is tiled by them exactly (no word has two names, none is unnamed).
struct CounterSpan { int first, words; };
constexpr CounterSpan counter_spans[] = {
    {C_NONE, 1}, {C_ZSTD, 1}, {C_LZ4, 1}, {C_LZ4_GEN, 1}, {C_LZ4_RUNS, 1}, {C_LZ4_HANDED, 1}, {C_RETRY_LZ4, 1}, {C_RETRY_ZSTD, 1}, {C_ZSTD_LEFT, 1},
    {C_ZSTD_HEAD, 1}, {C_ZSTD_RETRY_HEAD, 1}, {C_FSE_HEAD, 1}, {C_EXEC_HEAD, 1}, {C_LZ4_RUNS_HEAD, 1}, {C_LZ4_GEN_HEAD, 1}, {C_LZ4_HANDED_HEAD, 1},
    {C_LZ4_RETRY_HEAD, 1}, {C_ZSTD_TWO_STAGE, 1}, {C_ZSTD_FUSED, 1}, {C_FSE_WATCHDOG, 1}, {C_FSE_BUDGET, 1}, {C_FSE_MARKED, 1}, {C_EXEC_FAILED, 1},
    {C_EXEC_LAST_RC, 1}, {C_ORDER_SPAN, 1}, {C_ORDER_SPAN_INV, 1}, {C_ENC_HEAD, N_ENC_CLASSES}, {C_ENC_CLASS, N_ENC_CLASSES},
    {C_ORDER_HIST, N_ORDERED * ORD_CLASSES}, {C_ORDER_FILL, N_ORDERED * ORD_CLASSES},
};
constexpr bool counter_spans_tile(int total)
{
    int at = 0;
    for (const CounterSpan& s : counter_spans) { if (s.first != at || s.words <= 0) return false; at += s.words; }
    return at == total;
}
static_assert(counter_spans_tile(N_COUNTERS), "two names share a counter word, or a word has no name");
static_assert(N_COUNTERS == 128, "the counter block is 512 bytes: one memset, one copy per piece of the host pipeline");
static_assert(N_LIST_SLOTS == 11, "decode_launch sizes the list storage by N_LIST_SLOTS");

// the counter word that holds the length of a list k_classify fills
constexpr int list_count_word(int slot)
{
    return slot == S_NONE ? C_NONE : slot == S_ZSTD ? C_ZSTD : slot == S_LZ4 ? C_LZ4 : slot == S_LZ4_GEN ? C_LZ4_GEN : slot == S_LZ4_RUNS ? C_LZ4_RUNS : -1;
}

// Pinned on the host: what the device batch BEFORE held (decode_launch picks streams and launches by it).  One copy brings
// the four counts k_classify fills first, a second one the runs.
struct SeenCounts { unsigned none, zstd, lz4, lz4_gen, lz4_runs; };
static_assert(C_ZSTD == C_NONE + 1 && C_LZ4 == C_NONE + 2 && C_LZ4_GEN == C_NONE + 3, "SeenCounts' first four fields are one copy of counters[C_NONE ..]");

}  // namespace zpk
