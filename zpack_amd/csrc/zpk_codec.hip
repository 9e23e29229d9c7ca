// zpk_codec.hip — kernels + C-ABI of the MI355X entry codec (include/zpack_codec.h).
//
// Launch structure of one decode batch (all on one HIP stream, no host synchronisation):
//   1. k_classify   one thread per entry: the guards of zpack_read_file (lib/zpack_read.c:328-332,
//                   :354, :459) in the reference's order, then the entry index is appended to the
//                   work list of its method (wave-aggregated atomics).
//   2. k_stored / k_lz4_wave   one wave per work-list slot.
//   3. k_zstd_fse -> k_zstd_exec -> k_zstd   Zstandard: persistent grids that pull entries from the work list with an
//                   atomic dequeue (FSE sequence pre-decode four streams per wave; literals + execution + XXH3 of the
//                   pre-decoded entries; the full decoder for whatever is left over) — zstd_fse4.h, zstd_wg.h.
// Entries are independent, so there is no inter-workgroup communication besides the
// dequeue counters.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <time.h>
#include <pthread.h>
#include <thread>
#include <atomic>
#include <vector>
#include <algorithm>


#include "zpk_device.h"
#include "xxh3_device.h"
#include "xxh3_span.h"
#include "lz4_wave.h"
#include "lx_ring.h"
#ifndef LX_WAVES_PER_SIMD
#define LX_WAVES_PER_SIMD 6
#endif
#include "zstd_wg.h"
#include "zstd_fse4.h"
#include "zstd_ring.h"
#include "lz4_pj.h"
#include "zstd_pj.h"
#include "host_walk.h"                           // the host parsers of untrusted frame / block headers (plain C++, built under sanitizers by tools/hostfuzz)
#include "dec_plan.h"                            // a large entry's route on the read side: guards, candidates, chooser, walk layout, verdict (plain C++, likewise)
#include "big_walk.h"                            // k_big_walk: that walk over one large frame, on the device, for every large entry of a device-resident batch
#include "enc_plan.h"                            // an entry written in pieces: split rule, piece descriptors, frame envelope, verdict (plain C++, likewise)
#include "stored_plan.h"                         // the large stored entries of a device-resident batch: which are taken, their span table, the verdict (plain C++, likewise)
#include "stored_span.h"                         // k_stored_span: their copy fused with the XXH3 partial sums, across the chip
#include "copy_rows_plan.h"                      // the five row copies below: the 16 KiB item, the row search and the launch split they share (plain C++, likewise)
#include "span_copy_plan.h"                      // plaintext in the caller's DEVICE memory: the row table of k_span_copy, the staging slots, the pointer test (plain C++, likewise)
#include "plane_copy_plan.h"                     // byte-plane entries: the layout and the row table of k_plane_copy (plain C++, likewise)
#include "delta_copy_plan.h"                     // delta entries: a tensor stored as its XOR against a base in device memory, and the row table of k_delta_copy (plain C++, likewise)
#include "window_copy_plan.h"                    // window reads: a 2-D sub-block of an entry delivered densely, the rule, the map and the row table of k_window_copy (plain C++, likewise)
#include "place_copy_plan.h"                     // placed reads: that sub-block set into a sub-block of a larger tensor — the pitch, its rule, the extent and the row table of k_place_copy (plain C++, likewise)
// The five kernels are compiled in a file of their own, row_copy.hip: this file's code object stays the one it was, kernel for kernel at
// the same place (a 46th kernel among them cost c4_mixed 1.3 % in alternating pairs: profiles/r20/README.md)
namespace zpk {
void span_copy_launch(const SpanCopyRow* d_rows, u32 nrows, u64 item0, u64 nitems, u32 grid, hipStream_t st);
void plane_copy_launch(const PlaneCopyRow* d_rows, u32 nrows, u64 item0, u64 nitems, u32 grid, hipStream_t st);
void delta_copy_launch(const DeltaCopyRow* d_rows, u32 nrows, u64 item0, u64 nitems, u32 grid, hipStream_t st);
void window_copy_launch(const WindowCopyRow* d_rows, u32 nrows, u64 item0, u64 nitems, u32 grid, hipStream_t st);
void place_copy_launch(const PlaceCopyRow* d_rows, u32 nrows, u64 item0, u64 nitems, u32 grid, hipStream_t st);
}
#include "span_hash_plan.h"                      // XXH3 of arbitrary device spans (the bases of delta entries): one-wave and chip-wide rows, their tables, launches and loads (plain C++, likewise)
// k_span_hash (span_hash.h) and its copies of the chip-wide pair are compiled in span_hash.hip, for the same reason
namespace zpk { u32 span_hash_launch(u8* d_block, const SpanHashPlan& p, const SpanHashLayout& L, u64 max_wave_rows, u64 max_groups, u64 max_chains, hipStream_t st); }
// ... and so is k_stored_hash (stored_hash.h, stored_hash.hip): k_stored without the copy, for a batch that has no destination
namespace zpk { void stored_hash_launch(const u8* src, const zpk_decode_desc* desc, zpk_decode_result* res, const u32* list, const u32* counters, u32 grid, hipStream_t st); }
#include "dimage_plan.h"                         // a batch out of an archive image in DEVICE memory: its sub-batches and their staging slots (plain C++, likewise)
#include "host_plan.h"                           // the host-pointer read path: slot and sub-batch, staged image, pipeline pieces, copy shares, frame-parallel groups, delivery rules (plain C++, likewise)
#include "dsink_plan.h"                          // a batch compressed into a bounded sink in DEVICE memory: the cut, the span table, room and chaining, the staging (plain C++, likewise); the kernels: sink_commit.hip
#include "stream_plan.h"                        // the bounded steps of the stream reader: intake, go rule, hash sections, history carry, layouts, verdict (plain C++, likewise)
#include "codec_res.h"                           // what a codec or a stream context holds, each owned by its member: DevBuf, PinBuf / PinBlock, Event, Stream (plain C++ over the HIP runtime, likewise)

using namespace zpk;

// the counter block and the list storage: zpk_layout.h
__device__ __forceinline__ int order_list_slot(int y) { return y == 0 ? (int)S_ZSTD : y == 1 ? (int)S_LZ4 : (int)S_LZ4_GEN; }
__device__ __forceinline__ int order_count_word(int y) { return y == 0 ? (int)C_ZSTD : y == 1 ? (int)C_LZ4 : (int)C_LZ4_GEN; }
__device__ __forceinline__ int order_out_slot(int y) { return y == 0 ? (int)S_ZSTD_ORDERED : y == 1 ? (int)S_LZ4_ORDERED : (int)S_LZ4_GEN_ORDERED; }

// ------------------------------------------------------------------------------------ kernels

__device__ __forceinline__ int order_class(u64 size)
{
    const int lg = 63 - __clzll((long long)(size | 1));
    const int b = 26 - lg;                                                            // >= 64 MiB: class 0 ... < 4 KiB: class 15
    return b < 0 ? 0 : (b > ORD_CLASSES - 1 ? ORD_CLASSES - 1 : b);
}
// A batch of ONE size class (the uniform workloads) has nothing to order by size; there the entries that did not compress — payload not
// smaller than ~15/16 of the size: stored LZ4 blocks, raw Zstandard blocks, a copy that decodes several times faster than anything
// compressed — go LAST: they are what is left to fill the final round with (C2: +0.75 % over six A/B pairs; on the ragged c4_mixed the
// same key inside every size class measured -4 % +- noise, so it is not used there).
__device__ __forceinline__ int order_fast(u64 size, u64 comp) { return comp * 16 >= size * 15 ? 1 : 0; }
// Does the LZ4 entry begin like a PLAIN frame (what lz4f_plain_wave takes: version 01, no block / content checksum, no dictionary id, no
// reserved bits, block code >= 4)?  Only the 6 bytes in front of the header checksum are looked at; everything else is the decoder's.
__device__ __forceinline__ bool lz4_header_is_plain(const u8* __restrict__ p, u64 comp_size)
{
    if (comp_size < 11) return false;
    const u32 magic = (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24), flg = p[4], bd = p[5];
    return magic == 0x184D2204u && (flg & 0xD7u) == 0x40u && (bd & 0x8Fu) == 0 && ((bd >> 4) & 7u) >= 4u;
}
// wave-aggregated append of this wave's entries for list SLOT: one atomic per list per wave (a per-lane atomicAdd on three hot
// words cost 1.1 ms / 100k entries)
template <int SLOT>
__device__ __forceinline__ void classify_append(int list, u64 i, int lane, u32* __restrict__ lists, u64 list_stride, u32* __restrict__ counters)
{
    const u64 m = __ballot(list == SLOT);
    if (m == 0) return;
    const int leader = __ffsll((long long)m) - 1;
    u32 base = 0;
    if (lane == leader) base = atomicAdd(&counters[list_count_word(SLOT)], (u32)__popcll(m));
    base = (u32)__shfl((int)base, leader, 64);
    if (list == SLOT) lists[(u64)SLOT * list_stride + base + (u32)__popcll(m & ((1ull << lane) - 1))] = (u32)i;
}
__global__ __launch_bounds__(256) void k_classify(const u8* __restrict__ src, const zpk_decode_desc* __restrict__ desc, u64 n, u64 src_size, u64 dst_size,
                                                  zpk_decode_result* __restrict__ res, u32* __restrict__ lists, u64 list_stride,
                                                  u32* __restrict__ counters)
{
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    zpk_decode_desc d; memset(&d, 0, sizeof(d));
    if (live) d = desc[i];
    zpk_decode_result r; r.status = R_OK; r.detail = 0; r.produced = 0; r.hash = 0;
    int list = -1;                                                             // a ListSlot
    // lib/zpack_read.c:328-332, in this order
    if (!live) list = -1;
    else if (d.comp_size == 0) r.status = R_OK;
    else if (d.dst_capacity < d.uncomp_size) r.status = R_BUFFER_TOO_SMALL;
    else if (d.src_offset + d.comp_size >= src_size || d.src_offset > src_size || d.comp_size > src_size - d.src_offset)
        r.status = R_FILE_OFFSET_INVALID;
    else if (d.dst_offset > dst_size || d.dst_capacity > dst_size - d.dst_offset) { r.status = R_BUFFER_TOO_SMALL; r.detail = 0xBAD0D57u; }
    else if (d.method == ZPK_METHOD_NONE) {
        if (d.uncomp_size > d.comp_size) r.status = R_FILE_SIZE_INVALID;      // :354
        else list = S_NONE;
    }
    else if (d.method == ZPK_METHOD_ZSTD) list = S_ZSTD;
    else if (d.method == ZPK_METHOD_LZ4)                                       // mostly runs: k_lz4_left's; not a plain frame: k_lz4_general's
        list = d.comp_size < (d.uncomp_size >> 3) ? S_LZ4_RUNS : lz4_header_is_plain(src + d.src_offset, d.comp_size) ? S_LZ4 : S_LZ4_GEN;
    else r.status = R_COMP_METHOD_INVALID;                                     // :459
    // an entry that goes on a work list is not decoded yet: until its decoder writes the verdict the slot says so
    // (a decoder that never ran must not read as R_OK)
    if (list >= 0) { r.status = R_DECOMPRESS_FAILED; r.detail = 0xFFFFFFFFu; }
    if (live) res[i] = r;
    const int lane = lane_id();
    {   // the span of size classes among the entries that go to a decoder (k_order_*)
        const bool dec = list == S_ZSTD || list == S_LZ4 || list == S_LZ4_GEN;
        u32 hi = dec ? (u32)order_class(d.uncomp_size) + 1u : 0u, inv = dec ? (u32)(ORD_CLASSES - order_class(d.uncomp_size)) : 0u;   // (+1: 0 = none)
        #pragma unroll
        for (int m = 1; m < 64; m <<= 1) { const u32 a = (u32)__shfl_xor((int)hi, m, 64), b2 = (u32)__shfl_xor((int)inv, m, 64); hi = a > hi ? a : hi; inv = b2 > inv ? b2 : inv; }
        if (lane == 0 && hi) { atomicMax(&counters[C_ORDER_SPAN], hi - 1u); atomicMax(&counters[C_ORDER_SPAN_INV], inv - 1u); }
    }
    classify_append<S_NONE>(list, i, lane, lists, list_stride, counters);
    classify_append<S_ZSTD>(list, i, lane, lists, list_stride, counters);
    classify_append<S_LZ4>(list, i, lane, lists, list_stride, counters);
    classify_append<S_LZ4_RUNS>(list, i, lane, lists, list_stride, counters);
    classify_append<S_LZ4_GEN>(list, i, lane, lists, list_stride, counters);
}

// ---- largest entries first -----------------------------------------------------------------------------------------------------
// One wave (or one FSE row) works on one entry, and a batch is only a few rounds of the resident waves: with entries of 4 KiB ... 1 MiB
// in archive order, a 1 MiB entry that starts in the last round runs on alone for its whole length while the rest of the chip idles.
// The Zstandard and LZ4 work lists are therefore re-ordered by size class (floor(log2 uncomp_size), largest first: longest
// processing time first) with a two-kernel counting sort — per-workgroup LDS histograms, one global atomic per class and
// workgroup; entries of one class keep their neighbourhood.  (Uniform batches come out in nearly the order they went in.)
// (k_classify leaves the largest class and the largest 15 - class it saw in counters[C_ORDER_SPAN], [C_ORDER_SPAN_INV]: a batch of ONE
// class — the uniform workloads — is copied through in its own order.)
__device__ __forceinline__ bool order_single_class(const u32* counters) { return counters[C_ORDER_SPAN] + counters[C_ORDER_SPAN_INV] == ORD_CLASSES - 1; }
// rank of this lane among the lanes of its wave with the same class (in lane order), and how many there are
__device__ __forceinline__ void order_wave_rank(int b, int lane, u32& rank, u32& count)
{
    rank = 0; count = 0;
    u64 todo = __ballot(b >= 0);
    while (todo) {
        const int cls = __shfl(b, __ffsll((long long)todo) - 1, 64);
        const u64 m = __ballot(b == cls);
        if (b == cls) { rank = (u32)__popcll(m & ((1ull << lane) - 1)); count = (u32)__popcll(m); }
        todo &= ~m;
    }
}
__global__ __launch_bounds__(256) void k_order_count(const zpk_decode_desc* __restrict__ desc, const u32* __restrict__ lists, u64 list_stride,
                                                     u32* __restrict__ counters, int fast_last)
{
    __shared__ u32 h[ORD_CLASSES];
    const int L = order_list_slot(blockIdx.y);
    const u32 cnt = counters[order_count_word(blockIdx.y)];
    const bool uniform = order_single_class(counters);
    if ((u64)blockIdx.x * 256 >= cnt || (uniform && !fast_last)) return;
    if (threadIdx.x < ORD_CLASSES) h[threadIdx.x] = 0;
    __syncthreads();
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    const int lane = lane_id();
    int b = -1;
    if (k < cnt) { const zpk_decode_desc& d = desc[lists[(u64)L * list_stride + k]]; b = uniform ? order_fast(d.uncomp_size, d.comp_size) : order_class(d.uncomp_size); }
    u32 rank, count;
    order_wave_rank(b, lane, rank, count);
    if (b >= 0 && rank == 0) atomicAdd(&h[b], count);
    __syncthreads();
    if (threadIdx.x < ORD_CLASSES && h[threadIdx.x]) atomicAdd(&counters[C_ORDER_HIST + blockIdx.y * ORD_CLASSES + threadIdx.x], h[threadIdx.x]);
}
__global__ __launch_bounds__(256) void k_order_fill(const zpk_decode_desc* __restrict__ desc, const u32* __restrict__ lists, u64 list_stride,
                                                    u32* __restrict__ all_lists /* the ordered copies: order_out_slot() */, u32* __restrict__ counters, int fast_last)
{
    __shared__ u32 wcount[4][ORD_CLASSES], base[ORD_CLASSES];
    const int L = order_list_slot(blockIdx.y);
    const u32 cnt = counters[order_count_word(blockIdx.y)];
    u32* const ordered = all_lists + (u64)order_out_slot(blockIdx.y) * list_stride;
    if ((u64)blockIdx.x * 256 >= cnt) return;
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    const bool uniform = order_single_class(counters);
    if (uniform && !fast_last) { if (k < cnt) ordered[k] = lists[(u64)L * list_stride + k]; return; }
    if (threadIdx.x < 4 * ORD_CLASSES) (&wcount[0][0])[threadIdx.x] = 0;
    __syncthreads();
    const int lane = lane_id(), w = threadIdx.x >> 6;
    u32 e = 0; int b = -1;
    if (k < cnt) { e = lists[(u64)L * list_stride + k]; b = uniform ? order_fast(desc[e].uncomp_size, desc[e].comp_size) : order_class(desc[e].uncomp_size); }
    u32 rank, count;
    order_wave_rank(b, lane, rank, count);
    if (b >= 0 && rank == 0) wcount[w][b] = count;
    __syncthreads();
    if (threadIdx.x < ORD_CLASSES) {                                                   // this workgroup's range of the class: entries stay in list order inside it
        const int c = threadIdx.x;
        const u32 total = wcount[0][c] + wcount[1][c] + wcount[2][c] + wcount[3][c];
        const u32* const hist = counters + C_ORDER_HIST + blockIdx.y * ORD_CLASSES;
        u32 before = 0;
        for (int j = 0; j < c; j++) before += hist[j];
        base[c] = total ? before + atomicAdd(&counters[C_ORDER_FILL + blockIdx.y * ORD_CLASSES + c], total) : 0;
    }
    __syncthreads();
    if (b >= 0) {
        u32 at = base[b] + rank;
        for (int j = 0; j < w; j++) at += wcount[j][b];
        ordered[at] = e;
    }
}

// one wave per work-list slot: the hardware dispatcher is the load balancer
__device__ __forceinline__ bool my_slot(const u32* counters, int count_word, u32& idx)
{
    idx = uni((u32)(((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6));           // 64-bit: n blocks x 64 threads passes 2^32 at n = 2^26
    return idx < uni(counters[count_word]);
}

template <bool LDS_KEYS = false>
__device__ __forceinline__ void finish_entry(const zpk_decode_desc& d, zpk_decode_result* res, u32 e, int status, u32 detail,
                                             u64 produced, const u8* out, int lane, lds_p8 sec = nullptr)
{
    // LDS_KEYS: `sec` = 192 bytes of LDS (16-byte aligned) the caller no longer needs, for the hash loop's keys; else keys in registers
    u64 h = 0;
    lane0_guard();
    if (status == R_OK) {                                                      // (ZPK_DF_SKIP_HASH: the hash is still produced, the status ignores it)
        wave_mem_fence();
        h = xxh3_64_wave<LDS_KEYS>(out, d.uncomp_size, lane, sec);                 // lib/zpack_read.c:466
        if (h != d.expect_hash && !(d.flags & ZPK_DF_SKIP_HASH)) status = R_FILE_HASH_MISMATCH;   // :467-468
    }
    lane0_guard();
    if (lane == 0) {
        zpk_decode_result r; r.status = status; r.detail = detail; r.produced = produced; r.hash = h;
        res[e] = r;
    }
}

// method 0: copy + hash fused — each 1 KiB block is loaded once, stored, and folded into the hash
__global__ __launch_bounds__(256) void k_stored(const u8* __restrict__ src, const zpk_decode_desc* __restrict__ desc,
                                                u8* __restrict__ dst, zpk_decode_result* __restrict__ res,
                                                const u32* __restrict__ list, const u32* __restrict__ counters)
{
    const int lane = lane_id();
    u32 idx;
    if (my_slot(counters, C_NONE, idx)) {
        const u32 e = uni(list[idx]);
        const zpk_decode_desc d = desc[e];
        const u8* in = uni_ptr(src + d.src_offset);
        u8* out = uni_ptr(dst + d.dst_offset);
        const u64 len = uni64(d.uncomp_size);
        u64 h;
        if (len <= 240) {
            for (u64 i = lane; i < len; i += WAVE) st8(out + i, ld8(in + i));
            h = 0;
            lane0_guard();
            if (lane == 0) h = xxh3_short(in, (u32)len);
            h = uni64(h);
        } else {
            Xxh3Wave st; st.init(lane);
            const u64 nblocks = (len - 1) >> 10;
            const u8* q = in + 16 * lane;
            u8* o = out + 16 * lane;
            u128 cur = {0, 0};
            if (nblocks) cur = ld128(q);
            for (u64 b = 0; b < nblocks; b++) {
                u128 nxt = {0, 0};
                if (b + 1 < nblocks) nxt = ld128(q + ((b + 1) << 10));
                st128(o + (b << 10), cur);
                st.block(cur);
                cur = nxt;
            }
            const u64 done = nblocks << 10;
            for (u64 i = done + lane; i < len; i += WAVE) st8(out + i, ld8(in + i));
            const u32 nstripes = (u32)(((len - 1) - done) >> 6);
            h = st.finish(in + done, nstripes, in + len, len, lane);
        }
        int status = R_OK;
        if (!(d.flags & ZPK_DF_SKIP_HASH) && h != d.expect_hash) status = R_FILE_HASH_MISMATCH;
        lane0_guard();
        if (lane == 0) {
            zpk_decode_result r; r.status = status; r.detail = 0; r.produced = len; r.hash = h;
            res[e] = r;
        }
    }
}

// developer: the per-phase cycle counters of one entry (ZPK_STATS builds; dbg = 8 words per entry)
__device__ __forceinline__ void lz4_stats_out(u64* __restrict__ dbg, u32 e, const SeqStats& stt, u64 t_all, int lane)
{
#ifdef ZPK_STATS
    if (dbg && lane == 0) {
        u64* g = dbg + (u64)e * 8;
        g[0] = stt.t_parse; g[1] = stt.t_lit; g[2] = stt.t_dep; g[3] = stt.t_rounds;
        g[4] = ((u64)stt.batches << 32) | stt.rounds; g[5] = ((u64)stt.coops << 32) | stt.asm_batches; g[6] = SEQ_T() - t_all;
        g[7] = ((u64)stt.fix_iters << 32) | stt.chunks;
#ifdef ZPK_STATS_PARSE
        g[0] = stt.t_stage; g[1] = stt.t_walk1; g[2] = stt.t_fix; g[3] = stt.t_emit; g[4] = stt.t_tok;
        g[5] = ((u64)stt.hops_first << 32) | stt.hops_fix; g[6] = stt.slow_hops;
#endif
#ifdef ZPK_STATS_ASM
        g[0] = ((u64)stt.batches << 32) | stt.asm_batches; g[1] = ((u64)stt.r_room << 32) | stt.r_piece; g[2] = ((u64)stt.r_both << 32) | stt.r_straddle;
        g[3] = ((u64)stt.k_lit << 32) | stt.k_match; g[5] = stt.t_asm; g[6] = stt.t_dir;
        // word 4: four counters of 16 bits (each fits them per entry): self-overlapping offset >= 16, < 16, assembled with a self-overlapping match, its extra rounds
        g[4] = ((u64)(stt.k_so16 & 0xFFFFu) << 48) | ((u64)(stt.k_so1 & 0xFFFFu) << 32) | ((u64)(stt.a_self & 0xFFFFu) << 16) | (stt.x_rounds & 0xFFFFu);
        g[7] = ((u64)stt.b_asm << 32) | stt.b_dir;
#endif
    }
#else
    (void)dbg; (void)e; (void)stt; (void)t_all; (void)lane;
#endif
}

// one LZ4 entry, one wave, the GENERAL decoder (every frame shape, every verdict).  retry_list != nullptr: a decode that ran out of
// its time budget is not reported — the entry goes on that list (counters[C_RETRY_LZ4]) and k_lz4_retry decodes it again behind the
// batch with ZPK_WATCHDOG_RETRY_SCALE times the budget.
// COOP: seq_exec.h — 0 = the round-4 code, one cooperative piece at a time (k_lz4_wave), 2 = grouped cooperative copies.
template <int COOP>
__device__ __forceinline__ void lz4_entry_wave(Lz4WaveShared& shw, const u8* __restrict__ src, const u8* read_lo, const u8* read_hi,
                                               const zpk_decode_desc* __restrict__ desc, u8* dst, zpk_decode_result* __restrict__ res,
                                               u32 e, u32* __restrict__ counters, u64* __restrict__ dbg, u32* __restrict__ retry_list,
                                               u32 wd_scale, int lane)
{
    const zpk_decode_desc d = desc[e];
    const u8* in = uni_ptr(src + d.src_offset);
    u8* out = uni_ptr(dst + d.dst_offset);
    Watchdog wd; wd.arm(uni64(d.comp_size) + uni64(d.dst_capacity), wd_scale);
    SeqStats stt = {};
    const u64 t_all = SEQ_T(); (void)t_all;
    DecodeOut o = lz4f_decode_wave<COOP>(shw, wd, stt, in, uni64(d.comp_size), read_lo, read_hi, out, uni64(d.dst_capacity), lane);
    lz4_stats_out(dbg, e, stt, t_all, lane);
    if (wd.fired && retry_list) {                               // slow is not a verdict: again, later, with the large budget
        lane0_guard();
        if (lane == 0) retry_list[atomicAdd(&counters[C_RETRY_LZ4], 1u)] = e;
        return;
    }
    // lib/zpack_read.c:421-450
    int status = R_OK;
    if (o.rc == D_MALFORMED) status = R_DECOMPRESS_FAILED;
    else if (o.rc == D_TRUNCATED) status = o.produced < d.dst_capacity ? R_FILE_INCOMPLETE : R_BUFFER_TOO_SMALL;
    else if (o.rc == D_DST_FULL) status = R_BUFFER_TOO_SMALL;
    finish_entry<true>(d, res, e, status, wd.fired ? 0xDEADu : (u32)(-o.rc), o.produced, out, lane, to_lds_rw(shw.stage));
}

// one LZ4 entry, one wave, the LEAN decoder of the hot kernel: one plain frame (lz4f_plain_wave) that decodes to exactly uncomp_size
// bytes is finished here (OK, or FILE_HASH_MISMATCH from the XXH3 pass).  EVERYTHING else — another frame shape, damage of any kind,
// a spent time budget — is not judged: the entry goes on the hand-over list (a spent budget: on the retry list) and k_lz4_retry decodes it
// from scratch with the general decoder, so every other verdict is produced by the code that always produced it.
__device__ __forceinline__ void lz4_entry_plain(Lz4WaveShared& shw, const u8* __restrict__ src, const u8* read_hi,
                                                const zpk_decode_desc* __restrict__ desc, u8* dst, zpk_decode_result* __restrict__ res,
                                                u32 e, u32* __restrict__ counters, u64* __restrict__ dbg, u32* __restrict__ retry_list,
                                                u32* __restrict__ handed_list, u32 wd_scale, int lane)
{
    const zpk_decode_desc& d = desc[e];
    const u8* in = uni_ptr(src + d.src_offset);
    u8* out = uni_ptr(dst + d.dst_offset);
    Watchdog wd; wd.arm(uni64(d.comp_size) + uni64(d.dst_capacity), wd_scale);
    SeqStats stt = {};
    const u64 t_all = SEQ_T(); (void)t_all;
    const bool done = lz4f_plain_wave<0>(shw, wd, stt, in, uni64(d.comp_size), read_hi, out, uni64(d.dst_capacity), uni64(d.uncomp_size), lane);
    lz4_stats_out(dbg, e, stt, t_all, lane);
    if (!done) {
        lane0_guard();
        if (lane == 0) {                                        // (slow is a retry, like everywhere; anything else a hand-over)
            if (wd.fired) retry_list[atomicAdd(&counters[C_RETRY_LZ4], 1u)] = e;
            else handed_list[atomicAdd(&counters[C_LZ4_HANDED], 1u)] = e;
        }
        return;
    }
    finish_entry<true>(d, res, e, R_OK, 0u, uni64(d.uncomp_size), out, lane, to_lds_rw(shw.stage));
}

// one wave per slot of the LZ4 work list: the hardware dispatcher is the load balancer.  (The developer build keeps the phase
// counters' buffer and the scale of the time budget as arguments; the product kernel carries neither.)
__global__ __launch_bounds__(64, 8) void k_lz4_wave(const u8* __restrict__ src, const u8* read_hi,
                                                  const zpk_decode_desc* __restrict__ desc, u8* dst,
                                                  zpk_decode_result* __restrict__ res, const u32* __restrict__ list,
                                                  u32* __restrict__ counters, u32* __restrict__ retry_list, u32* __restrict__ handed_list
#ifdef ZPK_DEVELOPER
                                                  , u64* __restrict__ dbg, u32 wd_scale
#endif
                                                  )
{
#ifndef ZPK_DEVELOPER
    const u32 wd_scale = 1u;
    u64* const dbg = nullptr;
#endif
    const int lane = lane_id();
    __shared__ Lz4WaveShared shw;
    u32 idx;
    if (my_slot(counters, C_LZ4, idx))
        lz4_entry_plain(shw, src, read_hi, desc, dst, res, uni(list[idx]), counters, dbg, retry_list, handed_list, wd_scale, lane);
}

#ifdef ZPK_DEVELOPER
// developer hook (ZPK_LZ4_GENERAL=1), launched INSTEAD of k_lz4_wave: every entry of the LZ4 work list goes to the general decoder
__global__ __launch_bounds__(256) void k_lz4_hand_all(const u32* __restrict__ list, u32* __restrict__ counters, u32* __restrict__ handed_list)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < counters[C_LZ4]) handed_list[atomicAdd(&counters[C_LZ4_HANDED], 1u)] = list[i];
}
#endif

// k_lz4_general: the LZ4 entries whose frame header is not that of a plain frame (k_classify reads magic, FLG and BD: checksums on — what
// the lz4 command line tool writes —, a dictionary id, a skippable frame in front, anything unknown) by the general decoder, the code
// k_lz4_wave was before it went lean (COOP = 0, the normal time budget, the retry list behind it), from a list of their own in
// largest-first order.  A persistent grid as wide as the chip's resident waves with an atomic dequeue, beside k_lz4_wave and k_lz4_left;
// it leaves at once when the list is empty (archives of the reference writer and of this library: always).
#define LZ4_GENERAL_GRID_MAX 8192u
__global__ __launch_bounds__(64, 8) void k_lz4_general(const u8* __restrict__ src, const u8* read_lo, const u8* read_hi,
                                                     const zpk_decode_desc* __restrict__ desc, u8* dst,
                                                     zpk_decode_result* __restrict__ res, const u32* __restrict__ list,
                                                     u32* __restrict__ counters, u64* __restrict__ dbg, u32* __restrict__ retry_list, u32 wd_scale)
{
    const int lane = lane_id();
    __shared__ Lz4WaveShared shw;
    const u32 n_slots = uni(counters[C_LZ4_GEN]);
    if (n_slots == 0) return;
    for (u32 idx; dequeue(counters, C_LZ4_GEN_HEAD, n_slots, lane, idx); )
        lz4_entry_wave<0>(shw, src, read_lo, read_hi, desc, dst, res, uni(list[idx]), counters, dbg, retry_list, wd_scale, lane);
}

// The general decoder behind all other LZ4 kernels of the batch, a small grid (what it finds is rare: normally nothing, and then every
// workgroup leaves at once).  It drains, in this order: what is left of k_lz4_general's list (all of it when that kernel was not
// launched: see decode_launch), the entries k_lz4_wave handed over without judging them (a plain header, but a decode without a clean
// end: damaged or truncated frames, output full, trailing bytes), and the entries whose decoder ran out of its time budget.
// ZPK_WATCHDOG_RETRY_SCALE times the budget, and now the verdict counts.
__global__ __launch_bounds__(64, 8) void k_lz4_retry(const u8* __restrict__ src, const u8* read_lo, const u8* read_hi,
                                                   const zpk_decode_desc* __restrict__ desc, u8* dst,
                                                   zpk_decode_result* __restrict__ res, const u32* __restrict__ lists, u64 list_stride,
                                                   u32* __restrict__ counters, u64* __restrict__ dbg, int gen_slot)
{
    const int lane = lane_id();
    __shared__ Lz4WaveShared shw;
    for (int k = 0; k < 3; k++) {
        const int count_word = k == 0 ? (int)C_LZ4_GEN : k == 1 ? (int)C_LZ4_HANDED : (int)C_RETRY_LZ4;
        const int head_word = k == 0 ? (int)C_LZ4_GEN_HEAD : k == 1 ? (int)C_LZ4_HANDED_HEAD : (int)C_LZ4_RETRY_HEAD;
        const u32* const list = lists + (u64)(k == 0 ? gen_slot : k == 1 ? (int)S_LZ4_HANDED : (int)S_RETRY_LZ4) * list_stride;
        const u32 n_slots = uni(counters[count_word]);
        if (n_slots == 0 || uni(counters[head_word]) >= n_slots) continue;          // (empty, or drained by an earlier launch)
        for (u32 idx; dequeue(counters, head_word, n_slots, lane, idx); )
            lz4_entry_wave<2>(shw, src, read_lo, read_hi, desc, dst, res, uni(list[idx]), counters, dbg, nullptr, (u32)ZPK_WATCHDOG_RETRY_SCALE, lane);
    }
}

// k_lz4_left: the LZ4 entries that are mostly RUNS — k_classify puts an entry compressed to less than an eighth of its size on this
// list instead of k_lz4_wave's (byte runs, repeated blocks: matches longer than 32 bytes or feeding themselves; on the benchmark
// corpus exactly the `runs` class) — decoded by the same one-wave decoder built with the grouped cooperative copies (seq_exec.h
// COOP = 2): 614 -> ~2 000 GiB/s on such entries.  A persistent grid with an atomic dequeue, launched in FRONT of k_lz4_wave (a
// launch behind it would be a serial tail); it leaves at once when the list is empty (text, records: always).
#define LZ4_LEFT_GRID_MAX 8192u
#ifndef LZ4_LEFT_WAVES
#define LZ4_LEFT_WAVES 8
#endif
__global__ __launch_bounds__(64, LZ4_LEFT_WAVES) void k_lz4_left(const u8* __restrict__ src, const u8* read_lo, const u8* read_hi,
                                                  const zpk_decode_desc* __restrict__ desc, u8* dst,
                                                  zpk_decode_result* __restrict__ res, const u32* __restrict__ list,
                                                  u32* __restrict__ counters, u64* __restrict__ dbg, u32* __restrict__ retry_list, u32 wd_scale)
{
    const int lane = lane_id();
    __shared__ Lz4WaveShared shw;
    const u32 n_slots = uni(counters[C_LZ4_RUNS]);
    if (n_slots == 0) return;                      // (text, records: always — 8192 dequeues on one word are 0.1 ms by themselves)
    for (u32 idx; dequeue(counters, C_LZ4_RUNS_HEAD, n_slots, lane, idx); )
        lz4_entry_wave<2>(shw, src, read_lo, read_hi, desc, dst, res, uni(list[idx]), counters, dbg, retry_list, wd_scale, lane);
}

// Stage 2 of the two-stage Zstandard path: entries whose sequences k_zstd_fse left in the arena (zstate == 1) are run
// here — Huffman literals, execution, XXH3 — by a kernel that carries neither the FSE decoder's code nor its tables:
// 9.4 KiB of LDS and <= 128 VGPRs, 16 workgroups per CU.  Only a COMPLETE entry (every frame decoded, exactly uncomp_size bytes) is finished here
// (result written, zstate = 2: status OK, or FILE_HASH_MISMATCH when its XXH3 differs — decoding it again could only find the same);
// everything else is left to k_zstd, so every verdict other than those two is always the full decoder's.
#define ZSTD_EXEC_GRID_MAX 4096
#ifndef ZSTD_EXEC_WAVES
#define ZSTD_EXEC_WAVES 4
#endif
// The execute stage runs through the LDS output ring (zstd_ring.h): aligned LDS accesses, near matches served from LDS, whole 1 KiB
// lines flushed with the XXH3 accumulators fed on the way out.  Against the direct executor of round 1 (every sequence written to and
// gathered from HBM with exact-tail accesses, hash by re-reading) it moves 34 % fewer bytes in and 27 % fewer out of HBM at the same
// speed (profiles/r02: text, 8192 x 256 KiB: FETCH 13.8 -> 9.1 GB raw, WRITE 4.5 -> 3.3 GB; C3 62.4 vs 61.3 ms, C4 equal).
__global__ __launch_bounds__(ZSTD_WG_THREADS, ZSTD_EXEC_WAVES) void k_zstd_exec(const u8* __restrict__ src, const zpk_decode_desc* __restrict__ desc,
                                                               u8* dst, zpk_decode_result* __restrict__ res,
                                                               const u32* __restrict__ list, u32* __restrict__ counters,
                                                               u8* __restrict__ lit_scratch, const u64* __restrict__ arena,
                                                               u32* __restrict__ zstate, u32* __restrict__ leftover, u64* __restrict__ dbg)
{
    const int lane = lane_id();
    const u32 nz = uni(counters[C_ZSTD]);
    if (nz == 0) return;
    __shared__ ZstdRingShared sh;
    if (threadIdx.x == 0) sh.huf_valid = 0;
    __syncthreads();
    u8* lit = lit_scratch + (u64)blockIdx.x * ZSTD_LIT_SCRATCH;
    for (u32 idx; dequeue(counters, C_EXEC_HEAD, nz, lane, idx); ) {
        const u32 e = uni(list[idx]);
        if (uni(zstate[e]) != 1u) {                     // not pre-decoded: straight to the full decoder's list
            lane0_guard();
            if (lane == 0) leftover[atomicAdd(&counters[C_ZSTD_LEFT], 1u)] = e;
            lane0_guard();
            continue;
        }
        const zpk_decode_desc d = desc[e];
        const u8* in = uni_ptr(src + d.src_offset);
        u8* out = uni_ptr(dst + d.dst_offset);
        const u64* const pre = arena + (((u64)d.dst_offset + 7) >> 3);
        Watchdog wd; wd.arm(uni64(d.comp_size) + uni64(d.dst_capacity));
        (void)dbg;
        // through the LDS output ring (zstd_ring.h): the hash comes out of the flushes
        struct { int rc; u64 produced; } o;
        const LxResult xr = zstd_ring_decode_wave(sh, wd, in, uni64(d.comp_size), out, uni64(d.dst_capacity), uni64(d.uncomp_size), lit, pre, lane,
                                                   dbg ? dbg + (u64)e * 16 : nullptr);
        o.rc = xr.rc == LX_OK ? D_OK : -(0x100 + xr.rc); o.produced = xr.produced;
        const u64 h = xr.hash;
        // A complete, byte-exact decode is finished here whatever its checksum says: FILE_HASH_MISMATCH is the verdict of
        // lib/zpack_read.c:466-468 for exactly this case, and decoding the entry a second time in k_zstd would only reach it again
        // (the set of frames this path accepts equals the oracle's on 18 000 damaged frames: profiles/r02/r02_fuzz_ring_executor.log)
        const bool ok = xr.rc == LX_OK && xr.produced == uni64(d.uncomp_size);
        const int ok_status = (h == d.expect_hash || (d.flags & ZPK_DF_SKIP_HASH)) ? R_OK : R_FILE_HASH_MISMATCH;
        lane0_guard();
        if (lane == 0) {
            if (ok) {
                zpk_decode_result r; r.status = ok_status; r.detail = 0; r.produced = o.produced; r.hash = h;
                res[e] = r;
                zstate[e] = 2u;
                atomicAdd(&counters[C_ZSTD_TWO_STAGE], 1u);
            } else {
                leftover[atomicAdd(&counters[C_ZSTD_LEFT], 1u)] = e;
                atomicAdd(&counters[C_EXEC_FAILED], 1u); counters[C_EXEC_LAST_RC] = ((u32)(-o.rc) & 0xFFFFu);
            }
        }
    }
}

// the full decoder: every Zstandard entry the two-stage path did not finish (all of them when it is off)
__global__ __launch_bounds__(ZSTD_WG_THREADS, 3) void k_zstd(const u8* __restrict__ src, const zpk_decode_desc* __restrict__ desc,
                                                          u8* dst, zpk_decode_result* __restrict__ res,
                                                          const u32* __restrict__ list, u32* __restrict__ counters,
                                                          u8* __restrict__ lit_scratch, u64* __restrict__ dbg, int count_word,
                                                          int head_word, u32* __restrict__ retry_list, int retry_word, u32 wd_scale)
{
    // `list` / counters[count_word]: the Zstandard work list itself, what k_zstd_exec left over, or (retry_list == nullptr) the
    // entries the first launch gave up on; counters[head_word]: the dequeue head of this launch
    const int lane = lane_id();
    const u32 nz = uni(counters[count_word]);
    if (nz == 0) return;
    __shared__ ZstdShared sh;
    if (threadIdx.x == 0) { sh.defaults_built = 0; sh.huf_valid = 0; }
    __syncthreads();
    u8* lit = lit_scratch + (u64)blockIdx.x * ZSTD_LIT_SCRATCH;
    for (u32 idx; dequeue(counters, head_word, nz, lane, idx); ) {
        const u32 e = uni(list[idx]);
        const zpk_decode_desc d = desc[e];
        const u8* in = uni_ptr(src + d.src_offset);
        u8* out = uni_ptr(dst + d.dst_offset);
        Watchdog wd; wd.arm(uni64(d.comp_size) + uni64(d.dst_capacity), wd_scale);
#ifdef ZPK_STATS
        ZstdStats zs = {};
        const u64 t_all = SEQ_T();
        DecodeOut o = zstd_decode_wave<false>(sh, wd, in, uni64(d.comp_size), out, uni64(d.dst_capacity), lit, lane, &zs);
        if (dbg && lane == 0) {
            u64* g = dbg + (u64)e * 8;
            g[0] = zs.t_lit; g[1] = zs.t_tab; g[2] = zs.t_fse; g[3] = zs.t_exec; g[4] = zs.nseq; g[5] = zs.nblk; g[6] = SEQ_T() - t_all; g[7] = 0;
        }
#else
        (void)dbg;
        DecodeOut o = zstd_decode_wave<false>(sh, wd, in, uni64(d.comp_size), out, uni64(d.dst_capacity), lit, lane);
#endif
        int status = o.rc == D_OK ? R_OK : R_DECOMPRESS_FAILED;               // lib/zpack_read.c:384-388
        if (wd.fired && retry_list) {                               // slow is not a verdict: again, later, with the large budget
            lane0_guard();
            if (lane == 0) retry_list[atomicAdd(&counters[retry_word], 1u)] = e;
            lane0_guard();
            continue;
        }
        finish_entry(d, res, e, status, wd.fired ? 0xDEADu : (u32)(-o.rc), o.produced, out, lane);
        lane0_guard();
        if (lane == 0) atomicAdd(&counters[C_ZSTD_FUSED], 1u);
    }
}

__global__ __launch_bounds__(256) void k_hash(const u8* __restrict__ src, const u64* __restrict__ offsets,
                                              const u64* __restrict__ sizes, u64 n, u64* __restrict__ hashes)
{
    const int lane = lane_id();
    const u64 w = uni64(((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (w < n) {
        u64 h = xxh3_64_wave(uni_ptr(src + offsets[w]), uni64(sizes[w]), lane);
        lane0_guard();
        if (lane == 0) hashes[w] = h;
    }
}

// ------------------------------------------------------------------------------------ host side

#define ZPK_ENC_SPLIT_MIN_DEFAULT (2ull << 20)
#define ZPK_STORED_SPAN_MIN_DEFAULT (256ull << 10) // (round 17: tools/big_batch_device_rate.py --stored, profiles/r17)
#define ZPK_SPAN_HASH_MIN_DEFAULT ZPK_STORED_SPAN_MIN_DEFAULT // (the same decision for spans that are no entries: tools/base_check_rate.py kernels, profiles/r31)
#ifndef ZPK_STORED_SPAN_FORK
#define ZPK_STORED_SPAN_FORK 1                     // zpk_codec_decode_big_batch_device runs the stored spans on a second stream beside the rest of the call; 0: on its own stream, in front of the walk
                                                   // (256 MiB stored + 256 MiB LZ4 text in one call: 14.9-15.2 ms forked against 23.6-23.9 ms serial, every forked run ahead: profiles/r17/r17_fork_ab.txt)
#endif
#ifndef ZPK_PJ_CHUNK_BLOCKS
#define ZPK_PJ_CHUNK_BLOCKS 512u                   // lz4_pj.h: blocks per chunk = 32 MiB of output, 128 MiB of byte references (the Infinity Cache holds 256)
#endif
#define ZPK_PJ_MAX_CHUNKS 64u

// What a batch holds, handed to decode_launch by the caller that knows: 1 / 0 = it does / does not hold an entry of the method (the host
// paths count while they cut the batch), -1 = a device batch, which may hold any
struct BatchMethods { int zstd, lz4; };

// Where the plaintext of a host-path or device-image batch goes: the caller's HOST buffers (the copy home and the scatter), the caller's
// DEVICE buffers (k_span_copy), or NOWHERE — the batch is only tested (zpk_codec_verify_batch_host / _dimage): the verdicts come home,
// no plaintext byte does.  One routing serves the three.  Without a destination dst_ptrs is not looked at (it may be NULL), the
// descriptors' capacity is uncomp_size (verify_descs), a stored entry has no staging slot and is hashed where it lies (k_stored_hash;
// a large one: k_xxh3_partials over the source), and the tail of a short decode counts as zeros (rehash_short_entries).
enum class Dst : int { Host = 0, Device = 1, None = 2 };
// The element sizes of a batch whose plaintext lies in the caller's device memory (plane_copy_plan.h): elem[i] of entry i, none = every
// entry is plain bytes (element size 1).  Handed down as an argument to whatever stages sources or delivers slots.
// ... and their BASES (delta_copy_plan.h): base[i] of entry i is device memory of the entry's plain size, none (or NULL for an entry) =
// the entry has no base.  An entry with a base is stored as split(plain XOR base) and is treated wherever an element size above 1 is.
// ... and the VERDICTS on those bases (the _delta_checked calls): refused[i] != 0 = the base of entry i did not hash to the value the
// caller recorded for it; none = no base was checked.  The column travels with the other two.
// ... and their WINDOWS (window_copy_plan.h; the _windows reads): win[i].row_bytes != 0 = of entry i only that sub-block is delivered,
// densely, to a destination — and against a base — of window_bytes bytes; none (or row_bytes == 0 for an entry) = the entry whole.  An
// entry with a window is treated wherever a grouped entry is, whatever its element size or base.  The fourth column, cut and gathered
// with the other three.
// ... and their PITCHES (place_copy_plan.h; the _placed reads): pitch[i] != 0 = the window of entry i is PLACED — window row r at byte
// r * pitch[i] of the destination, and of the base — so destination and base hold place_extent bytes of which only the placed ones are
// touched; none (or 0 for an entry) = the window lies densely.  Only an entry with a window has one (placed_check).  The fifth column,
// cut and gathered with the other four.
struct Planes {
    const u8* elem = nullptr;
    const u8* const* base = nullptr;
    const u8* refused = nullptr;
    const zpk_window* win = nullptr;
    const u64* pitch = nullptr;
    u32 of(u64 i) const { return elem ? elem[i] : 1u; }
    const u8* base_of(u64 i) const { return base ? base[i] : nullptr; }
    bool refused_at(u64 i) const { return refused && refused[i] && base_of(i) != nullptr; }
    bool windowed(u64 i) const { return win && win[i].row_bytes != 0; }
    Window window_of(u64 i) const { return windowed(i) ? Window{ win[i].row_bytes, win[i].row0, win[i].rows, win[i].col0, win[i].cols } : Window{ 0, 0, 0, 0, 0 }; }
    bool grouped(u64 i) const { return of(i) > 1 || base_of(i) != nullptr || windowed(i); }        // not a plain copy: k_plane_copy's, k_delta_copy's or k_window_copy's
    u64 pitch_of(u64 i) const { return pitch ? pitch[i] : 0ull; }
    bool placed(u64 i) const { return windowed(i) && pitch_of(i) != 0; }
    Planes from(u64 first) const { return Planes{ elem ? elem + first : nullptr, base ? base + first : nullptr, refused ? refused + first : nullptr, win ? win + first : nullptr, pitch ? pitch + first : nullptr }; }
    bool any() const { return elem != nullptr || base != nullptr || win != nullptr; }
    // what the caller's buffer and the base of entry i hold: the placement's extent, the window's bytes, or those given
    u64 dst_len(u64 i, u64 whole) const { return placed(i) ? place_extent(window_of(i), pitch[i]) : windowed(i) ? window_bytes(window_of(i)) : whole; }
    // what of the caller's buffer of `cap` bytes the call may write: all of it, of a window's no more than the window (too small a one: cap)
    u64 room(u64 i, u64 cap) const { const u64 w = dst_len(i, cap); return w < cap ? w : cap; }
    inline u64 join_len(u64 i, const zpk_decode_desc& d, const zpk_decode_result& r) const;
};
// ZPK_E_INVALID: an element size that is none (plane_elem_valid), before anything is enqueued
static int planes_check(zpk_codec* c, const u8* elem, u64 n);
// what of a decoded entry is joined: all of it when all of it is there — status OK or a hash mismatch —, else nothing
static inline u64 planes_join_len(const zpk_decode_desc& d, const zpk_decode_result& r)
{
    return (r.status == DEC_R_OK || r.status == DEC_R_FILE_HASH_MISMATCH) && r.produced == d.uncomp_size ? (u64)d.uncomp_size : 0ull;
}
// THE BASE RULE, beside it: an entry with a base is delivered only when its base hashes to the value the caller recorded.  A refused
// entry (Planes::refused_at) is joined with no byte, so its destination — with base == dst the previous checkpoint — stays as it was,
// and exactly where it would otherwise have been delivered, status OK or FILE_HASH_MISMATCH, its status becomes ZPK_R_BASE_MISMATCH
// (base_verdicts_mark, once the call's results are final); every other status stays the entry's own.  The verdicts are complete before
// the call's first row reaches rows_enqueue (base_verdicts runs in front of the routing), so all four delivery sites see them.
inline u64 Planes::join_len(u64 i, const zpk_decode_desc& d, const zpk_decode_result& r) const { return refused_at(i) ? 0ull : planes_join_len(d, r); }
// (the staging slot of an entry under either kind of destination, and under none: read_slot, host_plan.h)

// The words the stats calls report of the most recent call.  begin_decode_call zeroes the decode words; dimage, dsink and enc_big are
// zeroed by the one call that counts them; totals_valid by every launch, fell_back_fused by the launch that decides it.
struct LastCall {
    u32  big[2] = {0, 0};                        // host decode path: entries decoded frame-parallel or block-parallel, their frames / blocks
    u32  walk[2] = {0, 0};                       // zpk_codec_decode_big_batch_device: entries walked on the device, those the walk accepted
    u32  span[2] = {0, 0};                       // large stored entries copied chip-wide, their groups
    u32  pipe = 0, sc = 0;                       // host decode call: sub-batches that took the three-stage pipeline; k_span_copy launches
    u32  zpj_err = 0;                            // developer: the flag word of the most recent large Zstandard frame (why it went to the one-wave decoder)
    u32  dimage[3] = {0, 0, 0};                  // zpk_codec_decode_batch_dimage: its sub-batches, k_span_copy launches and the bytes it copied home (saturating)
    u32  subs = 0;                               // host decode call, device-image call: their sub-batches (zpk_codec_verify_stats reports them for the calls without a destination)
    u64  home = 0;                               // ... the PLAINTEXT bytes they copied home (saturating) — 0 for a call without a destination
    u32  vstored = 0;                            // zpk_codec_verify_batch_host / _dimage: stored entries hashed where they lay
    u32  dsink[2] = {0, 0};                      // zpk_codec_encode_batch_dsink: its sub-batches and the last grid of k_sink_place
    u32  enc_big[2] = {0, 0};                    // zpk_codec_encode_big_device: entries written in pieces, their pieces
    u32  delta[4] = {0, 0, 0, 0};                // zpk_codec_delta_stats: rows split with a base, rows joined with a base, k_delta_copy launches, entries staged only because they had a base
    u32  base_check[4] = {0, 0, 0, 0};           // zpk_codec_base_check_stats: rows hashed by one wave, rows hashed chip-wide, entries refused for their base, launches of the hash pass
    u32  window[3] = {0, 0, 0};                  // zpk_codec_window_stats: rows windowed, k_window_copy launches, entries staged only because they had a window
    u32  place[2] = {0, 0};                      // zpk_codec_place_stats: rows placed, k_place_copy launches
    void no_planes() { for (int k = 0; k < 4; k++) planes[k] = delta[k] = base_check[k] = 0; window[0] = window[1] = window[2] = 0; place[0] = place[1] = 0; }      // (a call that could split or join begins with this)
    u32  planes[4] = {0, 0, 0, 0};               // zpk_codec_planes_stats: rows split, rows joined, k_plane_copy launches, entries staged only because they were grouped
    int  fell_back_fused = 0;                    // the last decode batch could not get its sequence arena and ran the fused decoder only
    // the host-path pipeline decodes one call in several launches: their counters are brought back piece by piece and summed, so that
    // decode_stats / decode_stats2 describe the whole call (a retry or watchdog event in an early piece is not lost)
    u32  host_totals[N_COUNTERS] = {};
    int  totals_valid = 0;
};

// The row table of one of the row copies (row_table_enqueue): on the device, and pinned going up — the event says that the upload has
// run, the pinned block is written again only behind it.
struct RowTable { DevBuf<u8> d; PinBuf h; Event ev; bool pending = false; };

// Every HIP resource below is owned by the member that names it (codec_res.h): deleting the codec releases all of them.
// A growable pinned block (PinBuf) is regrown only while nothing on a stream still reads or writes it: a call that uses one drains the
// stream it put the copies on before it returns (walk.h_bigsrc, walk.h_bigwalk, sh.h: hipStreamSynchronize behind the copy home; sspan.h: the
// run waits for its stream on every way out, ~StoredSpanRun), or waits for the event behind its last upload before the block's next turn
// (bigenc.h, sc.h, pc.h, dc.h, wc.h, plc.h).  A call that FAILED may leave a copy behind: zpk_codec_reset waits for the codec's stream.
struct zpk_codec {
    int device = 0;
    Stream stream;
    // One codec = one in-flight batch: the work lists, counters and staging buffers below are shared by every call.
    // The host-pointer entry points (decode/encode_batch_host, hash_host, the streaming triple) take `mu` for their
    // whole duration, so threads that share a codec are serialised, never corrupted.  The device-pointer entry points
    // take it only while they enqueue: batches on ONE stream are ordered by the stream; a codec must not be driven
    // from two streams at once (create one codec per stream — contexts are cheap).
    pthread_mutex_t mu;
    char err[256] = {0};
    LastCall last;

    // zpk_codec_set_option
    struct {
        int  order_fast_last = 1;                          // ZPK_OPT_ORDER_FAST_LAST: a batch of one size class runs its incompressible entries last
        u64  order_min = 8192;                             // ZPK_OPT_ORDER_MIN: decode batches of at least this many entries run their work lists largest entries first
        u64  enc_order_min = 4608;                         // ... and encode batches their ticket queue (the encoder's resident waves: 18 per CU)
        u64  dec_split_min = ZPK_DEC_SPLIT_MIN_DEFAULT;    // ZPK_OPT_DEC_SPLIT_MIN: entries of at least this many bytes that ARE sequences of frames are decoded frame-parallel
        u64  enc_split_min = ZPK_ENC_SPLIT_MIN_DEFAULT;    // ZPK_OPT_ENC_SPLIT_MIN: entries of at least this many bytes are written as a sequence of frames
        u64  stored_span_min = ZPK_STORED_SPAN_MIN_DEFAULT; // ZPK_OPT_STORED_SPAN_MIN: stored entries of at least this many bytes go chip-wide
        u64  dimage_chunk = 0;                             // ZPK_OPT_DIMAGE_CHUNK (0 = the default): the staging of one sub-batch of an archive image in device memory (dimage_plan.h)
        u64  span_hash_min = ZPK_SPAN_HASH_MIN_DEFAULT;    // ZPK_OPT_SPAN_HASH_MIN: spans of at least this many bytes are hashed chip-wide (span_hash_plan.h)
    } opt;

    // staging every path shares
    DevBuf<u32> d_counters;                      // N_COUNTERS words (zpk_layout.h)
    DevBuf<u8>  d_src;                           // host-API staging
    DevBuf<u8>  d_dst;
    DevBuf<void> d_desc, d_res;
    DevBuf<u64> d_dbg;
    DevBuf<u8>  d_xpart;                         // span list | 64 bytes of XXH3 partial sums per 1 KiB block | hashes (xxh3_span.h): split entries of the host encode path, the block-parallel readers
    // timing (zpk_codec_timer_*, zpk_codec_set_profiling)
    Event ev0, ev1;
    Event kev[ZPK_K_COUNT][2];
    int profiling = 0;

    // the classify / one-wave launch (decode_launch)
    struct {
        DevBuf<u32> d_lists;                     // N_LIST_SLOTS work lists (zpk_layout.h); an ordered encode batch keeps its ticket queue here
        DevBuf<u8>  d_lit;
        DevBuf<u64> d_zarena;                    // pre-decoded Zstandard sequences, laid out like dst (zstd_fse4.h)
        DevBuf<u32> d_zstate;                    // per entry, 1 = its sequences are in the arena
        SideStream side;                         // the LZ4 kernels beside the Zstandard stages (low priority)
        SideStream left;                         // k_lz4_left (the LZ4 entries that are mostly runs) beside k_lz4_wave
        PinBlock<volatile SeenCounts> h_seen;    // pinned: the work-list counts of an earlier device batch (what the next one probably holds)
    } wave;

    // the host-pointer decode pipeline (pin_ready, d2h_scatter / h2d_gather, decode_host_pipelined)
    struct {
        PinBlock<u8> h_pin[2];                   // pinned staging of the host-pointer paths (ZPK_PIN_CHUNK bytes each), created on first use
        Event pin_ev[2];
        Stream s_up, s_dn;                       // upload / download streams beside `stream` (created on first use)
        Event ev[2 * 64];                        // per piece: uploaded, decoded
        PinBlock<u32[N_COUNTERS]> piece_counters; // [64], pinned (pin_ready): a D2H copy into pageable memory would block the launcher thread per piece
    } pipe;

    // the block-parallel readers of large single frames (lz4_pj.h, zstd_pj.h)
    struct {
        DevBuf<void> d_blocks, d_recs, d_masks, d_S;   // LZ4: block table, sequence records, start masks, byte references
        DevBuf<u32>  d_flags;                    // ... and flags (256 bytes)
        DevBuf<void> d_zblocks, d_zaux, d_zpos;  // Zstandard: block table; work items, states, final histories; sequence positions
        Event ev[ZPK_PJ_MAX_CHUNKS];             // one event behind every chunk of a large frame (its bytes may go home)
        PinBlock<u64> h_words;                   // 8 pinned words (pin_ready): hash and flags of a large frame come home without blocking the launcher
    } pj;

    // the walk over the block headers of large device-resident entries
    struct {
        PinBuf h_bigsrc;                         // pinned: the compressed bytes of one large device-resident entry, for the host's block walk (zpk_codec_decode_big_device)
        DevBuf<u8> d_bigwalk;                    // zpk_codec_decode_big_batch_device: candidates | records | block tables (k_big_walk)
        PinBuf h_bigwalk;                        // ... pinned: the candidates going up, the records and tables coming home
    } walk;

    // large stored entries of a device-resident call (stored_plan.h / stored_span.h): span table | destination offsets | 64 bytes of XXH3
    // partial sums per 1 KiB block | hashes — a buffer of its own, d_xpart belongs to the block-parallel readers of the same call
    struct {
        DevBuf<u8> d;
        PinBuf h;                                // pinned: the table going up, the hashes coming home
        SideStream side;                         // the second stream of the forked form (created on first use)
    } sspan;

    // plaintext in the caller's device memory: the row tables of k_span_copy, k_plane_copy, k_delta_copy, k_window_copy and k_place_copy
    // (row_copy.hip; span_copy_plan.h, plane_copy_plan.h, delta_copy_plan.h, window_copy_plan.h, place_copy_plan.h).  FIVE tables, not one
    // that takes turns: a call with entries of several kinds fills several of them before any of their kernels has run (rows_enqueue).
    RowTable sc, pc, dc, wc, plc;
    // the spans k_span_hash and the chip-wide pair hash (span_hash_plan.h / span_hash.h): tables | hashes | partial sums on the device,
    // the tables going up and the hashes coming home through a pinned block of its own — a call that hashes spans waits for its stream
    // behind the copy home, so the block is idle whenever the next call writes it
    struct { DevBuf<u8> d; PinBuf h; } sh;

    // the encoder
    DevBuf<u64> d_seq;                           // sequence lists, one per workgroup
    DevBuf<u8>  d_pack;                          // K7: block sums + span index of the compaction
    DevBuf<u8>  d_packed;                        // host encode path: packed payload stream
    DevBuf<u8>  d_packoff;                       // host encode path: payload offsets
    // zpk_codec_encode_big_device: the tables of one call (descriptors, pieces, entry table, spans) go up from pinned memory behind
    // whatever the stream still holds; two blocks take turns, the event says that a block's upload has run
    struct { PinBuf h[2]; Event ev[2]; u32 turn = 0; } bigenc;

    // a sink in the caller's device memory (dsink_plan.h / sink_commit.h): the slots a sub-batch is encoded into — d_dst holds the pieces
    // of its large entries meanwhile —, the commit's tables (results | cut record | offsets | slot offsets) and the resident workgroups of
    // k_sink_place (0: not asked yet)
    struct { DevBuf<u8> d_slots, d_tab; u32 groups = 0; } sink;
};

struct CodecLock {
    pthread_mutex_t* m;
    explicit CodecLock(zpk_codec* c) : m(&c->mu) { pthread_mutex_lock(m); }
    ~CodecLock() { pthread_mutex_unlock(m); }
    CodecLock(const CodecLock&) = delete;
    CodecLock& operator=(const CodecLock&) = delete;
};

#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    snprintf((c)->err, sizeof((c)->err), "%s: %s", #call, hipGetErrorString(e_)); return ZPK_E_LAUNCH; } } while (0)

static int grow(zpk_codec* c, DevBufBase& b, u64 need)
{
    if (need <= b.cap) return ZPK_OK;
    // the buffer may still be in use by work enqueued earlier on the codec's stream or the caller's
    if (b.p) { (void)hipDeviceSynchronize(); b.release(); }
    u64 want = need + need / 4 + 4096;
    if (!b.alloc(want)) {
        want = need + 256;                                                          // the slack was a convenience, not a need
        if (!b.alloc(want)) { snprintf(c->err, sizeof(c->err), "hipMalloc(%llu) failed", (unsigned long long)want); return ZPK_E_NOMEM; }
    }
    return ZPK_OK;
}

extern "C" {

int zpk_codec_abi_version(void) { return ZPK_CODEC_ABI_VERSION; }

int zpk_codec_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int zpk_codec_create(zpk_codec** out, int device)
{
    if (!out) return ZPK_E_INVALID;
    *out = nullptr;
    int n = zpk_codec_device_count();
    if (n <= 0) return ZPK_E_NO_DEVICE;
    if (device < 0) {
        const char* e = getenv("ZPACK_AMD_DEVICE");
        if (!e) e = getenv("LOCAL_RANK");
        device = e ? atoi(e) : 0;
        if (device < 0 || device >= n) device = 0;
    }
    if (device >= n) return ZPK_E_INVALID;
    zpk_codec* c = new (std::nothrow) zpk_codec();
    if (!c) return ZPK_E_NOMEM;
    c->device = device;
    {   // recursive: the host entry points call the device ones underneath
        pthread_mutexattr_t at; pthread_mutexattr_init(&at); pthread_mutexattr_settype(&at, PTHREAD_MUTEX_RECURSIVE);
        pthread_mutex_init(&c->mu, &at); pthread_mutexattr_destroy(&at);
    }
    if (hipSetDevice(device) != hipSuccess || c->stream.ready(hipStreamNonBlocking) != hipSuccess ||
        !c->d_counters.ensure(N_COUNTERS * sizeof(u32)) ||
        c->ev0.ready(hipEventDefault) != hipSuccess || c->ev1.ready(hipEventDefault) != hipSuccess) {
        zpk_codec_destroy(c);                                                       // (whatever exists by now goes with it)
        return ZPK_E_NO_DEVICE;
    }
    *out = c;
    return ZPK_OK;
}

// the members own what they hold (codec_res.h): on the codec's device, behind whatever its stream still carries
void zpk_codec_destroy(zpk_codec* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    pthread_mutex_destroy(&c->mu);
    delete c;
}

// after an abandoned stream / a failed call (the reference resets its library context: lib/zpack_read.c:679-690): wait for
// whatever the codec still has in flight and forget the last error; every later call starts from a clean context
void zpk_codec_reset(zpk_codec* c)
{
    if (!c) return;
    CodecLock lk(c);
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    c->err[0] = 0;
    // a context keeps its grown staging between batches (the next batch of that size starts at once); a reset gives the large pieces
    // back — a process that holds many readers can bound what each one retains (zpack_reset_reader_dctx / zpack_reset_writer_cctx)
    const u64 keep = 64ull << 20;
    for (DevBufBase* b : { (DevBufBase*)&c->d_src, (DevBufBase*)&c->d_dst, (DevBufBase*)&c->wave.d_zarena, (DevBufBase*)&c->wave.d_lit, (DevBufBase*)&c->sink.d_slots }) if (b->cap > keep) b->release();
}
const char* zpk_codec_last_error(const zpk_codec* c) { return c ? c->err : "no codec"; }
int zpk_codec_device(const zpk_codec* c) { return c ? c->device : -1; }

// Developer hooks (ZPK_TRACE / ZPK_SKIP / ZPK_DEBUG_TIMING environment switches) exist only in a -DZPK_DEVELOPER build:
// the product launch path reads no environment and can neither drop a kernel nor end the host process.
#ifdef ZPK_DEVELOPER
#define ZPK_DEV(x) x
#define ZPK_WD_ARG , c->d_dbg, wd_scale
#else
#define ZPK_DEV(x)
#define ZPK_WD_ARG
#endif

// ---- memory of the caller's ON THE DEVICE: the pointer rule, the checked copy, the row copies' tables (copy_rows_plan.h, row_copy.hip) -----------
// THE QUERY, the one place that asks HIP about a caller's address: which device it lies on and which allocation [base, base + size) holds it.
// ZPK_OK: *r says so; ZPK_E_INVALID: NULL, host memory (HIP may never have seen it: its last error is cleared), memory of another device
// than `only` (that device is not entered; DEV_ANY: every device will do, DEV_NONE: none, the caller wants r->device alone), or no
// allocation; ZPK_E_LAUNCH: the allocation's device could not be entered.
// r->device is the memory's device whenever it is device memory, whatever else fails; -1 otherwise.  The current device is entered through
// `on`, which puts it back when it goes: at the end of the call or, handed in by the caller, when the caller is done with that device.
struct DevRange { int device; u64 base, size; };
enum { DEV_ANY = -1, DEV_NONE = -2 };
struct OnDevice {
    int was = -1, now = -1;
    bool enter(int device)
    {
        if (hipGetDevice(&was) != hipSuccess) { (void)hipGetLastError(); was = -1; }
        if (was != device && hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return false; }
        now = device;
        return true;
    }
    OnDevice() {}
    ~OnDevice() { if (now >= 0 && was >= 0 && was != now) (void)hipSetDevice(was); }
    OnDevice(const OnDevice&) = delete;
    OnDevice& operator=(const OnDevice&) = delete;
};
static int device_range_of(const void* ptr, DevRange* r, int only, OnDevice* stay = nullptr)
{
    *r = DevRange{ -1, 0, 0 };
    hipPointerAttribute_t at;
    if (!ptr || hipPointerGetAttributes(&at, ptr) != hipSuccess) { (void)hipGetLastError(); return ZPK_E_INVALID; }
    if (at.type != hipMemoryTypeDevice) return ZPK_E_INVALID;
    r->device = at.device;
    if (only != DEV_ANY && at.device != only) return ZPK_E_INVALID;
    OnDevice here;
    if (!(stay ? stay : &here)->enter(at.device)) return ZPK_E_LAUNCH;
    hipDeviceptr_t base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr) != hipSuccess) { (void)hipGetLastError(); return ZPK_E_INVALID; }
    r->base = (u64)base; r->size = (u64)size;
    return ZPK_OK;
}
// The rule — [ptr, ptr + len) lies inside ONE allocation (span_copy_in_range; no bytes pass wherever they point) — under its two policies:
//   a BATCH call (PtrRule) demands the codec's own device, before anything is enqueued.  The last allocation seen is kept while the rule
//     object lives, which is one call — the caller may free the buffer afterwards —, so a batch into one buffer is one query;
//   the instance-free copy (checked_copy: zpk_codec_fetch_device / _store_device) accepts any device and enters it for the copy.
extern "C++" {
struct PtrRule {
    zpk_codec* const c;
    DevRange last = { -1, 0, 0 };
    explicit PtrRule(zpk_codec* codec) : c(codec) {}
    bool ok(const void* ptr, u64 len)
    {
        if (len == 0) return true;
        if (!ptr) return false;
        if (last.size && span_copy_in_range((u64)ptr, len, last.base, last.size)) return true;
        DevRange r;
        if (device_range_of(ptr, &r, c->device) != ZPK_OK) return false;
        last = r;
        return span_copy_in_range((u64)ptr, len, r.base, r.size);
    }
    // entries [0, n) of a batch, `noun` i at ptr(i) with len(i) bytes; ZPK_E_INVALID with the message written
    template <class PtrFn, class LenFn>
    int batch(const char* noun, u64 n, PtrFn ptr, LenFn len)
    {
        for (u64 i = 0; i < n; i++)
            if (!ok(ptr(i), len(i))) {
                snprintf(c->err, sizeof(c->err), "%s %llu is not %llu bytes of one allocation on device %d", noun, (unsigned long long)i, (unsigned long long)len(i), c->device);
                return ZPK_E_INVALID;
            }
        return ZPK_OK;
    }
};
}  // extern "C++"

// instance-free: `bytes` bytes between [d_ptr, + bytes), when that lies inside one allocation in device memory, and `host` (none: the check
// alone); the memory's device is entered once, for the query and the copy
static int checked_copy(const void* d_ptr, void* host, u64 bytes, hipMemcpyKind dir)
{
    if (zpk_codec_device_count() <= 0) return ZPK_E_NO_DEVICE;
    if (bytes == 0) return ZPK_OK;
    OnDevice on;
    DevRange r;
    const int rc = device_range_of(d_ptr, &r, DEV_ANY, &on);
    if (rc) return rc;
    if (!span_copy_in_range((u64)d_ptr, bytes, r.base, r.size)) return ZPK_E_INVALID;
    const bool up = dir == hipMemcpyHostToDevice;
    if (host && hipMemcpy(up ? (void*)d_ptr : host, up ? host : d_ptr, bytes, dir) != hipSuccess) { (void)hipGetLastError(); return ZPK_E_LAUNCH; }
    return ZPK_OK;
}
int zpk_codec_fetch_device(const void* d_src, void* host_dst, uint64_t bytes) { return checked_copy(d_src, host_dst, bytes, hipMemcpyDeviceToHost); }
int zpk_codec_store_device(void* d_dst, const void* host_src, uint64_t bytes) { return checked_copy(d_dst, (void*)host_src, bytes, hipMemcpyHostToDevice); }
// the device whose memory `ptr` is, -1 for anything else: the memory's kind alone decides, as a host must not read through such a pointer
int zpk_codec_pointer_device(const void* ptr) { DevRange r; (void)device_range_of(ptr, &r, DEV_NONE); return r.device; }

// The skeleton of the five row copies: the entries [0, n) of which takes(i) says whether entry i takes a row of table `t`, in ONE kernel
// on `st` (a table past one grid: several, over the same table); returns when the table's upload and the kernel are enqueued.  The rows
// are written straight into the pinned table by emit(i, rows, p) — false: ZPK_E_INVALID, nothing is uploaded or launched —, so an entry
// is asked twice, once for the count; launch(d_rows, nrows, L) enqueues one launch.  No rows: nothing is touched.
extern "C++" {
template <class Row, class TakesFn, class EmitFn, class LaunchFn>
static int row_table_enqueue(zpk_codec* c, RowTable& t, const char* what, u64 n, TakesFn takes, EmitFn emit, LaunchFn launch, hipStream_t st)
{
    u64 nz = 0;
    for (u64 i = 0; i < n; i++) nz += takes(i) ? 1 : 0;
    if (nz == 0) return ZPK_OK;
    if (nz > ZPK_COPY_MAX_ROWS) return ZPK_E_INVALID;
    if (t.pending) { HIPCHK(c, hipEventSynchronize(t.ev)); t.pending = false; }                         // the pinned block's last upload has run
    if (t.ev.ready(hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); snprintf(c->err, sizeof(c->err), "%s: no event", what); return ZPK_E_LAUNCH; }
    if (!t.h.grow(nz * sizeof(Row))) { snprintf(c->err, sizeof(c->err), "%s: out of pinned memory", what); return ZPK_E_NOMEM; }
    int rc;
    if ((rc = grow(c, t.d, nz * sizeof(Row)))) return rc;
    Row* const rows = (Row*)t.h.p;
    CopyPlan p = { 0, 0 };
    for (u64 i = 0; i < n; i++) if (!emit(i, rows, p)) return ZPK_E_INVALID;
    HIPCHK(c, hipMemcpyAsync(t.d, rows, p.nrows * sizeof(Row), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(t.ev, st));
    t.pending = true;
    const u64 nl = copy_launches(p.items);
    for (u64 j = 0; j < nl; j++) launch((const Row*)(const u8*)t.d, (u32)p.nrows, copy_launch(p.items, j));
    HIPCHK(c, hipGetLastError());
    return ZPK_OK;
}
// k_span_copy: entry i the span row(i) (a zpk_span_copy; no bytes: no row).  The pointers have been checked by the caller, or are the
// codec's own.
template <class RowFn>
static int span_copy_enqueue(zpk_codec* c, u64 n, RowFn row, hipStream_t st)
{
    return row_table_enqueue<SpanCopyRow>(c, c->sc, "span copy", n, [&](u64 i) { return row(i).len != 0; },
        [&](u64 i, SpanCopyRow* rows, CopyPlan& p) { const zpk_span_copy s = row(i); return span_copy_emit(s.src, s.dst, s.len, rows, p); },
        [&](const SpanCopyRow* d, u32 nrows, const CopyLaunch& L) { span_copy_launch(d, nrows, L.item0, L.items, L.grid, st); c->last.sc++; }, st);
}
// k_plane_copy: entry i the row row(i) (a zpk_plane_copy; no bytes: no row).  The element sizes have been checked by the caller
// (planes_check).
template <class RowFn>
static int plane_copy_enqueue(zpk_codec* c, u64 n, RowFn row, hipStream_t st)
{
    return row_table_enqueue<PlaneCopyRow>(c, c->pc, "plane copy", n, [&](u64 i) { return row(i).len != 0; },
        [&](u64 i, PlaneCopyRow* rows, CopyPlan& p) {
            const zpk_plane_copy s = row(i);
            if (!plane_copy_emit(s.src, s.dst, s.len, s.elem, s.join, rows, p)) return false;
            if (s.len) c->last.planes[s.join ? 1 : 0]++;
            return true;
        },
        [&](const PlaneCopyRow* d, u32 nrows, const CopyLaunch& L) { plane_copy_launch(d, nrows, L.item0, L.items, L.grid, st); c->last.planes[2]++; }, st);
}
// k_delta_copy: entry i the row row(i) (a zpk_delta_copy; no bytes: no row).  Element sizes, bases and their overlap with the
// destinations have been checked by the caller.
template <class RowFn>
static int delta_copy_enqueue(zpk_codec* c, u64 n, RowFn row, hipStream_t st)
{
    return row_table_enqueue<DeltaCopyRow>(c, c->dc, "delta copy", n, [&](u64 i) { return row(i).len != 0; },
        [&](u64 i, DeltaCopyRow* rows, CopyPlan& p) {
            const zpk_delta_copy s = row(i);
            if (!delta_copy_emit(s.src, s.dst, s.base, s.len, s.elem, s.join, rows, p)) return false;
            if (s.len) c->last.delta[s.join ? 1 : 0]++;
            return true;
        },
        [&](const DeltaCopyRow* d, u32 nrows, const CopyLaunch& L) { delta_copy_launch(d, nrows, L.item0, L.items, L.grid, st); c->last.delta[2]++; }, st);
}
// k_window_copy: entry i the row row(i) (a zpk_window_copy; an entry or a window of no bytes: no row).  Element sizes, windows
// (window_valid), bases and their overlap with the destinations have been checked by the caller; a window that fails the rule all the
// same: ZPK_E_INVALID and nothing is launched.
template <class RowFn>
static int window_copy_enqueue(zpk_codec* c, u64 n, RowFn row, hipStream_t st)
{
    auto bytes = [](const zpk_window_copy& s) { return s.n ? s.win.rows * s.win.cols : 0ull; };
    return row_table_enqueue<WindowCopyRow>(c, c->wc, "window copy", n, [&](u64 i) { return bytes(row(i)) != 0; },
        [&](u64 i, WindowCopyRow* rows, CopyPlan& p) {
            const zpk_window_copy s = row(i);
            if (!bytes(s)) return true;
            if (!window_copy_emit(s.src, s.dst, s.base, s.n, Window{ s.win.row_bytes, s.win.row0, s.win.rows, s.win.col0, s.win.cols }, s.elem, rows, p)) return false;
            c->last.window[0]++;
            return true;
        },
        [&](const WindowCopyRow* d, u32 nrows, const CopyLaunch& L) { window_copy_launch(d, nrows, L.item0, L.items, L.grid, st); c->last.window[1]++; }, st);
}
// k_place_copy: entry i the row row(i) (a zpk_place_copy; an entry or a window of no bytes: no row).  Element sizes, placements
// (place_valid), bases and their overlap with the destinations have been checked by the caller; a placement that fails the rule all the
// same: ZPK_E_INVALID and nothing is launched.
template <class RowFn>
static int place_copy_enqueue(zpk_codec* c, u64 n, RowFn row, hipStream_t st)
{
    auto bytes = [](const zpk_place_copy& s) { return s.n ? s.win.rows * s.win.cols : 0ull; };
    return row_table_enqueue<PlaceCopyRow>(c, c->plc, "place copy", n, [&](u64 i) { return bytes(row(i)) != 0; },
        [&](u64 i, PlaceCopyRow* rows, CopyPlan& p) {
            const zpk_place_copy s = row(i);
            if (!bytes(s)) return true;
            if (!place_copy_emit(s.src, s.dst, s.base, s.n, Window{ s.win.row_bytes, s.win.row0, s.win.rows, s.win.col0, s.win.cols }, s.pitch, s.elem, rows, p)) return false;
            c->last.place[0]++;
            return true;
        },
        [&](const PlaceCopyRow* d, u32 nrows, const CopyLaunch& L) { place_copy_launch(d, nrows, L.item0, L.items, L.grid, st); c->last.place[1]++; }, st);
}
// The spans row(i) of a batch with element sizes, bases, windows and pitches `pl`, all of one direction (join: PLANE_SPLIT / PLANE_JOIN),
// split FIVE ways: those with a window and a pitch in ONE k_place_copy, even where pitch == cols; those with a window and none in ONE
// k_window_copy, whatever their element size or base (row(i).len is the entry's plain size there,
// or 0: nothing is delivered); of the others those with a base in ONE k_delta_copy, those without a base and with an element size above 1
// in ONE k_plane_copy, the rest in ONE k_span_copy as ever.  No element sizes, bases or windows: span_copy_enqueue and nothing else; no
// windows: what it was before there were any.
template <class RowFn>
static int rows_enqueue(zpk_codec* c, u64 n, RowFn row, const Planes& pl, u32 join, hipStream_t st)
{
    if (!pl.any()) return span_copy_enqueue(c, n, row, st);
    int rc = span_copy_enqueue(c, n, [&](u64 i) { zpk_span_copy s = row(i); if (pl.grouped(i)) s.len = 0; return s; }, st);
    if (rc) return rc;
    rc = plane_copy_enqueue(c, n, [&](u64 i) { const zpk_span_copy s = row(i); const u32 k = pl.of(i); return zpk_plane_copy{ s.src, s.dst, k > 1 && !pl.base_of(i) && !pl.windowed(i) ? s.len : 0ull, k, join }; }, st);
    if (rc) return rc;
    if (pl.base) rc = delta_copy_enqueue(c, n, [&](u64 i) { const zpk_span_copy s = row(i); const u8* const b = pl.base_of(i); return zpk_delta_copy{ s.src, s.dst, (u64)b, b && !pl.windowed(i) ? s.len : 0ull, pl.of(i), join }; }, st);
    if (rc || !pl.win) return rc;
    rc = window_copy_enqueue(c, n, [&](u64 i) {
        const zpk_span_copy s = row(i);
        return zpk_window_copy{ s.src, s.dst, (u64)pl.base_of(i), pl.windowed(i) && !pl.placed(i) ? s.len : 0ull, pl.win[i], pl.of(i), 0u };
    }, st);
    if (rc || !pl.pitch) return rc;
    return place_copy_enqueue(c, n, [&](u64 i) {
        const zpk_span_copy s = row(i);
        return zpk_place_copy{ s.src, s.dst, (u64)pl.base_of(i), pl.placed(i) ? s.len : 0ull, pl.win[i], pl.pitch[i], pl.of(i), 0u };
    }, st);
}
}  // extern "C++"
// false, with the message: `elem` is no element size (plane_elem_valid) — of entry i of a batch, or row i of a table (`noun`)
static bool elem_size_ok(zpk_codec* c, const char* noun, u64 i, u32 elem)
{
    if (plane_elem_valid(elem)) return true;
    snprintf(c->err, sizeof(c->err), "%s %llu: an element size of %u (1, 2, 4 or 8)", noun, (unsigned long long)i, (unsigned)elem);
    return false;
}
static int planes_check(zpk_codec* c, const u8* elem, u64 n)
{
    for (u64 i = 0; elem && i < n; i++) if (!elem_size_ok(c, "entry", i, elem[i])) return ZPK_E_INVALID;
    return ZPK_OK;
}
// ZPK_E_INVALID, before anything is enqueued: a base (those that are not NULL) that fails the pointer rule over len(i) bytes, or — where
// there are destinations, reading — one that overlaps its entry's destination other than exactly (delta_overlap_ok)
extern "C++" {
template <class LenFn>
static int bases_check(zpk_codec* c, PtrRule& rule, const Planes& pl, u64 n, LenFn len, uint8_t* const* dst_ptrs)
{
    if (!pl.base) return ZPK_OK;
    if (rule.batch("base", n, [&](u64 i) { return (const void*)pl.base[i]; }, [&](u64 i) { return pl.base[i] ? len(i) : 0ull; })) return ZPK_E_INVALID;
    for (u64 i = 0; dst_ptrs && i < n; i++)
        if (pl.base[i] && !delta_overlap_ok((u64)pl.base[i], (u64)dst_ptrs[i], len(i))) {
            snprintf(c->err, sizeof(c->err), "base %llu overlaps its destination without being it", (unsigned long long)i);
            return ZPK_E_INVALID;
        }
    return ZPK_OK;
}

}  // extern "C++"
// The windows of a batch and the pitches of those that are placed, before anything is enqueued.  ZPK_E_INVALID: a window that fails
// window_valid against its entry's uncomp_size and element size, a pitch on an entry without a window or one that fails place_valid with
// it, or either on a batch whose destinations are not device memory.  `staged` becomes the descriptors as the routing is to
// see them when an entry has a window (else it stays empty): such an entry decodes into the codec's staging with a slot of uncomp_size
// — its dst_capacity counts as that; the caller's says what room its buffer has, window_bytes (of a placed entry place_extent:
// Planes::dst_len) is all the delivery needs of it, and with
// less the capacity counts as 0: the entry earns BUFFER_TOO_SMALL from the kernels' guards, in their order, and nothing is delivered.
static int windows_check(zpk_codec* c, const Planes& pl, const zpk_decode_desc* desc, u64 n, bool ddst, std::vector<zpk_decode_desc>& staged)
{
    staged.clear();
    bool any = false;
    for (u64 i = 0; pl.pitch && i < n; i++) {                                          // the placements: a pitch belongs to a window, and the pair passes place_valid
        if (!pl.pitch[i]) continue;
        if (!ddst || !pl.windowed(i) || !place_valid(desc[i].uncomp_size, pl.of(i), pl.window_of(i), pl.pitch[i])) {
            snprintf(c->err, sizeof(c->err), "entry %llu: a pitch of %llu %s", (unsigned long long)i, (unsigned long long)pl.pitch[i],
                     !ddst ? "(placements belong to device destinations)" : !pl.windowed(i) ? "without a window" : "that its window does not fit, or an extent that wraps");
            return ZPK_E_INVALID;
        }
    }
    for (u64 i = 0; pl.win && i < n; i++) {
        if (!pl.windowed(i)) continue;
        if (!ddst || !window_valid(desc[i].uncomp_size, pl.of(i), pl.window_of(i))) {
            snprintf(c->err, sizeof(c->err), "entry %llu: its window does not lie in %llu bytes of %u-byte elements%s", (unsigned long long)i, (unsigned long long)desc[i].uncomp_size,
                     (unsigned)pl.of(i), ddst ? "" : " (windows belong to device destinations)");
            return ZPK_E_INVALID;
        }
        any = true;
    }
    if (!any) return ZPK_OK;
    try { staged.assign(desc, desc + n); } catch (...) { return ZPK_E_NOMEM; }
    for (u64 i = 0; i < n; i++) if (pl.windowed(i)) staged[i].dst_capacity = desc[i].dst_capacity < pl.dst_len(i, 0) ? 0 : desc[i].uncomp_size;     // (a placed one: place_extent)
    return ZPK_OK;
}
// base_hash[i] is the XXH3 of a contiguous span, and the base of a placed entry is not one: ZPK_E_INVALID, before anything runs, for a
// placed entry with a base in a call that checks bases — unless its extent IS its window's bytes (one row, or pitch == cols), which is
// checked as ever.  (The caller hashes its whole merged base once: zpk_codec_hash_spans_device.)
static int placed_hash_check(zpk_codec* c, const Planes& pl, const u64* base_hash, u64 n)
{
    for (u64 i = 0; pl.pitch && pl.base && base_hash && i < n; i++)
        if (pl.placed(i) && pl.base[i] && place_extent(pl.window_of(i), pl.pitch[i]) != window_bytes(pl.window_of(i))) {
            snprintf(c->err, sizeof(c->err), "entry %llu: a placed base is no contiguous span, there is no hash to check it by", (unsigned long long)i);
            return ZPK_E_INVALID;
        }
    return ZPK_OK;
}
extern "C++" {

// XXH3-64 of the spans row(i) = SpanHashRow{ address, len }, i in [0, n), into out[0, n) (HOST memory): the two tables of span_hash_plan.h
// go up from the codec's pinned block, one pass of launches follows (span_hash_launch: k_span_hash for the short rows, the partial sums
// and the chains for the long ones), the hashes come home and the stream is waited for.  The addresses have passed the pointer rule.
// Adds to last.base_check[0], [1] and [3].
template <class RowFn>
static int span_hash_run(zpk_codec* c, u64 n, RowFn row, u64* out, hipStream_t st)
{
    if (n == 0) return ZPK_OK;
    if (n > ZPK_SPAN_HASH_MAX_ROWS) { snprintf(c->err, sizeof(c->err), "span hash: %llu rows", (unsigned long long)n); return ZPK_E_INVALID; }
    const u64 thr = c->opt.span_hash_min;
    SpanHashPlan sized = { 0, 0, 0, 0 };
    for (u64 i = 0; i < n; i++) {
        const u64 len = row(i).len;
        if (span_hash_wide(len, thr)) { sized.nwide++; sized.part_blocks += xxh3_span_blocks(len); } else sized.nwave++;
    }
    const SpanHashLayout L = span_hash_layout(sized);
    if (!c->sh.h.grow(L.partial)) { snprintf(c->err, sizeof(c->err), "span hash: out of pinned memory"); return ZPK_E_NOMEM; }
    int rc;
    if ((rc = grow(c, c->sh.d, L.bytes))) return rc;
    SpanHashRow* const wave = (SpanHashRow*)(c->sh.h.p + L.wave_rows);
    SpanHashWide* const wide = (SpanHashWide*)(c->sh.h.p + L.wide_rows);
    const u64* const home = (const u64*)(c->sh.h.p + L.out);
    std::vector<u64> kept;
    try { kept.resize(n); } catch (...) { return ZPK_E_NOMEM; }
    SpanHashPlan p = { 0, 0, 0, 0 };
    for (u64 i = 0; i < n; i++) { const SpanHashRow r = row(i); kept[i] = span_hash_emit(r.addr, r.len, thr, wave, wide, p); }
    HIPCHK(c, hipMemcpyAsync(c->sh.d, c->sh.h.p, L.up_bytes, hipMemcpyHostToDevice, st));
    const u32 launches = span_hash_launch(c->sh.d, p, L, ZPK_SPAN_HASH_MAX_WAVE_ROWS, ZPK_SPAN_HASH_MAX_GROUPS, ZPK_SPAN_HASH_MAX_CHAINS, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->sh.h.p + L.out, c->sh.d + L.out, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (u64 i = 0; i < n; i++) out[i] = home[span_hash_out_slot(kept[i], p.nwave)];
    c->last.base_check[0] += (u32)p.nwave; c->last.base_check[1] += (u32)p.nwide; c->last.base_check[3] += launches;
    return ZPK_OK;
}

// The verdicts of the base rule (beside planes_join_len) for a batch: the bases that are there are hashed in ONE pass on the codec's
// stream, in front of everything the call enqueues, and compared with base_hash[i]; refused[i] = 1 where they differ.  No bases or no
// hashes: `refused` stays empty and nothing runs — the call is the _delta call.  (The pass could run on a second stream beside the first
// sub-batch's decode; it is waited for here instead, which keeps every delivery site behind the verdicts without an event per site —
// profiles/r31 has what that costs.)
template <class LenFn>
static int base_verdicts(zpk_codec* c, const Planes& pl, const u64* base_hash, u64 n, LenFn len, std::vector<u8>& refused)
{
    refused.clear();
    if (!pl.base || !base_hash) return ZPK_OK;
    try {
        std::vector<u64> idx;
        for (u64 i = 0; i < n; i++) if (pl.base[i]) idx.push_back(i);
        if (idx.empty()) return ZPK_OK;
        std::vector<u64> h(idx.size());
        const int rc = span_hash_run(c, idx.size(), [&](u64 k) { return SpanHashRow{ (u64)pl.base[idx[k]], len(idx[k]) }; }, h.data(), c->stream);
        if (rc) return rc;
        refused.assign(n, 0);
        for (u64 k = 0; k < idx.size(); k++) if (h[k] != base_hash[idx[k]]) { refused[idx[k]] = 1; c->last.base_check[2]++; }
    } catch (...) { return ZPK_E_NOMEM; }
    return ZPK_OK;
}
}  // extern "C++"
// ... and the status of the refused entries, once the call's results are final
static void base_verdicts_mark(const std::vector<u8>& refused, const zpk_decode_desc* desc, zpk_decode_result* results, u64 n)
{
    for (u64 i = 0; i < n && !refused.empty(); i++)
        if (refused[i] && (results[i].status == DEC_R_OK || results[i].status == DEC_R_FILE_HASH_MISMATCH) && results[i].produced == desc[i].uncomp_size)
            results[i].status = ZPK_R_BASE_MISMATCH;                                  // (the condition of planes_join_len, with nothing to join counting as delivered)
}

// XXH3-64 of `nspans` long spans of `base` (xxh3_span.h): enqueues the upload of the span list and the two kernels; the hashes stay on
// the device, *d_hash_out says where (inside c->d_xpart, valid until the next call that hashes spans).  `h_spans` must stay as it is
// until the upload has run: the caller synchronises, or hands pinned memory it keeps.
static int xxh3_spans_enqueue(zpk_codec* c, const u8* base, const zpk_span* h_spans, u64 nspans, u64 part_blocks, u64** d_hash_out, hipStream_t st)
{
    *d_hash_out = nullptr;
    if (nspans == 0) return ZPK_OK;
    if (nspans > 0x7FFFFFFFull) return ZPK_E_INVALID;
    const u64 span_bytes = (nspans * sizeof(zpk_span) + 255) & ~255ull, part_bytes = part_blocks * 64;
    int rc;
    if ((rc = grow(c, c->d_xpart, span_bytes + part_bytes + nspans * 8 + 64))) return rc;
    zpk_span* d_spans = (zpk_span*)c->d_xpart;
    u64* d_part = (u64*)(c->d_xpart + span_bytes);
    u64* d_hash = (u64*)(c->d_xpart + span_bytes + part_bytes);
    HIPCHK(c, hipMemcpyAsync(d_spans, h_spans, nspans * sizeof(zpk_span), hipMemcpyHostToDevice, st));
    const u64 ngroups = part_blocks / XS_GROUP;
    if (ngroups) hipLaunchKernelGGL(k_xxh3_partials, dim3((u32)((ngroups + 3) / 4)), dim3(256), 0, st, base, (const zpk_span*)d_spans, (u32)nspans, (u64)0, ngroups, d_part);
    hipLaunchKernelGGL(k_xxh3_chain, dim3((u32)nspans), dim3(64), 0, st, base, (const zpk_span*)d_spans, (const u64*)d_part, d_hash, (u64*)nullptr, (u64)0, ~(u64)0, 1);
    HIPCHK(c, hipGetLastError());
    *d_hash_out = d_hash;
    return ZPK_OK;
}
// ... and the copy of the hashes to `h_hash`
static int xxh3_spans_launch(zpk_codec* c, const u8* base, const zpk_span* h_spans, u64 nspans, u64 part_blocks, u64* h_hash, hipStream_t st)
{
    u64* d_hash = nullptr;
    const int rc = xxh3_spans_enqueue(c, base, h_spans, nspans, part_blocks, &d_hash, st);
    if (rc || !d_hash) return rc;
    HIPCHK(c, hipMemcpyAsync(h_hash, d_hash, nspans * 8, hipMemcpyDeviceToHost, st));
    return ZPK_OK;
}
// (xxh3_span_blocks, the partial-sum slots of one span: stored_plan.h)

// Fork: work enqueued on x.s from here on runs beside `from`, behind everything `from` holds now.  The stream (low_priority: at
// the device's lowest) and the two events are created on first use; false = no second stream, the caller stays on `from`.
static bool fork_stream(SideStream& x, hipStream_t from, bool low_priority)
{
    if (!x.s) {
        int lo_prio = 0, hi_prio = 0;
        if (low_priority) (void)hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio);
        (void)(low_priority ? x.s.ready_priority(hipStreamNonBlocking, lo_prio) : x.s.ready(hipStreamNonBlocking));
    }
    (void)x.fork.ready(hipEventDisableTiming);
    (void)x.join.ready(hipEventDisableTiming);
    return x.s && x.fork && x.join && hipEventRecord(x.fork, from) == hipSuccess && hipStreamWaitEvent(x.s, x.fork, 0) == hipSuccess;
}
// Join: `into` goes on behind what x.s holds; when that cannot be enqueued the host waits for x.s instead.
static void join_stream(SideStream& x, hipStream_t into)
{
    if (hipEventRecord(x.join, x.s) != hipSuccess || hipStreamWaitEvent(into, x.join, 0) != hipSuccess) (void)hipStreamSynchronize(x.s);
}

// hash_only: the batch has no destination (Dst::None) — its stored entries have no slot in dst and are hashed where they lie
// (k_stored_hash in place of k_stored); everything else decodes into its slot as ever.
static int decode_launch(zpk_codec* c, BatchMethods holds, const u8* src, u64 src_size, const u8* read_lo, const u8* read_hi,
                         const zpk_decode_desc* desc, u64 n, u8* dst, u64 dst_size, zpk_decode_result* res, hipStream_t st, bool hash_only = false)
{
    if (n == 0) return ZPK_OK;
    if (n > 0x7FFFFFF0ull) return ZPK_E_INVALID;               // one workgroup per LZ4 entry: the grid's x limit
    c->last.totals_valid = 0;                                        // (the pipeline sets it again once it has summed its pieces)
    int rc;
    if ((rc = grow(c, c->wave.d_lists, N_LIST_SLOTS * n * sizeof(u32)))) return rc;
    const u64 stride = c->wave.d_lists.cap / (N_LIST_SLOTS * sizeof(u32));
    auto list_at = [&](int slot) { return c->wave.d_lists + (u64)slot * stride; };
    u32* const retry_lz4 = list_at(S_RETRY_LZ4);
    u32* const retry_zstd = list_at(S_RETRY_ZSTD);
    u32* const left_lz4 = list_at(S_LZ4_RUNS);
    u32* const handed_lz4 = list_at(S_LZ4_HANDED);
    u32 wd_scale = 1; (void)wd_scale;
    ZPK_DEV(static const int wd_env = getenv("ZPK_WD_SCALE") ? atoi(getenv("ZPK_WD_SCALE")) : 1; wd_scale = (u32)wd_env;)
    int skip = 0; (void)skip;
#ifdef ZPK_DEVELOPER
    static const int want_dbg = getenv("ZPK_DEBUG_TIMING") ? atoi(getenv("ZPK_DEBUG_TIMING")) : 0;
    if (want_dbg) { if ((rc = grow(c, c->d_dbg, n * 128))) return rc; }
    static const int trace = getenv("ZPK_TRACE") ? atoi(getenv("ZPK_TRACE")) : 0;
    static const int skip_env = getenv("ZPK_SKIP") ? atoi(getenv("ZPK_SKIP")) : 0;      // bitmask: 1 stored, 2 lz4, 4 zstd
    skip = skip_env;
#define ZPK_TRACE_STEP(name) do { if (trace == 1) { hipError_t te_ = hipStreamSynchronize(st); \
        fprintf(stderr, "[zpk] %s done: %s\n", name, hipGetErrorString(te_)); fflush(stderr); } } while (0)
#else
#define ZPK_TRACE_STEP(name) do { } while (0)
#endif
    const u32 zstd_grid = (u32)(n < ZSTD_GRID_MAX ? n : ZSTD_GRID_MAX);
    const u32 exec_grid = (u32)(n < ZSTD_EXEC_GRID_MAX ? n : ZSTD_EXEC_GRID_MAX);
    const bool maybe_zstd = holds.zstd != 0;                  // the host path knows its methods; device batches may hold any
    if (maybe_zstd && (rc = grow(c, c->wave.d_lit, (u64)(exec_grid > zstd_grid ? exec_grid : zstd_grid) * ZSTD_LIT_SCRATCH))) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_counters, 0, N_COUNTERS * sizeof(u32), st));
    ZPK_TRACE_STEP("memset");
#define ZPK_KEV(k, j) do { if (c->profiling) (void)hipEventRecord(c->kev[k][j], st); } while (0)
    ZPK_KEV(ZPK_K_CLASSIFY, 0);
    // (hash_only: k_classify's last guard — the slot lies inside dst, the bound of a CALLER'S layout in the device-resident call — is
    // switched off by its size: the slots are the codec's own layout of these very descriptors, and a stored entry has none)
    hipLaunchKernelGGL(k_classify, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, src, desc, n, src_size, hash_only ? ~0ull : dst_size, res,
                       c->wave.d_lists, stride, c->d_counters);
    // largest entries first (see k_order_count); batches that fit the resident waves in one round have nothing to order
    const u32* zstd_list = list_at(S_ZSTD);
    const u32* lz4_list = list_at(S_LZ4);
    int gen_slot = S_LZ4_GEN;                                   // the LZ4 entries that are not plain frames
    if (n >= c->opt.order_min) {
        const dim3 og((u32)((n + 255) / 256), N_ORDERED);
        hipLaunchKernelGGL(k_order_count, og, dim3(256), 0, st, desc, (const u32*)c->wave.d_lists, stride, c->d_counters, c->opt.order_fast_last);
        hipLaunchKernelGGL(k_order_fill, og, dim3(256), 0, st, desc, (const u32*)c->wave.d_lists, stride, c->wave.d_lists, c->d_counters, c->opt.order_fast_last);
        zstd_list = list_at(S_ZSTD_ORDERED); lz4_list = list_at(S_LZ4_ORDERED);
        gen_slot = S_LZ4_GEN_ORDERED;
    }
    const u32* const gen_list = list_at(gen_slot);
    ZPK_KEV(ZPK_K_CLASSIFY, 1);
    ZPK_TRACE_STEP("k_classify");
    const u32 wgrid = (u32)((n + 3) / 4);          // one wave per list slot
    ZPK_KEV(ZPK_K_STORED, 0);
    if (hash_only) { if (!(skip & 1)) stored_hash_launch(src, desc, res, list_at(S_NONE), c->d_counters, wgrid, st); }
    else if (!(skip & 1)) hipLaunchKernelGGL(k_stored, dim3(wgrid), dim3(256), 0, st, src, desc, dst, res, list_at(S_NONE), c->d_counters);
    ZPK_KEV(ZPK_K_STORED, 1);
    ZPK_TRACE_STEP("k_stored");
    // LZ4: one wave per work-list slot (lz4_wave.h).  A batch that may hold both methods runs the LZ4 kernels on a SIDE stream of
    // low priority, beside the Zstandard stages: those are bound by the latency of their serial chains and by LDS capacity (12 or
    // 16 workgroups per CU leave 3-8 KiB of LDS and most of the vector issue slots idle), so LZ4 waves fill what they leave.
    const bool maybe_lz4 = holds.lz4 != 0;
    hipStream_t sl = st;
    // (measured, 125 000 mixed entries: 112.0 -> 90.9 ms per batch, the LZ4 kernel's 25 ms disappear inside the Zstandard stages, which
    // get 1-3 ms longer; a pure LZ4 batch — the Zstandard kernels find empty lists — is unchanged within noise: 618.4 vs 618.2 GiB/s.)
    // A device batch does not say which methods it holds, and a pure Zstandard batch must NOT take the side stream: k_lz4_wave is one
    // workgroup per entry, and 100 000 EMPTY workgroups trickling through at low priority beside the pre-decode stage cost it 15 ms
    // (71.9 -> 87.6 ms).  So the codec looks at the work-list counts of the batch BEFORE (copied to pinned memory behind every batch,
    // no synchronisation): both methods there, or nothing known yet -> side stream; a codec fed batches of one method stays on one stream.
    if (!c->wave.h_seen && c->wave.h_seen.ready(64, hipHostMallocDefault)) {
        c->wave.h_seen->none = 0; c->wave.h_seen->zstd = 1; c->wave.h_seen->lz4 = 1; c->wave.h_seen->lz4_gen = 1; c->wave.h_seen->lz4_runs = 1;      // nothing known yet
    }
    const bool both_seen = holds.zstd >= 0 /* the host path knows */ || (c->wave.h_seen && c->wave.h_seen->zstd != 0 && (c->wave.h_seen->lz4 != 0 || c->wave.h_seen->lz4_gen != 0));
    if (maybe_lz4 && maybe_zstd && both_seen && !(skip & 6) && fork_stream(c->wave.side, st, true)) sl = c->wave.side.s;
    auto launch_lz4 = [&]() {
        if (c->profiling) (void)hipEventRecord(c->kev[ZPK_K_LZ4][0], sl);
        if (!(skip & 2) && maybe_lz4) {
            // The entries that are mostly runs (k_classify's second LZ4 list; none on text) by the build with the grouped cooperative copies,
            // BESIDE k_lz4_wave on a stream of its own: in front of it or behind it the few thousand of them were a serial stretch of one
            // entry's latency (0.4 ms of a 10 ms batch) with the chip nearly idle.
            hipStream_t sx = sl;
            // (a small batch is latency, not throughput: no second stream; neither when the batch BEFORE had no such entry — then the launch
            // is an empty grid in front of k_lz4_wave, and a batch that does have some pays the serial stretch once)
            if (n >= 4096 && c->wave.h_seen && c->wave.h_seen->lz4_runs != 0 && fork_stream(c->wave.left, sl, false)) sx = c->wave.left.s;
            hipLaunchKernelGGL(k_lz4_left, dim3((u32)(n < LZ4_LEFT_GRID_MAX ? n : LZ4_LEFT_GRID_MAX)), dim3(64), 0, sx, src, read_lo, read_hi, desc, dst, res,
                               (const u32*)left_lz4, c->d_counters, c->d_dbg, retry_lz4, wd_scale);
            // the hot kernel: plain frames only; whatever it does not finish cleanly is on its hand-over list
            bool lean = true;
#ifdef ZPK_DEVELOPER
            static const int all_general = getenv("ZPK_LZ4_GENERAL") ? atoi(getenv("ZPK_LZ4_GENERAL")) : 0;      // the general decoder alone (tests compare the two)
            lean = !all_general;
            if (!lean) hipLaunchKernelGGL(k_lz4_hand_all, dim3((u32)((n + 255) / 256)), dim3(256), 0, sl, lz4_list, c->d_counters, handed_lz4);
#endif
            if (lean) hipLaunchKernelGGL(k_lz4_wave, dim3((u32)n), dim3(64), 0, sl, src, read_hi, desc, dst, res,
                                         lz4_list, c->d_counters, retry_lz4, handed_lz4 ZPK_WD_ARG);
            // The entries that are not plain frames (k_classify's third LZ4 list): the general decoder at full width beside the two kernels
            // above — when the batch BEFORE had such entries, or nothing is known yet.  Otherwise the list is expected to be empty and
            // is left to k_lz4_retry below, so that archives of plain frames pay for no launch they do not need (a batch that does have
            // some then runs them on the small grid, once).
            if (!c->wave.h_seen || c->wave.h_seen->lz4_gen != 0)               // (the host-pointer paths do not bring the counts home: always launched there)
                hipLaunchKernelGGL(k_lz4_general, dim3((u32)(n < LZ4_GENERAL_GRID_MAX ? n : LZ4_GENERAL_GRID_MAX)), dim3(64), 0, sl, src, read_lo, read_hi,
                                   desc, dst, res, gen_list, c->d_counters, c->d_dbg, retry_lz4, wd_scale);
            if (sx != sl) join_stream(c->wave.left, sl);
            // whatever is left: k_lz4_general's list if that was not launched, what k_lz4_wave handed over, and the entries whose decoder
            // ran out of its time budget (ZPK_WATCHDOG_RETRY_SCALE times the budget; a small grid that leaves at once when the lists
            // are empty — the normal case)
            hipLaunchKernelGGL(k_lz4_retry, dim3((u32)(n < 256 ? n : 256)), dim3(64), 0, sl, src, read_lo, read_hi, desc, dst, res,
                               (const u32*)c->wave.d_lists, stride, c->d_counters, c->d_dbg, gen_slot);
        }
        if (c->profiling) (void)hipEventRecord(c->kev[ZPK_K_LZ4][1], sl);
    };
    if (sl == st) launch_lz4();                    // (side stream: enqueued BEHIND the Zstandard stages below, so that those are dispatched first)
    ZPK_TRACE_STEP("k_lz4_wave");
    // Zstandard in two stages: the FSE sequence streams four per wave into an arena laid out like dst (8 bytes per
    // sequence: room for one sequence per 8 output bytes; entries that need more stay with the fused decoder), then
    // literals + execution + checksum.  Without the arena (allocation refused) k_zstd does it all, and the codec says so
    // (zpk_codec_decode_stats out[7] bit 31, zpk_codec_last_error).
    bool two_stage = maybe_zstd && dst_size >= 64;
    ZPK_DEV(static const int fused_only = getenv("ZPK_ZSTD_FUSED") ? atoi(getenv("ZPK_ZSTD_FUSED")) : 0; if (fused_only) two_stage = false;)
    c->last.fell_back_fused = 0;
    if (two_stage && (grow(c, c->wave.d_zarena, dst_size + 64) != ZPK_OK ||
                      grow(c, c->wave.d_zstate, 2 * n * sizeof(u32)) != ZPK_OK)) {
        two_stage = false; c->last.fell_back_fused = 1;
        snprintf(c->err, sizeof(c->err), "note: no memory for the %llu-byte Zstandard sequence arena; this batch ran the fused decoder",
                 (unsigned long long)dst_size + 64);
    }
    u32* const leftover = two_stage ? c->wave.d_zstate + n : nullptr;          // entries k_zstd_exec hands to the full decoder
    ZPK_KEV(ZPK_K_ZSTD_FSE, 0);
    if (!(skip & 4) && two_stage) {
        HIPCHK(c, hipMemsetAsync(c->wave.d_zstate, 0, n * sizeof(u32), st));          // entries k_zstd_fse never reaches stay unmarked
        const u64 zwaves = (n + ZF_ROWS - 1) / ZF_ROWS;
        hipLaunchKernelGGL(k_zstd_fse, dim3((u32)(zwaves < ZF_GRID_MAX ? zwaves : ZF_GRID_MAX)), dim3(64), 0, st, src, desc,
                           zstd_list, c->d_counters, c->wave.d_zarena, c->wave.d_zstate);
    }
    ZPK_KEV(ZPK_K_ZSTD_FSE, 1);
    ZPK_TRACE_STEP("k_zstd_fse");
    ZPK_KEV(ZPK_K_ZSTD, 0);
    if (!(skip & 4) && two_stage)
        hipLaunchKernelGGL(k_zstd_exec, dim3(exec_grid), dim3(ZSTD_WG_THREADS), 0, st, src, desc, dst, res,
                           zstd_list, c->d_counters, c->wave.d_lit, c->wave.d_zarena, c->wave.d_zstate, leftover, c->d_dbg);
    if (!(skip & 4) && maybe_zstd)
        hipLaunchKernelGGL(k_zstd, dim3(zstd_grid), dim3(ZSTD_WG_THREADS), 0, st, src, desc, dst, res,
                       two_stage ? (const u32*)leftover : zstd_list, c->d_counters, c->wave.d_lit, c->d_dbg,
                       two_stage ? (int)C_ZSTD_LEFT : (int)C_ZSTD, (int)C_ZSTD_HEAD, retry_zstd, (int)C_RETRY_ZSTD, wd_scale);
    ZPK_KEV(ZPK_K_ZSTD, 1);
    ZPK_TRACE_STEP("k_zstd");
    // Entries whose decoder ran out of its time budget (a preempted or contended GPU, not the entry's fault) are decoded again
    // here, behind the stages of their method, with ZPK_WATCHDOG_RETRY_SCALE times the budget: small grids that leave at once
    // when their list is empty (the normal case).
    if (!(skip & 4) && maybe_zstd)
        hipLaunchKernelGGL(k_zstd, dim3(zstd_grid < 128 ? zstd_grid : 128), dim3(ZSTD_WG_THREADS), 0, st, src, desc, dst, res,
                           (const u32*)retry_zstd, c->d_counters, c->wave.d_lit, c->d_dbg, (int)C_RETRY_ZSTD, (int)C_ZSTD_RETRY_HEAD,
                           (u32*)nullptr, 0, (u32)ZPK_WATCHDOG_RETRY_SCALE);
    if (sl != st) {                                 // the LZ4 kernels, beside the above; the batch is done when both streams are
        launch_lz4();
        join_stream(c->wave.side, st);
    }
    ZPK_TRACE_STEP("retry");
    // what this batch held, for the next one: none / zstd / lz4 / lz4_gen (adjacent counter words: zpk_layout.h) in one copy; did it have LZ4 entries of runs?
    if (c->wave.h_seen && holds.zstd < 0) (void)hipMemcpyAsync((void*)&c->wave.h_seen->none, c->d_counters + C_NONE, 4 * sizeof(u32), hipMemcpyDeviceToHost, st);
    if (c->wave.h_seen) (void)hipMemcpyAsync((void*)&c->wave.h_seen->lz4_runs, c->d_counters + C_LZ4_RUNS, sizeof(u32), hipMemcpyDeviceToHost, st);
    HIPCHK(c, hipGetLastError());
    return ZPK_OK;
}

int zpk_codec_decode_batch_device(zpk_codec* c, const uint8_t* src, uint64_t src_size, const zpk_decode_desc* desc, uint64_t n,
                                  uint8_t* dst, uint64_t dst_size, zpk_decode_result* results, void* stream)
{
    if (!c || (n && (!desc || !results))) return ZPK_E_INVALID;
    CodecLock lk(c);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return decode_launch(c, BatchMethods{ -1, -1 }, src, src_size, src, src + src_size, desc, n, dst, dst_size, results, st);
}

// An entry whose frames end before uncomp_size bytes exist (a short decode is not an error of the libraries): lib/zpack_read.c:466
// hashes buffer[0, uncomp_size) all the same — the decoded bytes followed by whatever the CALLER'S buffer held.  The device slot holds
// something else there (an earlier batch's output), so for these rare entries the caller's bytes are brought up behind the decoded
// ones and the slot is hashed again: the verdict is the one the reference reaches on this caller's buffer.
// (Dst::Device: dst_ptrs are DEVICE pointers — zpk_codec_decode_batch_host_dptr — and the caller's bytes come over from there.
// Dst::None: there is no caller's buffer; the tail counts as ZEROS — the slot's tail is zeroed on the device, and the verdict is the one
// a read into a zero-filled buffer of uncomp_size bytes reaches.  An entry with a WINDOW, pl.windowed: likewise — the caller's buffer
// has window_bytes bytes and is no buffer of uncomp_size bytes, so the tail counts as zeros and the verdict is zpack_amd_test_files'.)
static int rehash_short_entries(zpk_codec* c, const zpk_decode_desc* hd, const zpk_decode_desc* desc, u64 n, uint8_t* const* dst_ptrs,
                                zpk_decode_result* results, Dst to = Dst::Host, const Planes& pl = Planes())
{
    for (u64 i = 0; i < n; i++) {
        zpk_decode_result& r = results[i];
        if (!host_short_decode(desc[i], r)) continue;
        int rc;
        if ((rc = grow(c, c->d_xpart, 64))) return rc;
        const u64 tail = desc[i].uncomp_size - r.produced;
        u64 meta[3] = { hd[i].dst_offset, desc[i].uncomp_size, 0 };
        if (to == Dst::None || pl.windowed(i)) HIPCHK(c, hipMemsetAsync(c->d_dst + hd[i].dst_offset + r.produced, 0, tail, c->stream));
        else HIPCHK(c, hipMemcpyAsync(c->d_dst + hd[i].dst_offset + r.produced, dst_ptrs[i] + r.produced, tail, to == Dst::Device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_xpart, meta, sizeof(meta), hipMemcpyHostToDevice, c->stream));
        u64* m = (u64*)c->d_xpart;
        hipLaunchKernelGGL(k_hash, dim3(1), dim3(64), 0, c->stream, (const u8*)c->d_dst, (const u64*)m, (const u64*)(m + 1), (u64)1, m + 2);
        u64 h = 0;
        HIPCHK(c, hipMemcpyAsync(&h, m + 2, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        r.hash = h;
        r.status = dec_hash_verdict(desc[i], h).status;
    }
    return ZPK_OK;
}

// One sub-batch of the host path: entries [0, n) of hd/desc, whose slots (hd[i].dst_offset, already laid out) total
// out_total bytes.  `image` is what gets staged: either the archive itself (span mode, src_offset = archive offsets,
// staged range [lo, hi)) or a packed copy of just these payloads (gather mode: hd[i].src_offset already rewritten).
// The pinned staging buffers are touched by copy engines and host threads only, never by kernels: non-coherent host memory
// (measured, tools/micro/pinned_copy.hip: H2D 47.8 vs 40.5 GB/s, D2H 55.9 vs 47.4 GB/s against the default, coherent kind)
#ifndef ZPK_PIN_FLAGS
#define ZPK_PIN_FLAGS hipHostMallocNonCoherent
#endif
static int pin_ready(zpk_codec* c)
{
    if (!c->pj.h_words.ready(64, hipHostMallocDefault)) return ZPK_E_NOMEM;
    if (!c->pipe.piece_counters.ready(64 * N_COUNTERS * sizeof(u32), hipHostMallocDefault)) return ZPK_E_NOMEM;
    for (int k = 0; k < 2; k++) {
        if (!c->pipe.h_pin[k].ready(ZPK_PIN_CHUNK, ZPK_PIN_FLAGS)) { snprintf(c->err, sizeof(c->err), "pinned staging: out of memory"); return ZPK_E_NOMEM; }
        if (c->pipe.pin_ev[k].ready(hipEventDisableTiming | hipEventReleaseToSystem) != hipSuccess) return ZPK_E_LAUNCH;
    }
    return ZPK_OK;
}

// One piece [p0, p1) of a staged range, moved between its pinned buffer and the buffers of those of the n entries that reach into it (entry
// i owns bytes [off(i), off(i) + len(i)) of the range, ascending in i; ei: the first that may, kept from piece to piece) by a few host
// threads.  Which entries reach into the piece, how many threads it gets and what each of them moves: host_plan.h (staged_reach,
// staged_threads, staged_share); move(i, in_entry, in_piece, bytes) copies, whichever way the caller goes.
extern "C++" {
template <class OffFn, class LenFn, class MoveFn>
static void staged_piece_copy(u64 p0, u64 p1, u64 n, u64& ei, OffFn off, LenFn len, MoveFn move)
{
    const u64 ej = staged_reach(p0, p1, n, ei, off, len);
    const unsigned T = staged_threads(p0, p1);
    auto share = [&](unsigned t) { staged_share_move(staged_share(p0, p1, ei, ej, t, T), p0, off, len, move); };
    // (a thread that cannot be started must not unwind through the C ABI: its share is copied inline instead)
    std::thread th[ZPK_SCATTER_THREADS - 1];
    bool started[ZPK_SCATTER_THREADS - 1] = {};
    for (unsigned t = 1; t < T; t++) {
        try { th[t - 1] = std::thread(share, t); started[t - 1] = true; }
        catch (...) { started[t - 1] = false; }
    }
    share(0);
    for (unsigned t = 1; t < T; t++) { if (started[t - 1]) th[t - 1].join(); else share(t); }
}

// Device range [d_base, d_base + total) back to the host in pieces of ZPK_PIN_CHUNK bytes through the two pinned buffers; piece j + 1 is
// on the bus while piece j is scattered: entry i owns bytes [off(i), off(i) + len(i)) of the range (ascending in i) and goes to dst_ptrs[i].
struct NoPre { hipError_t operator()(u64) const { return hipSuccess; } };
// pre(q1): called before bytes below q1 of the range are copied (the pipeline makes the download stream wait for their decode there)
template <class OffFn, class LenFn, class PreFn = NoPre>
static int d2h_scatter(zpk_codec* c, const u8* d_base, u64 total, u64 n, uint8_t* const* dst_ptrs, OffFn off, LenFn len, hipError_t& e,
                       hipStream_t st = nullptr, PreFn pre = PreFn())
{
    int rc = pin_ready(c);
    if (rc) return rc;
    if (total == 0) return ZPK_OK;
    if (!st) st = c->stream;
    const u64 npieces = staged_pieces(total);
    u64 ei = 0;                                                                       // first entry that may still reach into the current piece
    auto fetch = [&](u64 j) {                                                         // piece j sets out for its buffer
        const StagedPiece q = staged_piece(j, total);
        e = pre(q.p1);
        if (e == hipSuccess) e = hipMemcpyAsync(c->pipe.h_pin[j & 1], d_base + q.p0, q.p1 - q.p0, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipEventRecord(c->pipe.pin_ev[j & 1], st);
    };
    fetch(0);
    for (u64 j = 0; j < npieces && e == hipSuccess; j++) {
        const int k = (int)(j & 1);
        const StagedPiece p = staged_piece(j, total);
        if (j + 1 < npieces) { fetch(j + 1); if (e != hipSuccess) break; }
        e = hipEventSynchronize(c->pipe.pin_ev[k]);
        if (e != hipSuccess) break;
        staged_piece_copy(p.p0, p.p1, n, ei, off, len, [&](u64 i, u64 in_entry, u64 in_piece, u64 bytes) { memcpy(dst_ptrs[i] + in_entry, c->pipe.h_pin[k] + in_piece, bytes); });
    }
    return ZPK_OK;
}

// The other direction (round 3): entries that lie in the caller's (pageable, separate) buffers go up to the device range [d_base,
// d_base + total) in pieces of ZPK_PIN_CHUNK bytes through the two pinned buffers — piece j + 1 is gathered by a few host threads
// while piece j is on the bus.  Entry i owns bytes [off(i), off(i) + len(i)) of the range (ascending in i); the gaps between entries
// carry whatever the staging buffer held.  (One hipMemcpyAsync per entry out of pageable memory: 40 000 x 64 KiB took 0.5 s.)
template <class OffFn, class LenFn>
static int h2d_gather(zpk_codec* c, u8* d_base, u64 total, u64 n, const uint8_t* const* src_ptrs, OffFn off, LenFn len, hipError_t& e, hipStream_t st)
{
    int rc = pin_ready(c);
    if (rc) return rc;
    PinBlock<u8>* const pin = c->pipe.h_pin;
    Event* const evs = c->pipe.pin_ev;
    e = hipSuccess;
    if (total == 0) return ZPK_OK;
    const u64 npieces = staged_pieces(total);
    u64 ei = 0;
    bool used[2] = { false, false };
    for (u64 j = 0; j < npieces && e == hipSuccess; j++) {
        const int k = (int)(j & 1);
        const StagedPiece p = staged_piece(j, total);
        if (used[k]) { e = hipEventSynchronize(evs[k]); if (e != hipSuccess) break; }      // the buffer's previous piece has left
        staged_piece_copy(p.p0, p.p1, n, ei, off, len, [&](u64 i, u64 in_entry, u64 in_piece, u64 bytes) { memcpy(pin[k] + in_piece, src_ptrs[i] + in_entry, bytes); });
        e = hipMemcpyAsync(d_base + p.p0, pin[k], p.p1 - p.p0, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(evs[k], st);
        used[k] = true;
    }
    // the pinned buffers serve the download next: both uploads have to be off them
    for (int k = 0; k < 2 && e == hipSuccess; k++) if (used[k]) e = hipEventSynchronize(evs[k]);
    return ZPK_OK;
}

// The sources of a sub-batch into the staging c->d_src[0, in_total), entry i at off(i) with len(i) bytes (encode_batch_host_any, dsink_sub):
// DEVICE sources by ONE launch of k_span_copy (byte-plane entries: rows_enqueue), a single host source as it is, several gathered through the pinned buffers (h2d_gather).
// `e` as h2d_gather leaves it: the caller's table upload follows it and reports both.
template <class OffFn, class LenFn>
static int stage_sources(zpk_codec* c, const uint8_t* const* src_ptrs, bool dsrc, u64 n, OffFn off, LenFn len, u64 in_total, hipStream_t st, hipError_t& e,
                         const Planes& pl = Planes())
{
    e = hipSuccess;
    // (device sources with element sizes: those above 1 are SPLIT on the way, by ONE k_plane_copy — the staging holds the grouped bytes)
    if (dsrc) return rows_enqueue(c, n, [&](u64 i) { return zpk_span_copy{ (u64)src_ptrs[i], (u64)(c->d_src + off(i)), len(i) }; }, pl, PLANE_SPLIT, st);
    if (n == 1) { if (len(0)) e = hipMemcpyAsync(c->d_src, src_ptrs[0], len(0), hipMemcpyHostToDevice, st); return ZPK_OK; }
    return h2d_gather(c, c->d_src, in_total, n, src_ptrs, off, len, e, st);
}
}  // extern "C++"

// (the staged image is followed by ZPK_SRC_SLACK bytes of the codec's own, of which the kernels may read ZPK_SRC_READ_SLACK: host_plan.h)
static int deliver_slots(zpk_codec* c, const zpk_decode_desc* hd, const zpk_decode_desc* desc, u64 n, u64 out_total, uint8_t* const* dst_ptrs,
                         zpk_decode_result* results, Dst to, u64* home = nullptr, const Planes& pl = Planes());
static int decode_host_chunk(zpk_codec* c, const u8* image, u64 image_size, u64 lo, u64 hi, zpk_decode_desc* hd,
                             const zpk_decode_desc* desc, u64 n, u64 out_total, uint8_t* const* dst_ptrs, zpk_decode_result* results, BatchMethods holds, Dst to = Dst::Host,
                             const Planes& pl = Planes())
{
    int rc;
    if ((rc = grow(c, c->d_src, hi - lo + ZPK_SRC_SLACK)) || (rc = grow(c, c->d_dst, out_total + 16)) ||
        (rc = grow(c, c->d_desc, n * sizeof(zpk_decode_desc))) ||
        (rc = grow(c, c->d_res, n * sizeof(zpk_decode_result)))) return rc;
    hipError_t e = hipSuccess;
    if (hi > lo) e = hipMemcpyAsync(c->d_src, image + lo, hi - lo, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->d_desc, hd, n * sizeof(zpk_decode_desc), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "H2D: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    // base pointer such that base + src_offset lands in the staged range; reads are clamped to it
    const u8* base = c->d_src - lo;
    rc = decode_launch(c, holds, base, image_size, c->d_src, c->d_src + (hi - lo) + ZPK_SRC_READ_SLACK, (const zpk_decode_desc*)c->d_desc, n,
                       c->d_dst, out_total, (zpk_decode_result*)c->d_res, c->stream, to == Dst::None);
    if (rc) return rc;
    e = hipMemcpyAsync(results, c->d_res, n * sizeof(zpk_decode_result), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "decode: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    return deliver_slots(c, hd, desc, n, out_total, dst_ptrs, results, to, nullptr, pl);
}

// The slots of a decoded sub-batch, c->d_dst + hd[i].dst_offset, handed to the caller (decode_host_chunk; zpk_codec_decode_batch_dimage):
// everything the codec produced (a hash mismatch leaves the data in the buffer, like the reference), and only that — a generous
// max_size costs device address space, not PCIe time.  results[0, n) are home and the decode has completed.  *home: the bytes that
// crossed the bus for it.  Dst::None: nothing is handed over — no copy, no k_span_copy; only the short decodes are looked at.
static int deliver_slots(zpk_codec* c, const zpk_decode_desc* hd, const zpk_decode_desc* desc, u64 n, u64 out_total, uint8_t* const* dst_ptrs,
                         zpk_decode_result* results, Dst to, u64* home, const Planes& pl)
{
    int rc;
    hipError_t e = hipSuccess;
    u64 produced_total = 0;
    if (home) *home = 0;
    for (u64 i = 0; i < n; i++) {
        results[i].produced = host_delivered(desc[i], results[i]);
        produced_total += results[i].produced;
    }
    if (to == Dst::None) return rehash_short_entries(c, hd, desc, n, dst_ptrs, results, to);
    if (to == Dst::Device) {
        // DEVICE destinations: the same bytes — [slot, slot + produced) of every entry — by ONE launch of k_span_copy, no host in between
        // (an entry with an element size above 1 is JOINED on the way, all of it or none: planes_join_len)
        auto row = [&](u64 i) { return zpk_span_copy{ (u64)(c->d_dst + hd[i].dst_offset), (u64)dst_ptrs[i], pl.grouped(i) ? pl.join_len(i, desc[i], results[i]) : (u64)results[i].produced }; };
        if ((rc = rows_enqueue(c, n, row, pl, PLANE_JOIN, c->stream))) return rc;
        e = hipStreamSynchronize(c->stream);
    } else if (host_deliver_dense(n, produced_total, out_total)) {
        // dense: the slots come back in pieces of ZPK_PIN_CHUNK bytes through two PINNED staging buffers — piece j + 1 is on the bus
        // while piece j is scattered into the caller's (pageable) buffers.  (One hipMemcpy of everything into a fresh malloc, then
        // the scatter, ran at 6.7 GB/s: page faults + the driver's own staging of pageable memory.)
        rc = d2h_scatter(c, c->d_dst, out_total, n, dst_ptrs, [&](u64 i) { return (u64)hd[i].dst_offset; }, [&](u64 i) { return (u64)results[i].produced; }, e);
        if (rc) return rc;
        if (home) *home = out_total;
        sat_add(c->last.home, out_total);
    } else {
        for (u64 i = 0; i < n && e == hipSuccess; i++)
            if (results[i].produced) e = hipMemcpy(dst_ptrs[i], c->d_dst + hd[i].dst_offset, results[i].produced, hipMemcpyDeviceToHost);
        if (home) *home = produced_total;
        sat_add(c->last.home, produced_total);
    }
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "D2H: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    return rehash_short_entries(c, hd, desc, n, dst_ptrs, results, to, pl);
}

// ---- the same chunk as a three-stage pipeline (round 3) ------------------------------------------------------------------------
// decode_host_chunk runs upload -> decode -> download one after the other: 0.71 GB up, 2 ms of kernels and 1.31 GB down took 40 ms
// for 20 000 x 64 KiB LZ4 entries, i.e. 30 GiB/s of decoded bytes where the bus alone allows ~47 (PCIe is full duplex).  Here the
// chunk is cut into pieces (host_pieces, host_plan.h): an UPLOADER thread sends the compressed span of piece after piece (pageable memory, its own
// stream), a LAUNCHER thread starts the decode of piece k as soon as its upload has been enqueued (the codec's stream waits for
// the upload's event), and this thread brings the output range back as ONE continuous double-buffered stream through the pinned
// buffers (download stream; before a range is copied that stream is told to wait for the decode of the pieces it covers) and
// scatters it.  Entries must lie in the archive roughly in batch order (each piece uploads the span of its own entries);
// anything else, or a chunk too small to be worth it, takes decode_host_chunk.
// A stage's progress: pieces ENQUEUED with their event recorded, -1 = the stage failed.  -> once it is past piece k: true; failed: false
static bool stage_past(const std::atomic<int>& done, int k)
{
    int v;
    while ((v = done.load()) >= 0 && v <= k) std::this_thread::yield();
    return v >= 0;
}

static int decode_host_pipelined(zpk_codec* c, const u8* image, u64 image_size, u64 lo, u64 hi, zpk_decode_desc* hd,
                                 const zpk_decode_desc* desc, u64 n, u64 out_total, uint8_t* const* dst_ptrs, zpk_decode_result* results,
                                 bool& taken, BatchMethods holds, Dst to = Dst::Host, const Planes& pl = Planes())
{
    // Dst::None: stage 1 (the upload) still runs beside stage 2 (the decode); there is no stage 3 — no download stream, no `decoded`
    // events — and the verdicts come home in one copy behind the last piece
    const bool ddst = to == Dst::Device, none = to == Dst::None;
    taken = false;
    HostPiece pc[ZPK_HOST_MAX_PIECES];
    const int np = host_pieces(hd, n, image_size, lo, hi, out_total, host_pipe_min_entries(holds.zstd != 0), pc);
    if (np == 0) return ZPK_OK;
    int rc;
    if ((rc = grow(c, c->d_src, hi - lo + ZPK_SRC_SLACK)) || (rc = grow(c, c->d_dst, out_total + 16)) ||
        (rc = grow(c, c->d_desc, n * sizeof(zpk_decode_desc))) ||
        (rc = grow(c, c->d_res, n * sizeof(zpk_decode_result))) || (rc = pin_ready(c))) return rc;
    if (c->pipe.s_up.ready(hipStreamNonBlocking) != hipSuccess || (!none && c->pipe.s_dn.ready(hipStreamNonBlocking) != hipSuccess)) return ZPK_OK;
    for (int k = 0; k < 2 * np; k++)
        if (!(none && (k & 1)) && c->pipe.ev[k].ready(hipEventDisableTiming | hipEventReleaseToSystem) != hipSuccess) return ZPK_OK;
    taken = true;
    c->last.pipe++;
    hipError_t e = hipMemcpyAsync(c->d_desc, hd, n * sizeof(zpk_decode_desc), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "H2D: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    std::atomic<int> uploaded(0), launched(0);   // pieces whose upload / decode has been ENQUEUED with its event recorded (-1: failed)
    std::atomic<int> launch_rc(ZPK_OK);
    const int device = c->device;
    const u8* base = c->d_src - lo;
    auto uploader = [&]() {
        if (hipSetDevice(device) != hipSuccess) { uploaded.store(-1); return; }
        for (int k = 0; k < np; k++) {
            hipError_t ue = hipSuccess;
            if (pc[k].chi > pc[k].clo) ue = hipMemcpyAsync(c->d_src + (pc[k].clo - lo), image + pc[k].clo, pc[k].chi - pc[k].clo, hipMemcpyHostToDevice, c->pipe.s_up);
            if (ue == hipSuccess) ue = hipEventRecord(c->pipe.ev[2 * k], c->pipe.s_up);
            if (ue != hipSuccess) { uploaded.store(-1); return; }
            uploaded.store(k + 1);
        }
    };
    auto launcher = [&]() {
        if (hipSetDevice(device) != hipSuccess) { launch_rc.store(ZPK_E_LAUNCH); launched.store(-1); return; }
        for (int k = 0; k < np; k++) {
            int lrc = stage_past(uploaded, k) ? (int)ZPK_OK : (int)ZPK_E_LAUNCH;
            if (lrc == ZPK_OK && hipStreamWaitEvent(c->stream, c->pipe.ev[2 * k], 0) != hipSuccess) lrc = ZPK_E_LAUNCH;
            const HostPiece& P = pc[k];
            if (lrc == ZPK_OK)
                lrc = decode_launch(c, holds, base, image_size, c->d_src + (P.clo - lo), c->d_src + (P.chi - lo) + ZPK_SRC_READ_SLACK, (const zpk_decode_desc*)c->d_desc + P.e0,
                                    P.e1 - P.e0, c->d_dst, out_total, (zpk_decode_result*)c->d_res + P.e0, c->stream, none);
            if (lrc == ZPK_OK && hipMemcpyAsync(c->pipe.piece_counters[k], c->d_counters, N_COUNTERS * sizeof(u32), hipMemcpyDeviceToHost, c->stream) != hipSuccess) lrc = ZPK_E_LAUNCH;
            if (lrc == ZPK_OK && !none && hipEventRecord(c->pipe.ev[2 * k + 1], c->stream) != hipSuccess) lrc = ZPK_E_LAUNCH;
            if (lrc != ZPK_OK) { launch_rc.store(lrc); launched.store(-1); return; }
            launched.store(k + 1);
        }
    };
    // (a thread that cannot be started must not unwind through the C ABI: its stage then runs here, in order — still correct, no overlap)
    std::thread t_up, t_launch;
    bool up_threaded = true, launch_threaded = true;
    try { t_up = std::thread(uploader); } catch (...) { up_threaded = false; }
    if (!up_threaded) uploader();
    try { t_launch = std::thread(launcher); } catch (...) { launch_threaded = false; }
    if (!launch_threaded) launcher();
    // ---- download: one continuous stream over the chunk's output range ----
    // the results of piece k come home on the download stream, once its decode has been enqueued and behind it
    auto results_home = [&](int k) -> hipError_t {
        if (!stage_past(launched, k)) return hipErrorUnknown;
        const HostPiece& P = pc[k];
        hipError_t pe = hipStreamWaitEvent(c->pipe.s_dn, c->pipe.ev[2 * k + 1], 0);
        if (pe == hipSuccess) pe = hipMemcpyAsync(results + P.e0, (const zpk_decode_result*)c->d_res + P.e0, (P.e1 - P.e0) * sizeof(zpk_decode_result), hipMemcpyDeviceToHost, c->pipe.s_dn);
        return pe;
    };
    int next = 0;                                // first piece the download stream has not been told to wait for
    auto pre = [&](u64 q1) -> hipError_t {       // (the results in stream order before the bytes: there when they are scattered)
        for (; next < np && pc[next].olo < q1; next++) { const hipError_t pe = results_home(next); if (pe != hipSuccess) return pe; }
        return hipSuccess;
    };
    if (none) {
        // no destination: nothing comes home while the pieces run; the verdicts follow the last piece, below
    } else if (ddst) {
        // DEVICE destinations (zpk_codec_decode_batch_host_dptr): there is no download.  Piece by piece, as soon as its decode has run: the
        // verdicts come home and ONE k_span_copy on the download stream moves the piece's slots to their pointers — [slot, slot + produced),
        // the bytes the scatter below copies — while the upload and the decode of the pieces behind it go on.
        for (int k = 0; k < np && rc == ZPK_OK && e == hipSuccess; k++) {
            const HostPiece& P = pc[k];
            e = results_home(k);
            if (e == hipSuccess) e = hipStreamSynchronize(c->pipe.s_dn);
            if (e != hipSuccess) break;
            rc = rows_enqueue(c, P.e1 - P.e0, [&](u64 k2) {
                const u64 i = P.e0 + k2;
                return zpk_span_copy{ (u64)(c->d_dst + hd[i].dst_offset), (u64)dst_ptrs[i], pl.grouped(i) ? pl.join_len(i, desc[i], results[i]) : host_delivered(desc[i], results[i]) };
            }, pl.from(P.e0), PLANE_JOIN, c->pipe.s_dn);
        }
    } else
    rc = d2h_scatter(c, c->d_dst, out_total, n, dst_ptrs, [&](u64 i) { return (u64)hd[i].dst_offset; }, [&](u64 i) { return host_delivered(desc[i], results[i]); }, e, c->pipe.s_dn, pre);
    if (!ddst && !none && rc == ZPK_OK) sat_add(c->last.home, out_total);
    if (up_threaded) t_up.join();
    if (launch_threaded) t_launch.join();
    if (none && launch_rc.load() == ZPK_OK) {                                   // every piece is enqueued: the verdicts, behind the last one
        e = hipMemcpyAsync(results, c->d_res, n * sizeof(zpk_decode_result), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    if (!ddst && !none && rc == ZPK_OK && e == hipSuccess) e = pre(out_total + 1);       // (pieces with no output bytes: their results still come back)
    if (!none && rc == ZPK_OK && e == hipSuccess) e = hipStreamSynchronize(c->pipe.s_dn);
    if (launch_rc.load() != ZPK_OK) rc = launch_rc.load();
    else if (rc == ZPK_OK && e != hipSuccess) { snprintf(c->err, sizeof(c->err), "host decode pipeline: %s", hipGetErrorString(e)); rc = ZPK_E_LAUNCH; }
    if (rc != ZPK_OK) { (void)hipStreamSynchronize(c->pipe.s_up); (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->pipe.s_dn); }
    for (u64 i = 0; i < n && rc == ZPK_OK; i++) results[i].produced = host_delivered(desc[i], results[i]);
    if (rc == ZPK_OK && hipStreamSynchronize(c->stream) == hipSuccess) {
        memset(c->last.host_totals, 0, sizeof(c->last.host_totals));
        for (int k = 0; k < np; k++) for (int w = 0; w < N_COUNTERS; w++) c->last.host_totals[w] += c->pipe.piece_counters[k][w];
        c->last.totals_valid = 1;
    }
    if (rc == ZPK_OK) rc = rehash_short_entries(c, hd, desc, n, dst_ptrs, results, to, pl);
    return rc;
}

// ---- entries that are SEQUENCES OF FRAMES, decoded frame-parallel (host path): host_walk.h finds the frames (walk_lz4_frames, walk_zstd_frames) ----
// (struct BigEntry, the cut of such entries into groups and the staging of a group: host_plan.h)

// The common second half of the block-parallel readers (lz4_pj.h, zstd_pj.h): the blocks' references exist per chunk through `init`, the
// block table `hb` (output offsets) is on the host.  Chunks of ZPK_PJ_CHUNK_BLOCKS blocks are resolved one after the other, hashed and
// downloaded beside that.  accept_mismatch: a wrong XXH3 is this path's verdict (LZ4: everything about the frame was checked); otherwise
// the one-wave decoder decides.
extern "C++" {
template <class InitFn>
static int pj_finish(zpk_codec* c, const zpk_decode_desc& d, const std::vector<PjBlock>& hb, u64 chunk_blocks, u64 gather_src_size, InitFn init, bool accept_mismatch,
                     u8* d_out, uint8_t* dst_ptr, zpk_decode_result& result, u8& redo)
{
    const u64 nb = hb.size(), n = d.uncomp_size;
    hipStream_t st = c->stream;
    PjBlock* const B = (PjBlock*)c->pj.d_blocks;
    u32* const S = (u32*)c->pj.d_S;
    hipError_t e;
    int rc;
    if (chunk_blocks * ZPK_PJ_MAX_CHUNKS < nb) chunk_blocks = (nb + ZPK_PJ_MAX_CHUNKS - 1) / ZPK_PJ_MAX_CHUNKS;      // (small blocks, a very large entry: larger chunks)
    const u64 nchunks = (nb + chunk_blocks - 1) / chunk_blocks;
    if (nchunks > ZPK_PJ_MAX_CHUNKS) return ZPK_OK;
    for (u64 k = 0; k < nchunks; k++) if (c->pj.ev[k].ready(hipEventDisableTiming) != hipSuccess) return ZPK_OK;
    if (dst_ptr && c->pipe.s_dn.ready(hipStreamNonBlocking) != hipSuccess) return ZPK_OK;    // (no host destination: no download, no stream for one)
    if ((rc = pin_ready(c))) return rc;
    // the XXH3 of the output runs BESIDE all this on its own stream, section by section as the chunks become final (xxh3_span.h: the
    // partial sums of a section's blocks side by side, then the one-wave chain over them — 14 ms for 256 MiB, as long as everything else
    // together, which is why it must not come behind)
    if (c->wave.left.s.ready(hipStreamNonBlocking) != hipSuccess) return ZPK_OK;
    hipStream_t sh = c->wave.left.s;
    const u64 part_blocks = xxh3_span_blocks(n), ngroups = part_blocks / XS_GROUP;
    if ((rc = grow(c, c->d_xpart, 256 + part_blocks * 64 + 256))) return rc;
    zpk_span* const d_span = (zpk_span*)c->d_xpart;
    u64* const d_part = (u64*)(c->d_xpart + 256);
    u64* const d_hash = (u64*)(c->d_xpart + 256 + part_blocks * 64);
    u64* const d_state = d_hash + 8;
    zpk_span span; span.off = 0; span.len = n; span.part_base = 0;
    e = hipMemcpyAsync(d_span, &span, sizeof(span), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "large frame: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    // ---- the output to the caller's buffer starts while the chunks are still being resolved: d2h_scatter (pinned staging, the copy of piece
    // j + 1 on the bus while piece j is copied out by a few threads) runs on a helper thread and takes a piece as soon as the chunks under it
    // have been ENQUEUED (their events recorded).  The bytes are the entry's whatever the verdict (lib/zpack_read.c:466-468 leaves
    // them); if the path turns out not to have been regular the one-wave decoder overwrites them. ----
    std::vector<u64> chunk_hi(nchunks);
    for (u64 k = 0; k < nchunks; k++) { const u64 b1 = (k + 1) * chunk_blocks; chunk_hi[k] = b1 < nb ? hb[b1].out_off : n; }
    std::atomic<u64> enqueued{0};
    std::atomic<int> give_up{0};
    int dn_rc = ZPK_OK; hipError_t dn_e = hipSuccess;
    auto download = [&]() {
        (void)hipSetDevice(c->device);
        u64 waited = 0;
        auto pre = [&](u64 q1) -> hipError_t {
            while (waited < nchunks && (waited == 0 || chunk_hi[waited - 1] < q1)) {
                while (enqueued.load(std::memory_order_acquire) <= waited) { if (give_up.load(std::memory_order_acquire)) return hipErrorUnknown; std::this_thread::yield(); }
                const hipError_t we = hipStreamWaitEvent(c->pipe.s_dn, c->pj.ev[waited], 0);
                if (we != hipSuccess) return we;
                waited++;
            }
            return hipSuccess;
        };
        uint8_t* optr[1] = { dst_ptr };
        dn_rc = d2h_scatter(c, d_out, n, 1, optr, [&](u64) { return (u64)0; }, [&](u64) { return n; }, dn_e, c->pipe.s_dn, pre);
    };
    std::thread dn_thread;
    bool dn_started = false;
    if (dst_ptr) { try { dn_thread = std::thread(download); dn_started = true; } catch (...) { dn_started = false; } }      // (no thread: the download follows the loop; no host destination: the output stays where it is)
    // ---- every chunk: references, PJ_MAX_ROUNDS rounds of pointer doubling (a round behind the last one that changed anything returns at
    // once: no host round trip), the gather; an event behind each chunk lets its bytes be hashed and go home while the next is resolved ----
    bool launch_failed = false;
    const bool short_hash = n <= 240;
    u64 g_lo = 0;
    for (u64 k = 0; k < nchunks; k++) {
        const u32 b0 = (u32)(k * chunk_blocks), b1 = (u32)(b0 + chunk_blocks < nb ? b0 + chunk_blocks : nb);
        const u64 lo = hb[b0].out_off, hi = chunk_hi[k];
        const u32 grid = (u32)((hi - (lo & ~3ull) + 1023) / 1024), jgrid = (u32)((hi - lo + 1023) / 1024);
        (void)hipMemsetAsync(c->pj.d_flags + PJ_ROUND0, 0, PJ_MAX_ROUNDS * 4, st);
        init(b0, b1, st);
        if (grid) {
            for (u32 r = 0; r < PJ_MAX_ROUNDS; r++)
                hipLaunchKernelGGL(k_pj_jump, dim3(jgrid), dim3(256), 0, st, S, (const PjBlock*)B, b0, b1, (u32)nb, c->pj.d_flags, r);
            hipLaunchKernelGGL(k_pj_gather, dim3(grid), dim3(256), 0, st, (const u32*)S, (const PjBlock*)B, b0, b1, (u32)nb, (const u8*)c->d_src, gather_src_size, d_out, c->pj.d_flags);
        }
        if (hipEventRecord(c->pj.ev[k], st) != hipSuccess || hipStreamWaitEvent(sh, c->pj.ev[k], 0) != hipSuccess) { launch_failed = true; break; }
        enqueued.store(k + 1, std::memory_order_release);
        const bool last = k + 1 == nchunks;
        const u64 g_hi = last ? ngroups : (hi >> 10) / XS_GROUP;                       // groups of 64 blocks that are final now
        // (an output of at most 240 bytes: XXH3's short-input forms, not the chain — its tail reads the stripe at end - 64 and ends in the
        // avalanche of the long form.  One wave of k_hash behind the last chunk, the span's own off / len words as its one-row table)
        if (short_hash) { if (last) hipLaunchKernelGGL(k_hash, dim3(1), dim3(64), 0, sh, (const u8*)d_out, (const u64*)&d_span->off, (const u64*)&d_span->len, (u64)1, d_hash); continue; }
        if (g_hi > g_lo) hipLaunchKernelGGL(k_xxh3_partials, dim3((u32)((g_hi - g_lo + 3) / 4)), dim3(256), 0, sh, (const u8*)d_out, (const zpk_span*)d_span, 1u, g_lo, g_hi, d_part);
        if (g_hi > g_lo || last)
            hipLaunchKernelGGL(k_xxh3_chain, dim3(1), dim3(64), 0, sh, (const u8*)d_out, (const zpk_span*)d_span, (const u64*)d_part, d_hash, d_state, g_lo * XS_GROUP, g_hi * XS_GROUP, last ? 1 : 0);
        if (g_hi > g_lo) g_lo = g_hi;
    }
    if (launch_failed) give_up.store(1, std::memory_order_release);
    e = launch_failed ? hipErrorUnknown : hipMemcpyAsync(&c->pj.h_words[0], d_hash, 8, hipMemcpyDeviceToHost, sh);
    if (e == hipSuccess) e = hipMemcpyAsync(&c->pj.h_words[1], c->pj.d_flags, 4, hipMemcpyDeviceToHost, sh);
    if (dn_started) dn_thread.join(); else if (!launch_failed && dst_ptr) download();
    if (e != hipSuccess || dn_rc != ZPK_OK || dn_e != hipSuccess) {
        (void)hipDeviceSynchronize();
        if (dn_rc != ZPK_OK && !launch_failed) return dn_rc;
        snprintf(c->err, sizeof(c->err), "large frame: %s", hipGetErrorString(e != hipSuccess ? e : dn_e));
        return ZPK_E_LAUNCH;
    }
    e = dst_ptr ? hipStreamSynchronize(c->pipe.s_dn) : hipSuccess;
    const hipError_t e2 = hipStreamSynchronize(sh), e3 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2 != hipSuccess ? e2 : e3;
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "large frame: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    if (dst_ptr) sat_add(c->last.home, n);
    if ((u32)c->pj.h_words[1] != 0) return ZPK_OK;                                                      // PJ_ERR: something was irregular after all
    const zpk_decode_result v = dec_hash_verdict(d, c->pj.h_words[0]);
    if (v.status != DEC_R_OK && !accept_mismatch) return ZPK_OK;                                   // (the one-wave decoder gives this entry's verdict)
    result = v;
    c->last.big[0]++; c->last.big[1] += (u32)nb;
    redo = 0;
    return ZPK_OK;
}

}   // extern "C++"

// The two ends of a block-parallel entry: the archive its bytes are read from (archive + src_offset) and where ITS output goes, each
// either host or device memory.  Output on the device stays where it is written; a host destination gets it through c->d_dst.
struct BigSrc { const u8* archive; bool on_device; };
struct BigDst {                                                                      // to = Dst::None: p is not looked at, the output stays in c->d_dst and only its XXH3 is asked for
    u8* p; Dst to;
    bool staged() const { return to != Dst::Device; }                                // decoded into c->d_dst (from where a host destination gets it)
    u8* host() const { return to == Dst::Host ? p : nullptr; }
};

// -> ZPK_OK with redo = 0: the entry is decoded, hashed and delivered; redo = 1: not this path's (the one-wave decoder decides)
static int decode_big_lz4_single(zpk_codec* c, const BigSrc& src, const zpk_decode_desc& d, const std::vector<PjBlock>& blocks, int independent,
                                 const BigDst& dst, zpk_decode_result& result, u8& redo)
{
    redo = 1;
    const u64 nb = blocks.size(), n = d.uncomp_size;
    const u64 total_recs = (u64)blocks.back().rec_base + ((blocks.back().comp_size >> 31) ? 0 : (blocks.back().comp_size / 3 + 2));
    int rc;
    if ((rc = grow(c, c->d_src, d.comp_size + ZPK_SRC_SLACK)) || (dst.staged() && (rc = grow(c, c->d_dst, n + 16))) ||
        (rc = grow(c, c->pj.d_blocks, nb * sizeof(PjBlock))) || (rc = grow(c, c->pj.d_recs, (total_recs + 64) * 8)) ||
        (rc = grow(c, c->pj.d_masks, nb * (PJ_BLOCK / 8))) || (rc = grow(c, c->pj.d_S, n * 4 + 64))) { c->err[0] = 0; return ZPK_OK; }     // no memory for the scratch: the one-wave decoder
    if (!c->pj.d_flags.ensure(256)) return ZPK_OK;
    hipStream_t st = c->stream;
    hipError_t e = hipMemcpyAsync(c->d_src, src.archive + d.src_offset, d.comp_size, src.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(c->pj.d_blocks, blocks.data(), nb * sizeof(PjBlock), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(c->pj.d_flags, 0, 256, st);
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "H2D: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    PjBlock* const B = (PjBlock*)c->pj.d_blocks;
    u32* const S = (u32*)c->pj.d_S;
    hipLaunchKernelGGL(k_pj_parse, dim3((u32)nb), dim3(64), 0, st, (const u8*)c->d_src, d.comp_size, B, (u32)nb, (u64*)c->pj.d_recs, (u32*)c->pj.d_masks, c->pj.d_flags);
    hipLaunchKernelGGL(k_pj_scan, dim3(1), dim3(64), 0, st, B, (u32)nb, c->pj.d_flags);
    u32 hf[4] = {0, 0, 0, 0};
    // the verdict of the parse and the block table with its output offsets, back on the host (the one round trip of this path):
    // chunk k = blocks [k * ZPK_PJ_CHUNK_BLOCKS, ...) = output bytes [lo_k, hi_k)
    std::vector<PjBlock> hb(nb);
    e = hipMemcpyAsync(hf, c->pj.d_flags, sizeof(hf), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(hb.data(), B, nb * sizeof(PjBlock), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "large LZ4 frame: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    if (hf[PJ_ERR] || (((u64)hf[PJ_TOTAL + 1] << 32) | hf[PJ_TOTAL]) != n) return ZPK_OK;          // irregular, or the sizes do not add up
    auto init = [&](u32 b0, u32 b1, hipStream_t s2) {
        hipLaunchKernelGGL(k_pj_init, dim3(b1 - b0), dim3(256), 0, s2, (const PjBlock*)B, b0, (u32)nb, (const u64*)c->pj.d_recs, (const u32*)c->pj.d_masks, S, n, c->pj.d_flags, independent);
    };
    return pj_finish(c, d, hb, ZPK_PJ_CHUNK_BLOCKS, d.comp_size, init, true, dst.staged() ? (u8*)c->d_dst : dst.p, dst.host(), result, redo);
}

// -> ZPK_OK with redo = 0: the entry is decoded, its XXH3 is the expected one, the bytes are delivered; redo = 1: not this path's
static int decode_big_zstd_single(zpk_codec* c, const BigSrc& src, const zpk_decode_desc& d, std::vector<ZpjBlock>& blocks, u64 slots, u64 lit_total,
                                  const BigDst& dst, zpk_decode_result& result, u8& redo)
{
    redo = 1;
    const u64 nb = blocks.size(), n = d.uncomp_size;
    const u64 arena_off = (d.comp_size + 64 + 255) & ~255ull;
    for (u64 b = 0; b < nb; b++) if (blocks[b].type == 2 && blocks[b].lit_type >= 2) blocks[b].lit_ref = (u32)(arena_off + blocks[b].lit_base);
    // work items of the sequence stage: the compressed blocks that have sequences
    std::vector<zpk_decode_desc> items(nb);
    std::vector<u32> list;
    memset(items.data(), 0, nb * sizeof(zpk_decode_desc));
    for (u64 b = 0; b < nb; b++) {
        if (blocks[b].type != 2 || blocks[b].nseq == 0) continue;
        items[b].src_offset = blocks[b].hdr_off; items[b].comp_size = 3ull + blocks[b].size;
        items[b].dst_offset = 8ull * blocks[b].seq_base; items[b].dst_capacity = 8ull * blocks[b].nseq; items[b].method = ZPK_METHOD_ZSTD;
        items[b].uncomp_size = (u64)blocks[b].tab_off[0] | ((u64)blocks[b].tab_off[1] << 32);         // (k_zstd_fse_blocks: inherited table descriptions)
        items[b].expect_hash = (u64)blocks[b].tab_off[2] | ((u64)blocks[b].tab_modes << 32);
        list.push_back((u32)b);
    }
    const u64 aux_desc = 0, aux_list = (nb * sizeof(zpk_decode_desc) + 255) & ~255ull, aux_state = aux_list + ((nb * 4 + 255) & ~255ull),
              aux_rep = aux_state + ((nb * 4 + 255) & ~255ull), aux_size = aux_rep + nb * 12 + 256;
    int rc;
    if ((rc = grow(c, c->d_src, arena_off + lit_total + ZPK_SRC_SLACK)) || (dst.staged() && (rc = grow(c, c->d_dst, n + 16))) ||
        (rc = grow(c, c->pj.d_blocks, nb * sizeof(PjBlock))) || (rc = grow(c, c->pj.d_zblocks, nb * sizeof(ZpjBlock))) ||
        (rc = grow(c, c->pj.d_zaux, aux_size)) || (rc = grow(c, c->pj.d_recs, (slots + 64) * 8)) ||
        (rc = grow(c, c->pj.d_zpos, (slots + 64) * 8)) || (rc = grow(c, c->pj.d_masks, nb * (ZPJ_BLOCK / 8))) ||
        (rc = grow(c, c->pj.d_S, n * 4 + 64))) { c->err[0] = 0; return ZPK_OK; }        // no memory for the scratch: the one-wave decoder
    if (!c->pj.d_flags.ensure(256)) return ZPK_OK;
    hipStream_t st = c->stream;
    u8* const aux = (u8*)c->pj.d_zaux;
    u32 hflags[ZPJ_FLAG_WORDS]; memset(hflags, 0, sizeof(hflags));
    hflags[ZPJ_CNT + C_ZSTD] = (u32)list.size();
    std::vector<PjBlock> hb(nb);
    memset(hb.data(), 0, nb * sizeof(PjBlock));
    hipError_t e = hipMemcpyAsync(c->d_src, src.archive + d.src_offset, d.comp_size, src.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(c->pj.d_zblocks, blocks.data(), nb * sizeof(ZpjBlock), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(c->pj.d_blocks, hb.data(), nb * sizeof(PjBlock), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(aux + aux_desc, items.data(), nb * sizeof(zpk_decode_desc), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && !list.empty()) e = hipMemcpyAsync(aux + aux_list, list.data(), list.size() * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(aux + aux_state, 0, aux_size - aux_state, st);
    if (e == hipSuccess) e = hipMemcpyAsync(c->pj.d_flags, hflags, sizeof(hflags), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "H2D: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    PjBlock* const B = (PjBlock*)c->pj.d_blocks;
    ZpjBlock* const ZB = (ZpjBlock*)c->pj.d_zblocks;
    u32* const S = (u32*)c->pj.d_S;
    u32* const state = (u32*)(aux + aux_state);
    u32* const rep_out = (u32*)(aux + aux_rep);
    if (!list.empty()) {
        const u32 rows = (u32)list.size();
        const u32 grid = (rows + ZF_ROWS - 1) / ZF_ROWS < ZF_GRID_MAX ? (rows + ZF_ROWS - 1) / ZF_ROWS : ZF_GRID_MAX;
        hipLaunchKernelGGL(k_zstd_fse_blocks, dim3(grid), dim3(64), 0, st, (const u8*)c->d_src, (const zpk_decode_desc*)(aux + aux_desc), (const u32*)(aux + aux_list),
                           c->pj.d_flags + ZPJ_CNT, (u64*)c->pj.d_recs, state, rep_out, d.comp_size);
    }
    hipLaunchKernelGGL(k_zpj_lit, dim3((u32)nb), dim3(64), 0, st, c->d_src, arena_off + lit_total, arena_off, (const ZpjBlock*)ZB, (u32)nb, c->pj.d_flags);
    hipLaunchKernelGGL(k_zpj_reps, dim3(1), dim3(64), 0, st, ZB, (u32)nb, (const u32*)state, (const u32*)rep_out, c->pj.d_flags);
    hipLaunchKernelGGL(k_zpj_pos, dim3((u32)nb), dim3(256), 0, st, (const ZpjBlock*)ZB, B, (u32)nb, (const u64*)c->pj.d_recs, (u64*)c->pj.d_zpos, (u32*)c->pj.d_masks, c->pj.d_flags);
    hipLaunchKernelGGL(k_pj_scan, dim3(1), dim3(64), 0, st, B, (u32)nb, c->pj.d_flags);
    u32 hf[4] = {0, 0, 0, 0};
    e = hipMemcpyAsync(hf, c->pj.d_flags, sizeof(hf), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(hb.data(), B, nb * sizeof(PjBlock), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "large Zstandard frame: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    c->last.zpj_err = hf[PJ_ERR] | ((((u64)hf[PJ_TOTAL + 1] << 32) | hf[PJ_TOTAL]) != n ? 0x40000000u : 0u);
    if (hf[PJ_ERR] || (((u64)hf[PJ_TOTAL + 1] << 32) | hf[PJ_TOTAL]) != n) return ZPK_OK;          // irregular, or the sizes do not add up
    auto init = [&](u32 b0, u32 b1, hipStream_t s2) {
        hipLaunchKernelGGL(k_zpj_init, dim3(b1 - b0), dim3(256), 0, s2, (const ZpjBlock*)ZB, (const PjBlock*)B, b0, (u32)nb, (const u64*)c->pj.d_recs, (const u64*)c->pj.d_zpos,
                           (const u32*)c->pj.d_masks, S, n, c->pj.d_flags);
    };
    return pj_finish(c, d, hb, ZPK_PJ_CHUNK_BLOCKS * PJ_BLOCK / ZPJ_BLOCK, arena_off + lit_total, init, false, dst.staged() ? (u8*)c->d_dst : dst.p, dst.host(), result, redo);
}

// the frames of entries [g0, g1) of `be` as one device batch; redo[k] = 1: entry k takes the serial path after all.
// Dst::None: nothing is handed over.  A group of STORED entries (the caller keeps the kinds apart then) is not cut into pieces and gets
// no slots at all: its staged payloads are hashed where they lie, the partial sums and the chain over c->d_src.
static int decode_big_group(zpk_codec* c, const u8* archive, const zpk_decode_desc* desc, const BigEntry* be, u64 g0, u64 g1,
                            const std::vector<BigSub>& subs, uint8_t* const* dst_ptrs, zpk_decode_result* results, u8* redo, Dst to = Dst::Host,
                            const Planes& pl = Planes())
{
    const u64 ng = g1 - g0;
    std::vector<u64> coff(ng + 1), ooff(ng + 1);
    std::vector<StoredSpanRow> spans(ng);                                              // (the zpk_span of xxh3_span.h, field for field: stored_span.h asserts it)
    std::vector<u64> h_hash(ng);
    std::vector<zpk_decode_desc> hd;
    const HostGroup G = host_group_layout(desc, be, g0, g1, subs.data(), to == Dst::None, coff.data(), ooff.data(), spans.data(), hd);
    const bool src_only = G.src_only;
    const u64 nsub = G.nsub, ct = G.ct, ot = G.ot;
    std::vector<zpk_decode_result> hr(nsub);
    std::vector<const uint8_t*> cptr(ng);
    for (u64 k = 0; k < ng; k++) cptr[k] = archive + desc[be[g0 + k].idx].src_offset;
    int rc;
    if ((rc = grow(c, c->d_src, ct + ZPK_SRC_SLACK)) || (rc = grow(c, c->d_dst, ot + 16)) ||
        (rc = grow(c, c->d_desc, nsub * sizeof(zpk_decode_desc))) ||
        (rc = grow(c, c->d_res, nsub * sizeof(zpk_decode_result)))) return rc;
    hipError_t e = hipSuccess;
    if (ng == 1) e = hipMemcpyAsync(c->d_src, cptr[0], desc[be[g0].idx].comp_size, hipMemcpyHostToDevice, c->stream);
    else {
        const int grc = h2d_gather(c, c->d_src, ct, ng, cptr.data(), [&](u64 k) { return coff[k]; }, [&](u64 k) { return (u64)desc[be[g0 + k].idx].comp_size; }, e, c->stream);
        if (grc) return grc;
    }
    if (e == hipSuccess && nsub) e = hipMemcpyAsync(c->d_desc, hd.data(), nsub * sizeof(zpk_decode_desc), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "H2D: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    // (image size = the staged bytes + 1: the last frame still passes the `offset + comp_size < file_size` guard of :331)
    rc = decode_launch(c, BatchMethods{ G.zstd, G.lz4 }, c->d_src, ct + 1, c->d_src, c->d_src + ct + ZPK_SRC_READ_SLACK, (const zpk_decode_desc*)c->d_desc, nsub,
                       c->d_dst, ot, (zpk_decode_result*)c->d_res, c->stream);
    if (rc) return rc;
    if ((rc = xxh3_spans_launch(c, src_only ? c->d_src : c->d_dst, (const zpk_span*)spans.data(), ng, G.part_blocks, h_hash.data(), c->stream))) return rc;
    if (nsub) e = hipMemcpyAsync(hr.data(), c->d_res, nsub * sizeof(zpk_decode_result), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "decode: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    for (u64 k = 0, j = 0; k < ng; k++) {
        const BigEntry& E = be[g0 + k];
        const zpk_decode_desc& d = desc[E.idx];
        bool ok = true;
        for (u64 f = 0; f < E.nsub && !src_only; f++, j++) if (hr[j].status != 0 || hr[j].produced != subs[E.first_sub + f].size) ok = false;
        redo[g0 + k] = ok ? 0 : 1;
        if (!ok) continue;
        results[E.idx] = dec_hash_verdict(d, h_hash[k]);
        c->last.big[0]++; c->last.big[1] += (u32)E.nsub;
    }
    if (to == Dst::None) return ZPK_OK;                                                // no destination: the verdicts were all
    if (to == Dst::Device) {                                                           // DEVICE destinations: one launch of k_span_copy
        auto row = [&](u64 k) { return zpk_span_copy{ (u64)(c->d_dst + ooff[k]), (u64)dst_ptrs[be[g0 + k].idx], redo[g0 + k] || pl.refused_at(be[g0 + k].idx) ? 0ull : (u64)desc[be[g0 + k].idx].uncomp_size }; };   // (a refused base: no byte, the base rule)
        std::vector<u8> gelem;                                                         // (the group's element sizes and bases, in its own order)
        std::vector<const u8*> gbase;
        if (pl.any()) { gelem.resize(ng); for (u64 k = 0; k < ng; k++) gelem[k] = (u8)pl.of(be[g0 + k].idx); }
        if (pl.base) { gbase.resize(ng); for (u64 k = 0; k < ng; k++) gbase[k] = pl.base_of(be[g0 + k].idx); }
        std::vector<zpk_window> gwin;                                                  // (... and its windows)
        if (pl.win) { gwin.resize(ng); for (u64 k = 0; k < ng; k++) gwin[k] = pl.win[be[g0 + k].idx]; }
        std::vector<u64> gpitch;                                                       // (... and their pitches)
        if (pl.pitch) { gpitch.resize(ng); for (u64 k = 0; k < ng; k++) gpitch[k] = pl.pitch[be[g0 + k].idx]; }
        if ((rc = rows_enqueue(c, ng, row, Planes{ pl.any() ? gelem.data() : nullptr, pl.base ? gbase.data() : nullptr, nullptr, pl.win ? gwin.data() : nullptr, pl.pitch ? gpitch.data() : nullptr }, PLANE_JOIN, c->stream))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return ZPK_OK;
    }
    std::vector<uint8_t*> optr(ng);
    for (u64 k = 0; k < ng; k++) optr[k] = dst_ptrs[be[g0 + k].idx];
    rc = d2h_scatter(c, c->d_dst, ot, ng, optr.data(), [&](u64 k) { return ooff[k]; }, [&](u64 k) { return redo[g0 + k] ? 0ull : (u64)desc[be[g0 + k].idx].uncomp_size; }, e);
    if (rc) return rc;
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "D2H: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    sat_add(c->last.home, ot);
    return ZPK_OK;
}

// a large single frame that the walk (host_walk.h, on the host or by k_big_walk) accepted: entry idx of its batch and its block table
struct PjEntry { u64 idx; std::vector<PjBlock> blocks; int independent; std::vector<ZpjBlock> zblocks; u64 slots, lit_total; };
// ... the walk on the host over entry d (LZ4 or Zstandard) whose bytes are at p: true = accepted, P is its PjEntry
static bool walk_single(const u8* p, const zpk_decode_desc& d, u64 idx, PjEntry& P)
{
    P.idx = idx; P.independent = 0; P.slots = P.lit_total = 0;
    return d.method == ZPK_METHOD_LZ4 ? walk_lz4_single(p, d.comp_size, d.uncomp_size, P.blocks, P.independent)
                                      : walk_zstd_single(p, d.comp_size, d.uncomp_size, P.zblocks, P.slots, P.lit_total);
}

// Which single frames go block-parallel: dec_choose (dec_plan.h).  `pj` = the accepted frames of the batch desc[0, n); those that stay, in
// the order they are to run, are the block-parallel ones (zpk_codec_decode_batch_host and zpk_codec_decode_big_batch_device)
static void pj_choose(const zpk_decode_desc* desc, u64 n, std::vector<PjEntry>& pj)
{
    std::vector<u64> cand(pj.size());
    for (size_t k = 0; k < pj.size(); k++) cand[k] = pj[k].idx;
    std::vector<PjEntry> chosen;
    for (u64 k : dec_choose(desc, n, cand.data(), cand.size())) chosen.push_back(std::move(pj[k]));
    pj.swap(chosen);
}

// One accepted frame through the block-parallel reader of its method.  -> ZPK_OK with redo = 0: decoded, hashed, delivered, `result` is
// its verdict; redo = 1: not this path's, `result` is to be ignored (the one-wave decoder decides)
static int decode_big_single(zpk_codec* c, PjEntry& P, const zpk_decode_desc& d, const BigSrc& src, const BigDst& dst, zpk_decode_result& result, u8& redo)
{
    if (d.method == ZPK_METHOD_LZ4) return decode_big_lz4_single(c, src, d, P.blocks, P.independent, dst, result, redo);
    return decode_big_zstd_single(c, src, d, P.zblocks, P.slots, P.lit_total, dst, result, redo);
}

// the counts decode_stats2 reports of the most recent decode call: none yet
static void begin_decode_call(zpk_codec* c) { LastCall& l = c->last; l.no_planes(); l.big[0] = l.big[1] = 0; l.walk[0] = l.walk[1] = 0; l.span[0] = l.span[1] = 0; l.pipe = l.sc = 0; l.subs = 0; l.home = 0; l.vstored = 0; }

static int decode_batch_host_plain(zpk_codec* c, const uint8_t* archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                   uint8_t* const* dst_ptrs, zpk_decode_result* results, Dst to = Dst::Host, const Planes& pl = Planes())
{
    if (n == 0) return ZPK_OK;
    // (no destination: the sub-batches are cut by ZPK_OPT_DIMAGE_CHUNK, as those of a device image are — a caller can force several cheaply)
    const u64 chunk_bytes = to == Dst::None ? dimage_chunk(c->opt.dimage_chunk) : ZPK_HOST_CHUNK_BYTES;
    int rc = ZPK_OK;
    u8* gathered = nullptr; u64 gathered_cap = 0;
    try {
        std::vector<zpk_decode_desc> hd;
        std::vector<u64> at(n);                                                       // entry i lies at at[i] of ITS sub-batch's staging
        for (u64 first = 0; first < n && rc == ZPK_OK; ) {
            // ---- the sub-batch, cut by the size of its output slots (host_plan.h: read_slot; dimage_cut, as a device image's are) ----
            const DimageCut cut = dimage_cut(first, n, chunk_bytes, [&](u64 i) { return read_slot(to == Dst::None, desc[i]); }, at.data() + first);
            const u64 cnt = cut.count, out_total = cut.out_total;
            if (host_staging_refused(out_total)) { snprintf(c->err, sizeof(c->err), "a staging slot of %llu bytes", (unsigned long long)out_total); rc = ZPK_E_NOMEM; break; }
            hd.resize(cnt);
            for (u64 k = 0; k < cnt; k++) hd[k] = span_copy_staged_desc(desc[first + k], desc[first + k].method == ZPK_METHOD_NONE, at[first + k]);
            const HostSub sub = host_sub(desc + first, cnt, archive_size);
            const u8* image = archive; u64 image_size = archive_size, lo = sub.lo, hi = sub.hi;
            if (host_image_sparse(sub.lo, sub.hi, sub.comp_sum)) {
                // sparse picks out of a large archive: stage only the payloads, gathered into an image of their own (host_gather_layout)
                const HostGather G = host_gather_layout(desc + first, cnt, archive_size, hd.data());
                if (G.image_size + 1 > gathered_cap) { free(gathered); gathered = (u8*)malloc(G.image_size + 1); gathered_cap = gathered ? G.image_size + 1 : 0; }
                if (!gathered) { rc = ZPK_E_NOMEM; break; }
                for (u64 k = 0; k < cnt; k++) if (hd[k].src_offset != G.fail_offset) memcpy(gathered + hd[k].src_offset, archive + desc[first + k].src_offset, desc[first + k].comp_size);
                gathered[G.pad_at] = 0;
                image = gathered; image_size = G.image_size; lo = 0; hi = G.pad_at;
            }
            const BatchMethods holds = { sub.zstd, sub.lz4 };
            bool piped = false;
            uint8_t* const* const sub_ptrs = dst_ptrs ? dst_ptrs + first : nullptr;
            c->last.subs++;
            rc = decode_host_pipelined(c, image, image_size, lo, hi, hd.data(), desc + first, cnt, out_total, sub_ptrs, results + first, piped, holds, to, pl.from(first));
            if (rc == ZPK_OK && !piped)
                rc = decode_host_chunk(c, image, image_size, lo, hi, hd.data(), desc + first, cnt, out_total, sub_ptrs, results + first, holds, to, pl.from(first));
            first += cnt;
        }
    } catch (...) { rc = ZPK_E_NOMEM; }
    free(gathered);
    return rc;
}

// zpk_codec_decode_batch_host, zpk_codec_decode_batch_host_dptr and zpk_codec_verify_batch_host: one routing, the destinations host
// memory, device memory or none (Dst)
static int decode_batch_host_routed(zpk_codec* c, const uint8_t* archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                    uint8_t* const* dst_ptrs, zpk_decode_result* results, Dst to, const Planes& pl);
// base_hash (the _delta_checked call; else NULL): the value the base of entry i has to hash to — the base rule, beside planes_join_len
static int decode_batch_host_any(zpk_codec* c, const uint8_t* archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                 uint8_t* const* dst_ptrs, zpk_decode_result* results, Dst to, const Planes& pl = Planes(), const u64* base_hash = nullptr)
{
    const bool ddst = to == Dst::Device;
    if (!c || (n && (!desc || !results || (!dst_ptrs && to != Dst::None)))) return ZPK_E_INVALID;
    if (n == 0) return ZPK_OK;
    CodecLock lk(c);
    HIPCHK(c, hipSetDevice(c->device));
    if (planes_check(c, pl.elem, n)) return ZPK_E_INVALID;
    std::vector<zpk_decode_desc> staged;                                              // (the windows: their rule, and the slots of the entries that have one)
    if (const int wrc = windows_check(c, pl, desc, n, ddst, staged)) return wrc;
    if (placed_hash_check(c, pl, base_hash, n)) return ZPK_E_INVALID;
    // the pointer rule (PtrRule): before anything is enqueued.  (A window's destination and base hold window_bytes bytes, a placed one's place_extent: Planes::dst_len.)
    PtrRule rule(c);
    if (ddst && rule.batch("destination", n, [&](u64 i) { return dst_ptrs[i]; }, [&](u64 i) { return pl.room(i, desc[i].dst_capacity); })) return ZPK_E_INVALID;
    if (bases_check(c, rule, pl, n, [&](u64 i) { return pl.dst_len(i, desc[i].uncomp_size); }, dst_ptrs)) return ZPK_E_INVALID;
    begin_decode_call(c);
    // the base rule: every verdict is known before anything of the batch is routed, so before any row reaches rows_enqueue
    std::vector<u8> refused;
    int rc = base_verdicts(c, pl, base_hash, n, [&](u64 i) { return pl.dst_len(i, desc[i].uncomp_size); }, refused);
    if (rc) return rc;
    if (!staged.empty()) desc = staged.data();
    rc = decode_batch_host_routed(c, archive, archive_size, desc, n, dst_ptrs, results, to, Planes{ pl.elem, pl.base, refused.empty() ? nullptr : refused.data(), pl.win, pl.pitch });
    if (rc == ZPK_OK) base_verdicts_mark(refused, desc, results, n);
    return rc;
}
// ... what the call does once its arguments have passed: the lock is held, the device is the codec's
static int decode_batch_host_routed(zpk_codec* c, const uint8_t* archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                    uint8_t* const* dst_ptrs, zpk_decode_result* results, Dst to, const Planes& pl)
{
    const bool ddst = to == Dst::Device;
    // ---- which entries are sequences of frames worth decoding frame-parallel ----
    std::vector<BigEntry> be;
    std::vector<BigSub> subs;
    std::vector<PjEntry> pj;                                                          // large single frames (lz4_pj.h, zstd_pj.h)
    if (archive && c->opt.dec_split_min != ~0ull) {
        try {
            for (u64 i = 0; i < n; i++) {
                const zpk_decode_desc& d = desc[i];
                if (!dec_big_candidate(d, archive_size, c->opt.dec_split_min)) continue;      // (an entry that earns a verdict from a guard gets it from the usual path)
                const size_t s0 = subs.size();
                bool ok = false;
                if (d.method == ZPK_METHOD_NONE) {
                    if (d.comp_size == d.uncomp_size && d.uncomp_size > ZPK_ENC_PIECE) {
                        for (u64 o = 0; o < d.uncomp_size; o += ZPK_ENC_PIECE) {
                            const u64 len = d.uncomp_size - o < ZPK_ENC_PIECE ? d.uncomp_size - o : (u64)ZPK_ENC_PIECE;
                            subs.push_back(BigSub{ o, len, o, len });
                        }
                        ok = true;
                    }
                } else {
                    const u8* const p = archive + d.src_offset;
                    ok = d.method == ZPK_METHOD_LZ4 ? walk_lz4_frames(p, d.comp_size, d.uncomp_size, subs) : walk_zstd_frames(p, d.comp_size, d.uncomp_size, subs);
                    PjEntry P;                                                        // ONE frame (what the reference writes): block-parallel
                    if (!ok && walk_single(p, d, i, P)) pj.push_back(std::move(P));
                }
                if (ok) be.push_back(BigEntry{ i, (u64)s0, (u64)(subs.size() - s0) });
            }
        } catch (...) { be.clear(); subs.clear(); pj.clear(); }                       // out of host memory for the plan: the usual path
    }
    if (be.empty() && pj.empty()) return decode_batch_host_plain(c, archive, archive_size, desc, n, dst_ptrs, results, to, pl);
    int rc = ZPK_OK;
    try {
        std::vector<u8> redo(be.size(), 0), is_big(n, 0);
        for (u64 g0 = 0; g0 < be.size() && rc == ZPK_OK; ) {                          // groups by the size of their output
            const u64 g1 = host_group_cut(desc, be.data(), be.size(), g0, to == Dst::None);
            rc = decode_big_group(c, archive, desc, be.data(), g0, g1, subs, dst_ptrs, results, redo.data(), to, pl);
            g0 = g1;
        }
        // ---- everything else, and the entries a frame of which did not decode, through the usual path ----
        for (u64 k = 0; k < be.size(); k++) if (!redo[k]) is_big[be[k].idx] = 1;
        pj_choose(desc, n, pj);
        for (u64 k = 0; k < pj.size() && rc == ZPK_OK; k++) {                         // one large frame at a time: each fills the chip
            u8 again = 1;
            const u64 idx = pj[k].idx;
            // a device destination is decoded into straight away — unless the entry has an element size above 1, a base or a window: that one
            // decodes into the staging, as an entry without a destination does, and is JOINED (or cut) from there
            const bool grouped = ddst && pl.grouped(idx);
            rc = decode_big_single(c, pj[k], desc[idx], BigSrc{ archive, false }, grouped ? BigDst{ nullptr, Dst::None } : BigDst{ to == Dst::None ? nullptr : dst_ptrs[idx], to }, results[idx], again);
            if (rc == ZPK_OK && !again && grouped) {
                const u8 k1 = (u8)pl.of(idx);
                const u8* const b1 = pl.base_of(idx);
                if (k1 > 1) c->last.planes[3]++; else if (b1) c->last.delta[3]++; else c->last.window[2]++;     // (staged because it was grouped; staged only because it had a base; ... a window)
                const zpk_span_copy row = { (u64)(u8*)c->d_dst, (u64)dst_ptrs[idx], pl.join_len(idx, desc[idx], results[idx]) };
                const zpk_window w1 = pl.win ? pl.win[idx] : zpk_window{ 0, 0, 0, 0, 0 };
                const u64 p1 = pl.pitch_of(idx);
                if ((rc = rows_enqueue(c, 1, [&](u64) { return row; }, Planes{ &k1, pl.base ? &b1 : nullptr, nullptr, pl.win ? &w1 : nullptr, pl.pitch ? &p1 : nullptr }, PLANE_JOIN, c->stream)) == ZPK_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = ZPK_E_LAUNCH;
            }
            if (rc == ZPK_OK && !again) is_big[idx] = 1;
        }
        std::vector<u64> rest;
        for (u64 i = 0; i < n; i++) if (!is_big[i]) rest.push_back(i);
        if (rc == ZPK_OK && !rest.empty()) {
            std::vector<zpk_decode_desc> rd(rest.size());
            std::vector<uint8_t*> rp(rest.size());
            std::vector<zpk_decode_result> rr(rest.size());
            std::vector<u8> re(pl.any() ? rest.size() : 0);
            std::vector<const u8*> rb(pl.base ? rest.size() : 0);
            std::vector<u8> rf(pl.refused ? rest.size() : 0);
            std::vector<zpk_window> rw(pl.win ? rest.size() : 0);
            std::vector<u64> rpitch(pl.pitch ? rest.size() : 0);
            for (u64 k = 0; k < rest.size(); k++) {
                rd[k] = desc[rest[k]]; rp[k] = to == Dst::None ? nullptr : dst_ptrs[rest[k]];
                if (pl.any()) re[k] = (u8)pl.of(rest[k]);
                if (pl.base) rb[k] = pl.base_of(rest[k]);
                if (pl.refused) rf[k] = pl.refused[rest[k]];
                if (pl.win) rw[k] = pl.win[rest[k]];
                if (pl.pitch) rpitch[k] = pl.pitch[rest[k]];
            }
            rc = decode_batch_host_plain(c, archive, archive_size, rd.data(), rest.size(), rp.data(), rr.data(), to,
                                         Planes{ pl.any() ? re.data() : nullptr, pl.base ? rb.data() : nullptr, pl.refused ? rf.data() : nullptr, pl.win ? rw.data() : nullptr, pl.pitch ? rpitch.data() : nullptr });
            if (rc == ZPK_OK) for (u64 k = 0; k < rest.size(); k++) results[rest[k]] = rr[k];
        }
    } catch (...) { rc = ZPK_E_NOMEM; }
    return rc;
}

int zpk_codec_decode_batch_host(zpk_codec* c, const uint8_t* archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                uint8_t* const* dst_ptrs, zpk_decode_result* results)
{
    return decode_batch_host_any(c, archive, archive_size, desc, n, dst_ptrs, results, Dst::Host);
}

int zpk_codec_decode_batch_host_dptr(zpk_codec* c, const uint8_t* archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                     uint8_t* const* d_dst_ptrs, zpk_decode_result* results)
{
    return decode_batch_host_any(c, archive, archive_size, desc, n, d_dst_ptrs, results, Dst::Device);
}

int zpk_codec_decode_batch_host_dptr_placed(zpk_codec* c, const uint8_t* archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                            uint8_t* const* d_dst_ptrs, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base,
                                            const uint64_t* base_hash, const zpk_window* win, const uint64_t* pitch)
{
    return decode_batch_host_any(c, archive, archive_size, desc, n, d_dst_ptrs, results, Dst::Device, Planes{ elem, d_base, nullptr, win, pitch }, base_hash);
}

int zpk_codec_decode_batch_host_dptr_windows(zpk_codec* c, const uint8_t* archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                             uint8_t* const* d_dst_ptrs, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base,
                                             const uint64_t* base_hash, const zpk_window* win)
{
    return zpk_codec_decode_batch_host_dptr_placed(c, archive, archive_size, desc, n, d_dst_ptrs, results, elem, d_base, base_hash, win, nullptr);
}

int zpk_codec_decode_batch_host_dptr_delta_checked(zpk_codec* c, const uint8_t* archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                                   uint8_t* const* d_dst_ptrs, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base,
                                                   const uint64_t* base_hash)
{
    return zpk_codec_decode_batch_host_dptr_windows(c, archive, archive_size, desc, n, d_dst_ptrs, results, elem, d_base, base_hash, nullptr);
}

int zpk_codec_decode_batch_host_dptr_delta(zpk_codec* c, const uint8_t* archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                           uint8_t* const* d_dst_ptrs, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base)
{
    return zpk_codec_decode_batch_host_dptr_delta_checked(c, archive, archive_size, desc, n, d_dst_ptrs, results, elem, d_base, nullptr);
}

int zpk_codec_decode_batch_host_dptr_planes(zpk_codec* c, const uint8_t* archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                            uint8_t* const* d_dst_ptrs, zpk_decode_result* results, const uint8_t* elem)
{
    return zpk_codec_decode_batch_host_dptr_delta(c, archive, archive_size, desc, n, d_dst_ptrs, results, elem, nullptr);
}

int zpk_codec_copy_spans_device(zpk_codec* c, const zpk_span_copy* rows, uint64_t n, void* stream)
{
    if (!c || (n && !rows)) return ZPK_E_INVALID;
    if (n == 0) return ZPK_OK;
    CodecLock lk(c);
    HIPCHK(c, hipSetDevice(c->device));
    PtrRule rule(c);                                                                  // the pointer rule, on both ends of every span
    auto len = [&](u64 i) { return (u64)rows[i].len; };
    if (rule.batch("span source", n, [&](u64 i) { return (const void*)rows[i].src; }, len) ||
        rule.batch("span destination", n, [&](u64 i) { return (const void*)rows[i].dst; }, len)) return ZPK_E_INVALID;
    return span_copy_enqueue(c, n, [&](u64 i) { return rows[i]; }, stream ? (hipStream_t)stream : c->stream);
}

// rows of k_plane_copy on their own: element size, direction and both ends per row; the pointer rule on both ends of every row
int zpk_codec_plane_copy_device(zpk_codec* c, const zpk_plane_copy* rows, uint64_t n, void* stream)
{
    if (!c || (n && !rows)) return ZPK_E_INVALID;
    CodecLock lk(c);
    c->last.no_planes();
    if (n == 0) return ZPK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    for (u64 i = 0; i < n; i++) if (!elem_size_ok(c, "row", i, rows[i].elem)) return ZPK_E_INVALID;
    PtrRule rule(c);
    auto len = [&](u64 i) { return (u64)rows[i].len; };
    if (rule.batch("plane source", n, [&](u64 i) { return (const void*)rows[i].src; }, len) ||
        rule.batch("plane destination", n, [&](u64 i) { return (const void*)rows[i].dst; }, len)) return ZPK_E_INVALID;
    return plane_copy_enqueue(c, n, [&](u64 i) { return rows[i]; }, stream ? (hipStream_t)stream : c->stream);
}

// rows of k_delta_copy on their own: element size, direction, both ends and the base per row; the pointer rule on all three ends of every
// row, and the overlap rule between base and destination (delta_overlap_ok) — on refusal nothing has run
int zpk_codec_delta_copy_device(zpk_codec* c, const zpk_delta_copy* rows, uint64_t n, void* stream)
{
    if (!c || (n && !rows)) return ZPK_E_INVALID;
    CodecLock lk(c);
    c->last.no_planes();
    if (n == 0) return ZPK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    for (u64 i = 0; i < n; i++) {
        if (!elem_size_ok(c, "row", i, rows[i].elem)) return ZPK_E_INVALID;
        if (rows[i].len && !rows[i].base) { snprintf(c->err, sizeof(c->err), "row %llu has no base: a row of zpk_codec_plane_copy_device", (unsigned long long)i); return ZPK_E_INVALID; }
    }
    PtrRule rule(c);
    auto len = [&](u64 i) { return (u64)rows[i].len; };
    if (rule.batch("delta source", n, [&](u64 i) { return (const void*)rows[i].src; }, len) ||
        rule.batch("delta destination", n, [&](u64 i) { return (const void*)rows[i].dst; }, len) ||
        rule.batch("delta base", n, [&](u64 i) { return (const void*)rows[i].base; }, len)) return ZPK_E_INVALID;
    for (u64 i = 0; i < n; i++)
        if (!delta_overlap_ok(rows[i].base, rows[i].dst, rows[i].len) || (!rows[i].join && rows[i].len && rows[i].base == rows[i].dst)) {
            snprintf(c->err, sizeof(c->err), "row %llu: the base overlaps the destination (only a join may have base == dst, exactly)", (unsigned long long)i);
            return ZPK_E_INVALID;
        }
    return delta_copy_enqueue(c, n, [&](u64 i) { return rows[i]; }, stream ? (hipStream_t)stream : c->stream);
}

// the most recent call that could split or join: out[0] rows split with a base, out[1] rows joined with a base, out[2] k_delta_copy
// launches, out[3] entries that decoded into the staging only because they had a base
int zpk_codec_delta_stats(zpk_codec* c, uint32_t out[4])
{
    if (!c || !out) return ZPK_E_INVALID;
    CodecLock lk(c);
    for (int k = 0; k < 4; k++) out[k] = c->last.delta[k];
    return ZPK_OK;
}

// rows of k_window_copy on their own: element size, window, both ends and the base (0: none) per row; window_valid, the pointer rule on
// all three ends of every row — the source over n bytes, destination and base over window_bytes — and the overlap rule between base and
// destination (window_overlap_ok) — on refusal nothing has run
int zpk_codec_window_copy_device(zpk_codec* c, const zpk_window_copy* rows, uint64_t n, void* stream)
{
    if (!c || (n && !rows)) return ZPK_E_INVALID;
    CodecLock lk(c);
    c->last.no_planes();
    if (n == 0) return ZPK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    auto win = [&](u64 i) { const zpk_window& w = rows[i].win; return Window{ w.row_bytes, w.row0, w.rows, w.col0, w.cols }; };
    for (u64 i = 0; i < n; i++) {
        if (!elem_size_ok(c, "row", i, rows[i].elem)) return ZPK_E_INVALID;
        if (!window_valid(rows[i].n, rows[i].elem, win(i))) { snprintf(c->err, sizeof(c->err), "row %llu: its window does not lie in %llu bytes of %u-byte elements", (unsigned long long)i, (unsigned long long)rows[i].n, (unsigned)rows[i].elem); return ZPK_E_INVALID; }
    }
    PtrRule rule(c);
    auto len = [&](u64 i) { return window_bytes(win(i)); };
    if (rule.batch("window source", n, [&](u64 i) { return (const void*)rows[i].src; }, [&](u64 i) { return len(i) ? (u64)rows[i].n : 0ull; }) ||
        rule.batch("window destination", n, [&](u64 i) { return (const void*)rows[i].dst; }, len) ||
        rule.batch("window base", n, [&](u64 i) { return (const void*)rows[i].base; }, [&](u64 i) { return rows[i].base ? len(i) : 0ull; })) return ZPK_E_INVALID;
    for (u64 i = 0; i < n; i++)
        if (rows[i].base && !window_overlap_ok(rows[i].base, rows[i].dst, win(i))) {
            snprintf(c->err, sizeof(c->err), "row %llu: the base overlaps the destination without being it", (unsigned long long)i);
            return ZPK_E_INVALID;
        }
    return window_copy_enqueue(c, n, [&](u64 i) { return rows[i]; }, stream ? (hipStream_t)stream : c->stream);
}

// window_valid and window_overlap_ok (window_copy_plan.h) for the callers that judge a window before they have a codec
int zpk_codec_window_valid(uint64_t n, uint32_t elem, const zpk_window* win, uint64_t* bytes)
{
    if (!win) return 0;
    const Window w = { win->row_bytes, win->row0, win->rows, win->col0, win->cols };
    if (!window_valid(n, elem, w)) return 0;
    if (bytes) *bytes = window_bytes(w);
    return 1;
}
int zpk_codec_window_overlap_ok(uint64_t base, uint64_t dst, const zpk_window* win)
{
    return win && window_overlap_ok(base, dst, Window{ win->row_bytes, win->row0, win->rows, win->col0, win->cols }) ? 1 : 0;
}

// the most recent call that could split, join or cut: out[0] rows windowed, out[1] k_window_copy launches, out[2] entries that decoded
// into the staging only because they had a window
int zpk_codec_window_stats(zpk_codec* c, uint32_t out[3])
{
    if (!c || !out) return ZPK_E_INVALID;
    CodecLock lk(c);
    for (int k = 0; k < 3; k++) out[k] = c->last.window[k];
    return ZPK_OK;
}

// rows of k_place_copy on their own: element size, window, pitch, both ends and the base (0: none) per row; place_valid, the pointer rule
// on all three ends of every row — the source over n bytes, destination and base over place_extent — and the overlap rule between base
// and destination (place_overlap_ok) — on refusal nothing has run
int zpk_codec_place_copy_device(zpk_codec* c, const zpk_place_copy* rows, uint64_t n, void* stream)
{
    if (!c || (n && !rows)) return ZPK_E_INVALID;
    CodecLock lk(c);
    c->last.no_planes();
    if (n == 0) return ZPK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    auto win = [&](u64 i) { const zpk_window& w = rows[i].win; return Window{ w.row_bytes, w.row0, w.rows, w.col0, w.cols }; };
    for (u64 i = 0; i < n; i++) {
        if (!elem_size_ok(c, "row", i, rows[i].elem)) return ZPK_E_INVALID;
        if (!place_valid(rows[i].n, rows[i].elem, win(i), rows[i].pitch)) {
            snprintf(c->err, sizeof(c->err), "row %llu: its window does not lie in %llu bytes of %u-byte elements, or not at a pitch of %llu", (unsigned long long)i, (unsigned long long)rows[i].n,
                     (unsigned)rows[i].elem, (unsigned long long)rows[i].pitch);
            return ZPK_E_INVALID;
        }
    }
    PtrRule rule(c);
    auto ext = [&](u64 i) { return place_extent(win(i), rows[i].pitch); };
    if (rule.batch("place source", n, [&](u64 i) { return (const void*)rows[i].src; }, [&](u64 i) { return ext(i) ? (u64)rows[i].n : 0ull; }) ||
        rule.batch("place destination", n, [&](u64 i) { return (const void*)rows[i].dst; }, ext) ||
        rule.batch("place base", n, [&](u64 i) { return (const void*)rows[i].base; }, [&](u64 i) { return rows[i].base ? ext(i) : 0ull; })) return ZPK_E_INVALID;
    for (u64 i = 0; i < n; i++)
        if (rows[i].base && !place_overlap_ok(rows[i].base, rows[i].dst, win(i), rows[i].pitch)) {
            snprintf(c->err, sizeof(c->err), "row %llu: the base overlaps the destination without being it", (unsigned long long)i);
            return ZPK_E_INVALID;
        }
    return place_copy_enqueue(c, n, [&](u64 i) { return rows[i]; }, stream ? (hipStream_t)stream : c->stream);
}

// place_valid and place_overlap_ok (place_copy_plan.h) for the callers that judge a placement before they have a codec
int zpk_codec_place_valid(uint64_t n, uint32_t elem, const zpk_window* win, uint64_t pitch, uint64_t* extent)
{
    if (!win) return 0;
    const Window w = { win->row_bytes, win->row0, win->rows, win->col0, win->cols };
    if (!place_valid(n, elem, w, pitch)) return 0;
    if (extent) *extent = place_extent(w, pitch);
    return 1;
}
int zpk_codec_place_overlap_ok(uint64_t base, uint64_t dst, const zpk_window* win, uint64_t pitch)
{
    return win && place_overlap_ok(base, dst, Window{ win->row_bytes, win->row0, win->rows, win->col0, win->cols }, pitch) ? 1 : 0;
}

// the most recent call that could split, join, cut or place: out[0] rows placed, out[1] k_place_copy launches
int zpk_codec_place_stats(zpk_codec* c, uint32_t out[2])
{
    if (!c || !out) return ZPK_E_INVALID;
    CodecLock lk(c);
    out[0] = c->last.place[0]; out[1] = c->last.place[1];
    return ZPK_OK;
}

// XXH3-64 of rows of device memory on their own (k_span_hash and the chip-wide pair): the pointer rule on every row — on refusal nothing
// has run —, then one pass; the hashes are home when the call returns
int zpk_codec_hash_spans_device(zpk_codec* c, const zpk_hash_span* rows, uint64_t n, uint64_t* out_hashes, void* stream)
{
    if (!c || (n && (!rows || !out_hashes))) return ZPK_E_INVALID;
    CodecLock lk(c);
    for (int k = 0; k < 4; k++) c->last.base_check[k] = 0;
    if (n == 0) return ZPK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    PtrRule rule(c);
    if (rule.batch("span", n, [&](u64 i) { return (const void*)rows[i].addr; }, [&](u64 i) { return (u64)rows[i].len; })) return ZPK_E_INVALID;
    return span_hash_run(c, n, [&](u64 i) { return SpanHashRow{ rows[i].addr, rows[i].len }; }, out_hashes, stream ? (hipStream_t)stream : c->stream);
}

// the most recent call that hashed spans or could have (the _delta_checked reads, the reads they extend): out[0] rows hashed by one wave,
// out[1] rows hashed chip-wide, out[2] bases that did not hash to their value, out[3] launches of the hash pass
int zpk_codec_base_check_stats(zpk_codec* c, uint32_t out[4])
{
    if (!c || !out) return ZPK_E_INVALID;
    CodecLock lk(c);
    for (int k = 0; k < 4; k++) out[k] = c->last.base_check[k];
    return ZPK_OK;
}

// the most recent call that could split or join: out[0] rows split, out[1] rows joined, out[2] k_plane_copy launches, out[3] entries that
// decoded into the staging only because they were grouped
int zpk_codec_planes_stats(zpk_codec* c, uint32_t out[4])
{
    if (!c || !out) return ZPK_E_INVALID;
    CodecLock lk(c);
    for (int k = 0; k < 4; k++) out[k] = c->last.planes[k];
    return ZPK_OK;
}

uint64_t zpk_codec_packed_stride(uint64_t uncomp_size) { return span_copy_packed_stride(uncomp_size); }

// ---- large STORED entries of a device-resident call, copied and hashed by the whole chip (round 17; stored_plan.h, stored_span.h) ----
// The entries of desc[0, n) that stored_span_takes, in one k_stored_span (the copy fused with the XXH3 partial sums, any number of spans),
// one k_xxh3_chain with one wave per span — on the SOURCE, so it does not wait for the copy's bytes — and the copy home of the hashes,
// all enqueued on run.st: the codec's stream or, `fork`, a second stream beside it (the slots are disjoint, and the chain is one wave per
// span, so the rest of the chip is free while it runs).  The table goes up from pinned memory the codec owns and the hashes land there.
// run.idx = the entries taken (none when the option is off, nothing qualifies or there is no memory for the tables: those stay with the
// one-wave launch); stored_span_finish waits for run.st and composes their results.  A run that goes out of scope unfinished — every
// error path of its call — waits too: nothing stays in flight that reads the pinned block or writes the caller's slots.
struct StoredSpanRun {
    std::vector<u64> idx; const u64* h_hash = nullptr; hipStream_t st = nullptr;
    ~StoredSpanRun() { if (st) (void)hipStreamSynchronize(st); }
};
// hash_only (the batch has no destination): the entries have no slots — dst_size does not bound them, and k_xxh3_partials over the source
// stands in for k_stored_span: the same sums in the same places without the copy; the chain behind them hashes from the source either way.
static int stored_span_enqueue(zpk_codec* c, const u8* d_archive, u64 archive_size, const zpk_decode_desc* desc, u64 n, u8* d_dst, u64 dst_size,
                               bool fork, StoredSpanRun& run, bool hash_only = false)
{
    if (c->opt.stored_span_min == ~0ull) return ZPK_OK;
    if (hash_only) dst_size = ~0ull;
    u64 k = 0;
    for (u64 i = 0; i < n; i++) k += stored_span_takes(desc[i], archive_size, dst_size, c->opt.stored_span_min) ? 1 : 0;
    if (k == 0) return ZPK_OK;
    const hipStream_t st = fork && fork_stream(c->sspan.side, c->stream, false) ? c->sspan.side.s : c->stream;
    const u64 dst_at = (k * sizeof(StoredSpanRow) + 255) & ~255ull, up_bytes = dst_at + ((k * 8 + 255) & ~255ull), h_total = up_bytes + k * 8;
    if (!c->sspan.h.grow(h_total)) return ZPK_OK;                            // no pinned memory for the table: one wave per entry
    u8* const h_sspan = c->sspan.h.p;
    StoredSpanRow* const rows = (StoredSpanRow*)h_sspan;
    u64* const dst_off = (u64*)(h_sspan + dst_at);
    StoredPlan plan = { 0, 0, 0 };
    run.idx.reserve(k);
    for (u64 i = 0; i < n; i++)
        if (stored_span_takes(desc[i], archive_size, dst_size, c->opt.stored_span_min)) {
            if (!stored_span_emit(desc[i], rows, dst_off, plan)) break;              // the launch is full: the rest stays one wave per entry
            run.idx.push_back(i);
        }
    if (plan.nspans == 0) return ZPK_OK;
    const u64 part_at = up_bytes, hash_at = part_at + plan.part_blocks * 64;
    if (grow(c, c->sspan.d, hash_at + plan.nspans * 8 + 64)) { c->err[0] = 0; run.idx.clear(); return ZPK_OK; }
    const zpk_span* const d_spans = (const zpk_span*)(u8*)c->sspan.d;
    u64* const d_part = (u64*)(c->sspan.d + part_at);
    u64* const d_hash = (u64*)(c->sspan.d + hash_at);
    run.h_hash = (const u64*)(h_sspan + up_bytes);
    run.st = st;
    HIPCHK(c, hipMemcpyAsync(c->sspan.d, h_sspan, up_bytes, hipMemcpyHostToDevice, st));
    if (hash_only) hipLaunchKernelGGL(k_xxh3_partials, dim3((u32)((plan.groups + 3) / 4)), dim3(256), 0, st, d_archive, d_spans, (u32)plan.nspans, (u64)0, plan.groups, d_part);
    else hipLaunchKernelGGL(k_stored_span, dim3((u32)((plan.groups + 3) / 4)), dim3(256), 0, st, d_archive, d_dst, d_spans,
                       (const u64*)(c->sspan.d + dst_at), (u32)plan.nspans, plan.groups, d_part);
    hipLaunchKernelGGL(k_xxh3_chain, dim3((u32)plan.nspans), dim3(64), 0, st, d_archive, d_spans, (const u64*)d_part, d_hash, (u64*)nullptr, (u64)0, ~(u64)0, 1);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_sspan + up_bytes, d_hash, plan.nspans * 8, hipMemcpyDeviceToHost, st));
    c->last.span[0] += (u32)plan.nspans; c->last.span[1] += (u32)(plan.groups > 0xFFFFFFFFull ? 0xFFFFFFFFull : plan.groups);      // (+=: as last.walk)
    return ZPK_OK;
}
// ... the join: their stream has drained -> their hashes are in the pinned block, their results are composed
static int stored_span_finish(zpk_codec* c, StoredSpanRun& run, const zpk_decode_desc* desc, zpk_decode_result* results)
{
    if (run.idx.empty()) return ZPK_OK;
    const hipStream_t st = run.st;
    run.st = nullptr;
    HIPCHK(c, hipStreamSynchronize(st));
    for (u64 k = 0; k < run.idx.size(); k++) results[run.idx[k]] = dec_hash_verdict(desc[run.idx[k]], run.h_hash[k]);
    return ZPK_OK;
}

// The one-wave tail of the device-resident calls: entries desc[rest[0, nr)] through the one-wave kernels in ONE launch over their
// descriptors, exactly as zpk_codec_decode_batch_device would (every verdict other than OK / hash mismatch is theirs), their results
// scattered to results[rest[k]]; returns when they are home.  No entry left while the stored spans took some: no work list held an entry
// in this call, the counters say so.
static int decode_rest_device(zpk_codec* c, const u8* d_archive, u64 archive_size, const zpk_decode_desc* desc, const u64* rest, u64 nr,
                              u8* d_dst, u64 dst_size, zpk_decode_result* results, bool hash_only = false)
{
    if (nr == 0) {
        if (c->last.span[0]) { (void)hipMemsetAsync(c->d_counters, 0, N_COUNTERS * sizeof(u32), c->stream); c->last.totals_valid = 0; }
        return ZPK_OK;
    }
    std::vector<zpk_decode_desc> rd(nr);
    std::vector<zpk_decode_result> rr(nr);
    for (u64 k = 0; k < nr; k++) rd[k] = desc[rest[k]];
    int rc;
    if ((rc = grow(c, c->d_desc, nr * sizeof(zpk_decode_desc))) || (rc = grow(c, c->d_res, nr * sizeof(zpk_decode_result)))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_desc, rd.data(), nr * sizeof(zpk_decode_desc), hipMemcpyHostToDevice, c->stream));
    if ((rc = decode_launch(c, BatchMethods{ -1, -1 }, d_archive, archive_size, d_archive, d_archive + archive_size, (const zpk_decode_desc*)c->d_desc, nr,
                            d_dst, dst_size, (zpk_decode_result*)c->d_res, c->stream, hash_only))) return rc;
    HIPCHK(c, hipMemcpyAsync(rr.data(), c->d_res, nr * sizeof(zpk_decode_result), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (u64 k = 0; k < nr; k++) results[rest[k]] = rr[k];
    return ZPK_OK;
}

// ONE entry whose compressed bytes are ON THE DEVICE, decoded into device memory (round 5; the device-pointer form of what
// zpk_codec_decode_batch_host does for a large single frame).  desc and result are HOST memory; the call returns when the entry is
// decoded and verified.  A large entry that is one frame of the reference writer is decoded block-parallel (lz4_pj.h / zstd_pj.h): its
// compressed bytes come to the host once, into a pinned buffer, for the walk over the block headers (2.6 ms for 130 MiB; the walk on
// the device, k_big_walk, measured 1.77 ms for such an LZ4 entry but 77.6 ms for a Zstandard one: profiles/r15), everything else stays
// on the device — a sole candidate always goes block-parallel, the chooser (dec_choose) is the batch call's.  Any other entry — and any
// entry the block-parallel path does not finish — is decoded by the one-wave kernels, exactly as zpk_codec_decode_batch_device would.
int zpk_codec_decode_big_device(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size, const zpk_decode_desc* desc,
                                uint8_t* d_dst, uint64_t dst_size, zpk_decode_result* result)
{
    if (!c || !desc || !result || !d_archive) return ZPK_E_INVALID;
    CodecLock lk(c);
    HIPCHK(c, hipSetDevice(c->device));
    begin_decode_call(c);
    const zpk_decode_desc d = *desc;
    int rc = ZPK_OK;
    bool done = false;                                                                // a chip-wide path has finished the entry
    try {
        if (d_dst && stored_span_takes(d, archive_size, dst_size, c->opt.stored_span_min)) {   // a large stored entry: copied and hashed chip-wide (serial form)
            StoredSpanRun run;
            if ((rc = stored_span_enqueue(c, d_archive, archive_size, &d, 1, d_dst, dst_size, false, run)) || (rc = stored_span_finish(c, run, &d, result))) return rc;
            done = !run.idx.empty();
        } else if (d_dst && dec_big_candidate_device(d, archive_size, dst_size, c->opt.dec_split_min) && c->walk.h_bigsrc.grow(d.comp_size)) {
            u8* const h_src = c->walk.h_bigsrc.p;                                          // (no pinned memory for the entry's bytes: one wave)
            hipError_t e = hipMemcpyAsync(h_src, d_archive + d.src_offset, d.comp_size, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "large entry: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
            PjEntry P;
            if (walk_single(h_src, d, 0, P)) {
                zpk_decode_result r; memset(&r, 0, sizeof(r));
                u8 redo = 1;
                if ((rc = decode_big_single(c, P, d, BigSrc{ d_archive, true }, BigDst{ d_dst + d.dst_offset, Dst::Device }, r, redo))) return rc;
                if (!redo) { *result = r; done = true; }
            }
        }
    } catch (...) { c->last.span[0] = c->last.span[1] = 0; }                          // out of host memory for a table: one wave
    const u64 self = 0;
    try { rc = decode_rest_device(c, d_archive, archive_size, &d, &self, done ? 0 : 1, d_dst, dst_size, result); } catch (...) { rc = ZPK_E_NOMEM; }
    return rc;
}

// A BATCH whose compressed bytes are ON THE DEVICE and whose output stays there, with large entries in it (the batch form of
// zpk_codec_decode_big_device, the read-side mirror of zpk_codec_encode_big_device).  desc and results are HOST memory; the call returns
// when every entry is decoded and verified.  The compressed bytes never leave the device: k_big_walk (big_walk.h) walks the block headers
// of every candidate (dec_big_candidate_device, as in zpk_codec_decode_big_device) side by side where they lie, one copy brings the tables home.
// Of the frames the walk accepted, pj_choose picks those worth a turn of the whole chip (lz4_pj.h / zstd_pj.h, one after the other);
// every other entry — and every entry the block-parallel path does not finish — is decoded by the one-wave kernels in ONE launch over
// their descriptors, exactly as zpk_codec_decode_batch_device would: every verdict other than OK / hash mismatch is theirs.
// (the body: the caller holds the lock, has set the device and called begin_decode_call — zpk_codec_decode_batch_dimage runs it once per
// sub-batch, with d_dst = the codec's own staging; to = Dst::None there when the batch is only tested: the stored entries have no slot in
// d_dst and are hashed where they lie, large ones chip-wide, everything else decodes into its slot as ever)
static int decode_big_batch_body(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                 uint8_t* d_dst, uint64_t dst_size, zpk_decode_result* results, Dst to = Dst::Device)
{
    const bool hash_only = to == Dst::None;
    int rc = ZPK_OK;
    StoredSpanRun span;                                                               // (declared in front of the try: it waits on every way out)
    try {
        // ---- the large stored entries: copy + XXH3 across the chip.  Serial form: on c->stream, in front of the walk.  Forked form: on a
        // second stream beside the walk, the block-parallel entries and the one-wave launch.
        if ((rc = stored_span_enqueue(c, d_archive, archive_size, desc, n, d_dst, dst_size, ZPK_STORED_SPAN_FORK != 0, span, hash_only))) return rc;
        // ---- the candidates, walked where they lie: one launch over all of them, one copy home (records + tables), one synchronisation ----
        std::vector<u64> cand;
        for (u64 i = 0; i < n; i++) if (dec_big_candidate_device(desc[i], archive_size, dst_size, c->opt.dec_split_min)) cand.push_back(i);
        const u64 nc = cand.size();
        std::vector<BigWalkItem> items;
        const BigWalkLayout L = dec_walk_layout(desc, cand.data(), nc, items);
        std::vector<PjEntry> pj;
        bool walk = nc > 0 && c->walk.h_bigwalk.grow(L.total);
        if (walk && grow(c, c->walk.d_bigwalk, L.total)) { c->err[0] = 0; walk = false; }  // no memory for the tables, pinned or on the device: one wave per entry
        if (walk) {
            u8* const h_walk = c->walk.h_bigwalk.p;
            memcpy(h_walk, items.data(), nc * sizeof(BigWalkItem));
            HIPCHK(c, hipMemcpyAsync(c->walk.d_bigwalk, h_walk, nc * sizeof(BigWalkItem), hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_big_walk, dim3((u32)nc), dim3(64), 0, c->stream, d_archive, (const BigWalkItem*)(u8*)c->walk.d_bigwalk, (u32)nc,
                               (u8*)c->walk.d_bigwalk, (BigWalkRec*)(c->walk.d_bigwalk + L.rec_off));
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(h_walk + L.rec_off, c->walk.d_bigwalk + L.rec_off, L.total - L.rec_off, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            const BigWalkRec* const recs = (const BigWalkRec*)(h_walk + L.rec_off);
            c->last.walk[0] += (u32)nc;                                                // (+=: begin_decode_call zeroed it; the sub-batches of zpk_codec_decode_batch_dimage add up)
            for (u64 k = 0; k < nc; k++) {
                const BigWalkRec& r = recs[k];
                if (r.accepted != 1 || r.nblocks == 0 || r.nblocks > items[k].cap) continue;
                c->last.walk[1]++;
                PjEntry P; P.idx = cand[k]; P.independent = (int)(r.independent & 1); P.slots = r.slots; P.lit_total = r.lit_total;
                if (items[k].method == ZPK_METHOD_LZ4) { const PjBlock* t = (const PjBlock*)(h_walk + items[k].tab_off); P.blocks.assign(t, t + r.nblocks); }
                else { const ZpjBlock* t = (const ZpjBlock*)(h_walk + items[k].tab_off); P.zblocks.assign(t, t + r.nblocks); }
                pj.push_back(std::move(P));
            }
        }
        pj_choose(desc, n, pj);
        std::vector<u8> is_big(n, 0);
        for (u64 i : span.idx) is_big[i] = 1;                                         // (composed behind the join, below)
        for (u64 k = 0; k < pj.size(); k++) {                                         // one large frame at a time: each fills the chip
            const zpk_decode_desc& d = desc[pj[k].idx];
            zpk_decode_result r; memset(&r, 0, sizeof(r));
            u8 again = 1;
            if ((rc = decode_big_single(c, pj[k], d, BigSrc{ d_archive, true }, BigDst{ d_dst + d.dst_offset, Dst::Device }, r, again))) return rc;
            if (!again) { results[pj[k].idx] = r; is_big[pj[k].idx] = 1; }
        }
        // ---- everything else through the one-wave kernels, one launch (every verdict is theirs) ----
        std::vector<u64> rest;
        for (u64 i = 0; i < n; i++) if (!is_big[i]) rest.push_back(i);
        if ((rc = decode_rest_device(c, d_archive, archive_size, desc, rest.data(), rest.size(), d_dst, dst_size, results, hash_only))) return rc;
        rc = stored_span_finish(c, span, desc, results);
    } catch (...) { rc = ZPK_E_NOMEM; }
    return rc;
}

int zpk_codec_decode_big_batch_device(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                      uint8_t* d_dst, uint64_t dst_size, zpk_decode_result* results)
{
    if (!c || (n && (!desc || !results || !d_archive || !d_dst))) return ZPK_E_INVALID;
    if (n == 0) return ZPK_OK;
    if (n > 0x7FFFFFF0ull) return ZPK_E_INVALID;
    CodecLock lk(c);
    HIPCHK(c, hipSetDevice(c->device));
    begin_decode_call(c);
    return decode_big_batch_body(c, d_archive, archive_size, desc, n, d_dst, dst_size, results);
}

// ---- the ARCHIVE IMAGE in the caller's device memory, the destinations host or device pointers (dimage_plan.h) ----------------------------
// zpk_codec_decode_batch_host / _host_dptr for a reader whose image lies in device memory: the batch is cut into sub-batches by the size
// of their staging slots (dimage_cut), each runs the body of zpk_codec_decode_big_batch_device with d_dst = c->d_dst — the walk on the
// device, dec_choose, the stored spans, one one-wave launch for the rest: the verdicts come from where they always came from — and
// deliver_slots hands the slots over as the host path does: one k_span_copy to device pointers; the copy home and the scatter to host
// pointers.  The compressed bytes never cross the bus.  (Dst::None — zpk_codec_verify_batch_dimage: the same sub-batches and the same body;
// nothing is handed over, only descriptors go up and verdicts come home.)
static int decode_batch_dimage_any(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                   uint8_t* const* dst_ptrs, Dst to, zpk_decode_result* results, const Planes& pl_given = Planes(), const u64* base_hash = nullptr)
{
    if (!c || (n && (!desc || !results || (!dst_ptrs && to != Dst::None) || !d_archive))) return ZPK_E_INVALID;
    CodecLock lk(c);
    HIPCHK(c, hipSetDevice(c->device));
    c->last.dimage[0] = c->last.dimage[1] = c->last.dimage[2] = 0;
    if (n == 0) return ZPK_OK;
    if (planes_check(c, pl_given.elem, n)) return ZPK_E_INVALID;
    const bool ddst = to == Dst::Device, none = to == Dst::None;
    PtrRule rule(c);                                                                  // the pointer rule: before anything is enqueued
    if (rule.batch("archive image", 1, [&](u64) { return d_archive; }, [&](u64) { return (u64)archive_size; })) return ZPK_E_INVALID;
    std::vector<zpk_decode_desc> staged;                                              // (the windows: their rule, and the slots of the entries that have one)
    if (const int wrc = windows_check(c, pl_given, desc, n, ddst, staged)) return wrc;
    if (placed_hash_check(c, pl_given, base_hash, n)) return ZPK_E_INVALID;
    if (ddst && rule.batch("destination", n, [&](u64 i) { return dst_ptrs[i]; }, [&](u64 i) { return pl_given.room(i, desc[i].dst_capacity); })) return ZPK_E_INVALID;
    if (bases_check(c, rule, pl_given, n, [&](u64 i) { return pl_given.dst_len(i, desc[i].uncomp_size); }, dst_ptrs)) return ZPK_E_INVALID;
    begin_decode_call(c);
    // the base rule (beside planes_join_len): every verdict is known before the first sub-batch is decoded, so before any row reaches
    // rows_enqueue; the column is cut with the others (Planes::from)
    std::vector<u8> refused;
    if (const int vrc = base_verdicts(c, pl_given, base_hash, n, [&](u64 i) { return pl_given.dst_len(i, desc[i].uncomp_size); }, refused)) return vrc;
    if (!staged.empty()) desc = staged.data();
    const Planes pl = { pl_given.elem, pl_given.base, refused.empty() ? nullptr : refused.data(), pl_given.win, pl_given.pitch };
    const u64 chunk = dimage_chunk(c->opt.dimage_chunk);
    auto slot = [&](u64 i) { return read_slot(none, desc[i]); };                      // (host_plan.h: the host path's slot)
    int rc = ZPK_OK;
    u64 home_total = 0;
    try {
        std::vector<zpk_decode_desc> hd;
        std::vector<u64> at(n);                                                       // entry i lies at at[i] of ITS sub-batch's staging
        for (u64 first = 0; first < n && rc == ZPK_OK; ) {
            const DimageCut cut = dimage_cut(first, n, chunk, slot, at.data() + first);
            hd.resize(cut.count);
            for (u64 k = 0; k < cut.count; k++) hd[k] = span_copy_staged_desc(desc[first + k], desc[first + k].method == ZPK_METHOD_NONE, at[first + k]);      // (as in the host path)
            if (cut.out_total > ~0ull - 16) { snprintf(c->err, sizeof(c->err), "a staging slot of %llu bytes", (unsigned long long)cut.out_total); rc = ZPK_E_NOMEM; break; }
            if ((rc = grow(c, c->d_dst, cut.out_total + 16))) break;
            if ((rc = decode_big_batch_body(c, d_archive, archive_size, hd.data(), cut.count, c->d_dst, cut.out_total, results + first, none ? Dst::None : Dst::Device))) break;
            u64 home = 0;
            if ((rc = deliver_slots(c, hd.data(), desc + first, cut.count, cut.out_total, dst_ptrs ? dst_ptrs + first : nullptr, results + first, to, &home, pl.from(first)))) break;
            sat_add(home_total, home);
            c->last.dimage[0]++; c->last.subs++;
            first += cut.count;
        }
    } catch (...) { rc = ZPK_E_NOMEM; }
    c->last.dimage[1] = c->last.sc;
    c->last.dimage[2] = home_total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)home_total;
    if (rc == ZPK_OK) base_verdicts_mark(refused, desc, results, n);
    return rc;
}

int zpk_codec_decode_batch_dimage(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                  uint8_t* const* dst_ptrs, int dst_on_device, zpk_decode_result* results)
{
    return decode_batch_dimage_any(c, d_archive, archive_size, desc, n, dst_ptrs, dst_on_device ? Dst::Device : Dst::Host, results);
}

// (element sizes and bases belong to DEVICE destinations: with host destinations every element size has to be 1 and no entry has a base)
// (... and so do windows and pitches: with host destinations no entry has one)
int zpk_codec_decode_batch_dimage_placed(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                         uint8_t* const* dst_ptrs, int dst_on_device, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base,
                                         const uint64_t* base_hash, const zpk_window* win, const uint64_t* pitch)
{
    if (!dst_on_device) for (u64 i = 0; i < n; i++) if ((elem && elem[i] != 1) || (d_base && d_base[i]) || (win && win[i].row_bytes) || (pitch && pitch[i])) return ZPK_E_INVALID;
    return decode_batch_dimage_any(c, d_archive, archive_size, desc, n, dst_ptrs, dst_on_device ? Dst::Device : Dst::Host, results,
                                   Planes{ dst_on_device ? elem : nullptr, dst_on_device ? d_base : nullptr, nullptr, dst_on_device ? win : nullptr, dst_on_device ? pitch : nullptr }, base_hash);
}

int zpk_codec_decode_batch_dimage_windows(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                          uint8_t* const* dst_ptrs, int dst_on_device, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base,
                                          const uint64_t* base_hash, const zpk_window* win)
{
    return zpk_codec_decode_batch_dimage_placed(c, d_archive, archive_size, desc, n, dst_ptrs, dst_on_device, results, elem, d_base, base_hash, win, nullptr);
}

int zpk_codec_decode_batch_dimage_delta_checked(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                                uint8_t* const* dst_ptrs, int dst_on_device, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base,
                                                const uint64_t* base_hash)
{
    return zpk_codec_decode_batch_dimage_windows(c, d_archive, archive_size, desc, n, dst_ptrs, dst_on_device, results, elem, d_base, base_hash, nullptr);
}

int zpk_codec_decode_batch_dimage_delta(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                        uint8_t* const* dst_ptrs, int dst_on_device, zpk_decode_result* results, const uint8_t* elem, const uint8_t* const* d_base)
{
    return zpk_codec_decode_batch_dimage_delta_checked(c, d_archive, archive_size, desc, n, dst_ptrs, dst_on_device, results, elem, d_base, nullptr);
}

int zpk_codec_decode_batch_dimage_planes(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                         uint8_t* const* dst_ptrs, int dst_on_device, zpk_decode_result* results, const uint8_t* elem)
{
    return zpk_codec_decode_batch_dimage_delta(c, d_archive, archive_size, desc, n, dst_ptrs, dst_on_device, results, elem, nullptr);
}

// ---- a batch that is only TESTED: the verdicts of the two calls above without a destination (Dst::None) --------------------------------------
// The descriptors as the routing sees them: dst_offset and dst_capacity of the caller's are ignored, the capacity counts as uncomp_size —
// what an exact-size buffer gives, so BUFFER_TOO_SMALL cannot occur.
static std::vector<zpk_decode_desc> verify_descs(const zpk_decode_desc* desc, u64 n)
{
    std::vector<zpk_decode_desc> vd(desc, desc + n);
    for (zpk_decode_desc& d : vd) { d.dst_offset = 0; d.dst_capacity = d.uncomp_size; }
    return vd;
}
// the stored entries that were hashed where they lay: those with a payload that passed every guard (OK or a hash mismatch is all that is left)
static void verify_count_stored(zpk_codec* c, const zpk_decode_desc* desc, const zpk_decode_result* results, u64 n)
{
    u64 k = 0;
    for (u64 i = 0; i < n; i++) k += desc[i].method == ZPK_METHOD_NONE && desc[i].comp_size != 0 && (results[i].status == DEC_R_OK || results[i].status == DEC_R_FILE_HASH_MISMATCH);
    c->last.vstored = k > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)k;
}

int zpk_codec_verify_batch_host(zpk_codec* c, const uint8_t* archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                zpk_decode_result* results)
{
    if (!c || (n && (!desc || !results))) return ZPK_E_INVALID;
    CodecLock lk(c);
    begin_decode_call(c);
    if (n == 0) return ZPK_OK;
    int rc;
    try {
        const std::vector<zpk_decode_desc> vd = verify_descs(desc, n);
        rc = decode_batch_host_any(c, archive, archive_size, vd.data(), n, nullptr, results, Dst::None);
        if (rc == ZPK_OK) verify_count_stored(c, vd.data(), results, n);
    } catch (...) { rc = ZPK_E_NOMEM; }
    return rc;
}

int zpk_codec_verify_batch_dimage(zpk_codec* c, const uint8_t* d_archive, uint64_t archive_size, const zpk_decode_desc* desc, uint64_t n,
                                  zpk_decode_result* results)
{
    if (!c || (n && (!desc || !results || !d_archive))) return ZPK_E_INVALID;
    CodecLock lk(c);
    begin_decode_call(c);
    if (n == 0) return ZPK_OK;
    int rc;
    try {
        const std::vector<zpk_decode_desc> vd = verify_descs(desc, n);
        rc = decode_batch_dimage_any(c, d_archive, archive_size, vd.data(), n, nullptr, Dst::None, results);
        if (rc == ZPK_OK) verify_count_stored(c, vd.data(), results, n);
    } catch (...) { rc = ZPK_E_NOMEM; }
    return rc;
}

// the most recent of the two: out[0] sub-batches, out[1] stored entries hashed where they lay, out[2] plaintext bytes that came home
// (saturating; 0: such a call brings none), out[3] 0
int zpk_codec_verify_stats(zpk_codec* c, uint32_t out[4])
{
    if (!c || !out) return ZPK_E_INVALID;
    CodecLock lk(c);
    out[0] = c->last.subs; out[1] = c->last.vstored; out[2] = c->last.home > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)c->last.home; out[3] = 0;
    return ZPK_OK;
}

int zpk_codec_dimage_stats(zpk_codec* c, uint32_t out[4])
{
    if (!c || !out) return ZPK_E_INVALID;
    CodecLock lk(c);
    out[0] = c->last.dimage[0]; out[1] = c->last.dimage[1]; out[2] = c->last.dimage[2]; out[3] = 0;
    return ZPK_OK;
}

int zpk_codec_hash_batch_device(zpk_codec* c, const uint8_t* src, const uint64_t* offsets, const uint64_t* sizes, uint64_t n,
                                uint64_t* hashes, void* stream)
{
    if (!c) return ZPK_E_INVALID;
    if (n == 0) return ZPK_OK;
    CodecLock lk(c);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    hipLaunchKernelGGL(k_hash, dim3((u32)((n + 3) / 4)), dim3(256), 0, st, src, offsets, sizes, n, hashes);
    HIPCHK(c, hipGetLastError());
    return ZPK_OK;
}

int zpk_codec_hash_host(zpk_codec* c, const uint8_t* data, uint64_t size, uint64_t* hash)
{
    if (!c || !hash) return ZPK_E_INVALID;
    CodecLock lk(c);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = grow(c, c->d_src, size + 16)) || (rc = grow(c, c->d_res, 64))) return rc;
    u64 meta[3] = { 0, size, 0 };
    if (size) HIPCHK(c, hipMemcpyAsync(c->d_src, data, size, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_res, meta, sizeof(meta), hipMemcpyHostToDevice, c->stream));
    u64* m = (u64*)c->d_res;
    hipLaunchKernelGGL(k_hash, dim3(1), dim3(64), 0, c->stream, c->d_src, m, m + 1, (u64)1, m + 2);
    HIPCHK(c, hipMemcpyAsync(hash, m + 2, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ZPK_OK;
}

// debugging: copy the per-entry phase timing words (8 x u64 per entry; needs ZPK_DEBUG_TIMING=1) to the host
int zpk_codec_debug_read(zpk_codec* c, void* host, uint64_t bytes)
{
    if (!c || !c->d_dbg || bytes > c->d_dbg.cap) return ZPK_E_INVALID;      // d_dbg exists only in a -DZPK_DEVELOPER build
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(host, c->d_dbg, bytes, hipMemcpyDeviceToHost));
    return ZPK_OK;
}

// counters of the most recent decode batch (synchronises the device): out[0..2] = entries per work list
// (none, zstd, lz4), out[3] = Zstandard entries finished on pre-decoded sequences, out[4] = by the fused decoder
int zpk_codec_decode_stats(zpk_codec* c, uint32_t out[8])
{
    if (!c || !out) return ZPK_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    u32 h[N_COUNTERS];
    HIPCHK(c, hipMemcpy(h, c->d_counters, sizeof(h), hipMemcpyDeviceToHost));
    if (c->last.totals_valid) memcpy(h, c->last.host_totals, sizeof(h));          // a pipelined host batch: the sum over its launches
    out[0] = h[C_NONE]; out[1] = h[C_ZSTD]; out[2] = h[C_LZ4] + h[C_LZ4_RUNS] + h[C_LZ4_GEN] /* the three LZ4 lists */; out[3] = h[C_ZSTD_TWO_STAGE]; out[4] = h[C_ZSTD_FUSED];
    out[5] = h[C_FSE_WATCHDOG]; out[6] = h[C_FSE_BUDGET]; out[7] = h[C_FSE_MARKED];
    if (c->last.fell_back_fused) out[7] |= 0x80000000u;          // the batch could not get its sequence arena: fused decoder only
    ZPK_DEV(if (getenv("ZPK_TRACE")) fprintf(stderr, "[zpk] fse marked %u, pass-0 failures %u, last failure status/rc %08x\n", h[C_FSE_MARKED], h[C_EXEC_FAILED], h[C_EXEC_LAST_RC]);)
    return ZPK_OK;
}

// out[0], out[1] = LZ4 / Zstandard entries of the most recent decode batch whose first decode ran out of its time budget and that
// were decoded again by the retry launches (expected 0 on an idle GPU)
int zpk_codec_decode_stats2(zpk_codec* c, uint32_t out[16])
{
    if (!c || !out) return ZPK_E_INVALID;
    CodecLock lk(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    u32 h[N_COUNTERS];
    HIPCHK(c, hipMemcpy(h, c->d_counters, sizeof(h), hipMemcpyDeviceToHost));
    if (c->last.totals_valid) memcpy(h, c->last.host_totals, sizeof(h));
    memset(out, 0, ZPK_DS2_COUNT * sizeof(uint32_t));                                  // (ZPK_DS2_RESERVED2, _RESERVED4: the two-stage path of round 4 is gone, they read 0)
    out[ZPK_DS2_RETRY_LZ4] = h[C_RETRY_LZ4]; out[ZPK_DS2_RETRY_ZSTD] = h[C_RETRY_ZSTD];
    out[ZPK_DS2_LZ4_RUNS] = h[C_LZ4_RUNS];                                             // LZ4 entries that are mostly runs, decoded by k_lz4_left
    out[ZPK_DS2_BIG_ENTRIES] = c->last.big[0]; out[ZPK_DS2_BIG_FRAMES] = c->last.big[1];
    out[ZPK_DS2_ZPJ_ERR] = c->last.zpj_err;                                            // why the most recent large Zstandard frame was NOT finished block-parallel (0: it was, or none came)
    out[ZPK_DS2_LZ4_HANDED] = h[C_LZ4_HANDED];                                         // LZ4 entries k_lz4_wave handed to the general decoder without judging them
    out[ZPK_DS2_LZ4_GEN] = h[C_LZ4_GEN];                                               // LZ4 entries whose header is not that of a plain frame: k_lz4_general's
    out[ZPK_DS2_WALKED] = c->last.walk[0]; out[ZPK_DS2_WALK_ACCEPTED] = c->last.walk[1];     // zpk_codec_decode_big_batch_device: entries walked on the device (k_big_walk), those the walk accepted
    out[ZPK_DS2_SPAN_ENTRIES] = c->last.span[0]; out[ZPK_DS2_SPAN_GROUPS] = c->last.span[1]; // ... and zpk_codec_decode_big_device: stored entries copied chip-wide (k_stored_span), their groups
    out[ZPK_DS2_PIPE_SUBS] = c->last.pipe; out[ZPK_DS2_SPAN_COPIES] = c->last.sc;      // zpk_codec_decode_batch_host / _dptr: sub-batches through the three-stage pipeline; k_span_copy launches (_dptr)
    return ZPK_OK;
}

// developer aid: read back part of the Zstandard sequence arena (what = 0, byte offset = the entry's dst_offset
// rounded up to 8) or of the per-entry marks (what = 1, u32 per entry) of the most recent decode batch
int zpk_codec_debug_fetch(zpk_codec* c, int what, uint64_t offset, void* host, uint64_t bytes)
{
    if (!c || !host) return ZPK_E_INVALID;
    const u8* base = what == 0 ? (const u8*)c->wave.d_zarena : (const u8*)c->wave.d_zstate;
    const u64 cap = what == 0 ? c->wave.d_zarena.cap : c->wave.d_zstate.cap;
    if (!base || offset > cap || bytes > cap - offset) return ZPK_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(host, base + offset, bytes, hipMemcpyDeviceToHost));
    return ZPK_OK;
}

int zpk_codec_set_option(zpk_codec* c, int option, int value)
{
    if (!c) return ZPK_E_INVALID;
    CodecLock lk(c);
    if (option == ZPK_OPT_ORDER_FAST_LAST) { c->opt.order_fast_last = value ? 1 : 0; return ZPK_OK; }
    if (option == ZPK_OPT_ORDER_MIN) { if (value < 0) return ZPK_E_INVALID; c->opt.order_min = c->opt.enc_order_min = value == 0 ? ~0ull : (u64)value; return ZPK_OK; }
    if (option == ZPK_OPT_DEC_SPLIT_MIN) { if (value < 0) return ZPK_E_INVALID; c->opt.dec_split_min = value == 0 ? ~0ull : (u64)value; return ZPK_OK; }
    if (option == ZPK_OPT_ENC_SPLIT_MIN) { if (value < 0) return ZPK_E_INVALID; c->opt.enc_split_min = value == 0 ? ~0ull : (u64)value; return ZPK_OK; }
    if (option == ZPK_OPT_STORED_SPAN_MIN) { if (value < 0) return ZPK_E_INVALID; c->opt.stored_span_min = value == 0 ? ~0ull : (u64)value; return ZPK_OK; }
    if (option == ZPK_OPT_SPAN_HASH_MIN) { if (value < 0) return ZPK_E_INVALID; c->opt.span_hash_min = value == 0 ? ~0ull : (u64)value; return ZPK_OK; }
    if (option == ZPK_OPT_DIMAGE_CHUNK) { if (value < 0) return ZPK_E_INVALID; c->opt.dimage_chunk = (u64)value; return ZPK_OK; }       // (0 = the default: dimage_chunk())
    return ZPK_E_INVALID;
}

int zpk_codec_set_profiling(zpk_codec* c, int enabled)
{
    if (!c) return ZPK_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (enabled)
        for (int i = 0; i < ZPK_K_COUNT; i++) for (int j = 0; j < 2; j++)
            if (const hipError_t e = c->kev[i][j].ready(hipEventDefault)) { snprintf(c->err, sizeof(c->err), "profiling: no event: %s", hipGetErrorString(e)); return ZPK_E_LAUNCH; }
    c->profiling = enabled ? 1 : 0;
    return ZPK_OK;
}

int zpk_codec_kernel_ms(zpk_codec* c, int which, float* ms)
{
    if (!c || !ms || which < 0 || which >= ZPK_K_COUNT || !c->kev[which][1]) return ZPK_E_INVALID;
    HIPCHK(c, hipEventSynchronize(c->kev[which][1]));
    HIPCHK(c, hipEventElapsedTime(ms, c->kev[which][0], c->kev[which][1]));
    return ZPK_OK;
}

int zpk_codec_timer_start(zpk_codec* c, void* stream)
{
    if (!c) return ZPK_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventRecord(c->ev0, stream ? (hipStream_t)stream : c->stream));
    return ZPK_OK;
}

int zpk_codec_timer_stop(zpk_codec* c, void* stream, float* elapsed_ms)
{
    if (!c || !elapsed_ms) return ZPK_E_INVALID;
    HIPCHK(c, hipEventRecord(c->ev1, stream ? (hipStream_t)stream : c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    HIPCHK(c, hipEventElapsedTime(elapsed_ms, c->ev0, c->ev1));
    return ZPK_OK;
}

}  // extern "C"

#include "zpk_encode.inc"
#include "zpk_dsink.inc"
#include "zpk_stream.inc"
