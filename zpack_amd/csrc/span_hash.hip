// span_hash.hip — k_span_hash (span_hash.h) and the chip-wide pair it hands its long rows to, as a code object of its own, and the one
// host function that launches them.  zpk_codec.hip builds the tables and calls span_hash_launch; keeping the kernels out of that file
// keeps its code object, and those of row_copy.hip, sink_commit.hip and stored_hash.hip, unchanged.
#include <hip/hip_runtime.h>
// xxh3_span.h, which span_hash.h includes as it is, defines the kernels k_xxh3_partials and k_xxh3_chain, and zpk_codec.hip owns those
// names: a second definition would not link.  The copies compiled here are the ones this file launches, under names of their own.
#define k_xxh3_partials k_span_hash_partials
#define k_xxh3_chain k_span_hash_chain
#include "span_hash.h"
#undef k_xxh3_partials
#undef k_xxh3_chain

namespace zpk {

// Everything of one plan, on `st`: d_block holds the tables as span_hash_layout lays them out.  The one-wave rows in launches of at most
// max_wave_rows, the groups of the chip-wide rows in launches of at most max_groups, then their chains in launches of at most max_chains
// (the partial sums of a row are complete before its chain starts: same stream).  Returns the number of launches.
u32 span_hash_launch(u8* d_block, const SpanHashPlan& p, const SpanHashLayout& L, u64 max_wave_rows, u64 max_groups, u64 max_chains, hipStream_t st)
{
    u32 launches = 0;
    const SpanHashRow* const wave = (const SpanHashRow*)(d_block + L.wave_rows);
    const zpk_span* const wide = (const zpk_span*)(d_block + L.wide_rows);
    u64* const out = (u64*)(d_block + L.out);
    u64* const partial = (u64*)(d_block + L.partial);
    for (u64 j = 0, nl = span_hash_launches(p.nwave, max_wave_rows); j < nl; j++, launches++) {
        const SpanHashLaunch W = span_hash_launch(p.nwave, j, max_wave_rows, 4);
        hipLaunchKernelGGL(k_span_hash, dim3(W.grid), dim3(256), 0, st, wave, W.first, W.first + W.count, out);
    }
    for (u64 j = 0, nl = span_hash_launches(p.groups, max_groups); j < nl; j++, launches++) {
        const SpanHashLaunch G = span_hash_launch(p.groups, j, max_groups, 4);
        hipLaunchKernelGGL(k_span_hash_partials, dim3(G.grid), dim3(256), 0, st, (const u8*)nullptr, wide, (u32)p.nwide, G.first, G.first + G.count, partial);
    }
    for (u64 j = 0, nl = span_hash_launches(p.nwide, max_chains); j < nl; j++, launches++) {
        const SpanHashLaunch C = span_hash_launch(p.nwide, j, max_chains, 1);
        hipLaunchKernelGGL(k_span_hash_chain, dim3(C.grid), dim3(64), 0, st, (const u8*)nullptr, wide + C.first, (const u64*)partial, out + p.nwave + C.first,
                           (u64*)nullptr, (u64)0, (u64)0, 1);
    }
    return launches;
}

}  // namespace zpk
