// copy_rows_plan.h — what the five ROW COPIES share: k_span_copy, k_plane_copy, k_delta_copy, k_window_copy and k_place_copy (row_copy.hip)
// each read a table of rows, one wave per 16 KiB work item of a row, and a table past one grid goes in several launches.  Decided here, in one place:
// the piece, the limits, the count of a row's items, the search a wave finds its row by, and the launch split.  What a row IS — its
// struct, its emit, what an item of it covers — belongs to the table's own header: span_copy_plan.h, plane_copy_plan.h,
// delta_copy_plan.h, window_copy_plan.h, place_copy_plan.h.
// Plain C++17, pj_types.h and standard headers only: tools/hostfuzz builds this file with g++ under ASan + UBSan (g++ knows no HIP),
// which keeps it so.  copy_items is also device code: ZPK_HD is empty on a CPU build.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "pj_types.h"                            // (the typedefs)
#ifndef ZPK_HD
#ifdef __HIPCC__
#define ZPK_HD __host__ __device__
#else
#define ZPK_HD
#endif
#endif

namespace zpk {

// ---- the row table ---------------------------------------------------------------------------------------------------------------------
// A WORK ITEM is 16 KiB of one row, one wave's: 64 lanes x 16 bytes x 4 loads in flight, four times.  Row r owns the items
// [item_base, item_base + copy_items(len)); item_base ascends without gaps, so the wave of item t finds its row as the LAST one with
// item_base <= t (the search of k_stored_span over part_base).  A row of no bytes takes no row and no item.  Every Row struct has the
// members len and item_base; its emit appends { ..., p.items } at p.nrows and adds copy_items(len).
#define ZPK_COPY_PIECE (16u << 10)
#define ZPK_COPY_MAX_ROWS 0xFFFFFFFFull              // the kernels search with 32-bit row numbers
struct CopyPlan { u64 nrows, items; };
ZPK_HD static inline u64 copy_items(u64 len) { return len / ZPK_COPY_PIECE + (len % ZPK_COPY_PIECE ? 1 : 0); }       // (no sum that could wrap)
// the row of item t, as the kernels find it
template <class Row> static inline u64 copy_row_of(const Row* rows, u64 nrows, u64 t)
{
    u64 lo = 0, hi = nrows;
    while (hi - lo > 1) { const u64 mid = (lo + hi) >> 1; if (rows[mid].item_base <= t) lo = mid; else hi = mid; }
    return lo;
}

// ---- the launches ----------------------------------------------------------------------------------------------------------------------
// Four items per workgroup; a grid holds at most max_items of them (the x limit of a grid), a table with more goes in several launches
// over the SAME table: launch j takes the items [j * max_items, ...), the kernel adds that base to its wave number.
#define ZPK_COPY_MAX_ITEMS (4ull * 0x7FFFFFFFull)
struct CopyLaunch { u64 item0, items; u32 grid; };
static inline u64 copy_launches(u64 items, u64 max_items = ZPK_COPY_MAX_ITEMS) { return items / max_items + (items % max_items ? 1 : 0); }
static inline CopyLaunch copy_launch(u64 items, u64 j, u64 max_items = ZPK_COPY_MAX_ITEMS)
{
    CopyLaunch L;
    L.item0 = j * max_items;
    L.items = items - L.item0 < max_items ? items - L.item0 : max_items;
    L.grid = (u32)((L.items + 3) / 4);
    return L;
}

}  // namespace zpk
