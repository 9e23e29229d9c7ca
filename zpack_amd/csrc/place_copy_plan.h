// place_copy_plan.h — PLACED reads: an entry, or a window of it, delivered into a 2-D SUB-BLOCK of a larger device tensor.  A checkpoint
// written by 8 tensor-parallel ranks holds 8 shard entries per weight; a loader at another width puts several shards side by side in one
// tensor.  Along dimension 0 that is a pointer offset; along any other each shard is a strided sub-block of the destination, and the
// caller otherwise reads every shard into a scratch buffer and concatenates: a second pass over every plaintext byte and a scratch copy
// of the checkpoint.  The copy that delivers an entry moves every byte anyway, and the placement rides on it (k_place_copy, row_copy.hip,
// beside k_window_copy): what a window read lacks is a destination ROW PITCH.  Decided here, in one place: the pitch, the rule it has to
// pass, the extent, the map, the overlap rule, the row table the kernel reads and the placed offset of a place in an item.  The window,
// its rule, window_plain_index, the items and where a group or a loose byte lies (window_piece, window_group_at, window_loose_at) are
// window_copy_plan.h's, the 16 KiB item, the search and the launches copy_rows_plan.h's, and none is restated.
// Plain C++17 like those headers: tools/hostfuzz builds this file with g++ under ASan + UBSan.
#pragma once
#include "window_copy_plan.h"

namespace zpk {

// ---- the placement ---------------------------------------------------------------------------------------------------------------------
// A placed entry has a valid window w and a pitch p != 0, in bytes: window row r begins at buffer byte r * p.  An entry read whole is the
// window row0 = 0, col0 = 0, cols = row_bytes, rows = n / row_bytes.  The slice [start, start + length) along ONE dimension `dim` of a
// contiguous destination of `shape` and `itemsize` is  rows = prod(shape[:dim]), cols = length * inner, pitch = shape[dim] * inner,
// and the buffer begins start * inner bytes into the tensor, with inner = prod(shape[dim + 1:]) * itemsize.  p needs no alignment to k.
//
// what the placement spans in the buffer, from its first byte to its last: 0 for one of no bytes.  (Only of a pair that passes
// place_valid is the value meaningful: there it does not wrap.)
ZPK_HD static inline u64 place_extent(const Window& w, u64 p) { return w.rows == 0 || w.cols == 0 ? 0ull : (w.rows - 1) * p + w.cols; }
// The rule for an entry of n plain bytes with element size k: a valid window, rows that do not run into each other, and an extent that
// does not wrap — asked with a division, no product is formed before it is known to fit.
ZPK_HD static inline bool place_valid(u64 n, u32 k, const Window& w, u64 p)
{
    if (p == 0 || !window_valid(n, k, w) || p < w.cols) return false;
    if (w.rows == 0 || w.cols == 0) return true;
    return w.rows - 1 == 0 || p <= (~0ull - w.cols) / (w.rows - 1);
}
// ---- the map ---------------------------------------------------------------------------------------------------------------------------
// For window byte d in [0, window_bytes):
//     o(d)      = (d / cols) * p + d % cols                                             the buffer byte
//     dst[o(d)] = src[plane_stored_index(n, k, window_plain_index(w, d))] ^ (base ? base[o(d)] : 0)
// The base is indexed by the same BUFFER byte: it is the caller's previous checkpoint in the merged layout.  The bytes of the extent in
// the gaps [cols, p) of every row are never written and never read from the base: they belong to the neighbouring shards.
ZPK_HD static inline u64 place_offset(const Window& w, u64 p, u64 d) { return (d / w.cols) * p + d % w.cols; }

// ---- the row table ---------------------------------------------------------------------------------------------------------------------
// WindowCopyRow's fields and the pitch.  src: the entry's stored bytes, n of them; dst, base: place_extent bytes each (base 0: none).
// A WORK ITEM is 16 KiB of the row's WINDOW bytes, len = window_bytes of them: window_piece as it is.
struct PlaceCopyRow { u64 src, dst, base, n, row_bytes, row0, col0, cols, len, item_base, pitch; u32 elem, pad; };
// Appends the row.  false: the table is full or the placement fails place_valid — nothing is written.  One of no bytes takes no row.
static inline bool place_copy_emit(u64 src, u64 dst, u64 base, u64 n, const Window& w, u64 pitch, u32 elem, PlaceCopyRow* rows, CopyPlan& p)
{
    if (!place_valid(n, elem, w, pitch)) return false;
    const u64 len = window_bytes(w);
    if (len == 0) return true;
    if (p.nrows >= ZPK_COPY_MAX_ROWS) return false;
    rows[p.nrows] = PlaceCopyRow{ src, dst, base, n, w.row_bytes, w.row0, w.col0, w.cols, len, p.items, pitch, elem, 0 };
    p.nrows++; p.items += copy_items(len);
    return true;
}
// the buffer byte of a place in an item (window_group_at, window_loose_at), all in 64 bits: the one statement of it, the kernel's and the
// host tests'.  With pitch == cols it is window_dst_of.
ZPK_HD static inline u64 place_dst_of(const WindowPiece& P, u64 pitch, WindowAt a) { return (P.r0 + (u64)a.row) * pitch + a.col; }

// ---- base and destination --------------------------------------------------------------------------------------------------------------
// base == dst EXACTLY is legal, by the argument of window_copy_plan.h carried over to the placed bytes: the items tile the window's index
// space, and o is one-to-one on it, so no two items touch the same buffer byte; an item reads the base at the very addresses it writes
// — base + o(d) against dst + o(d) —, so with base == dst no item writes what another reads; and inside an item a lane loads the base
// bytes of a step before it stores to the same addresses, lanes owning disjoint groups.  Any other overlap of the two ranges of
// place_extent bytes is refused: a base shifted against the destination by less than the extent could lie in the destination's placed
// bytes of another row.  (A base wholly inside the destination's GAPS would be harmless and is refused all the same: the rule stays
// two cases.)
static inline bool place_overlap_ok(u64 base, u64 dst, const Window& w, u64 p) { return delta_overlap_ok(base, dst, place_extent(w, p)); }

}  // namespace zpk
