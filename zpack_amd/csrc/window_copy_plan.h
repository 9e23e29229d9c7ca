// window_copy_plan.h — WINDOW reads: a 2-D sub-block of an entry, seen as a matrix of rows x row_bytes, delivered densely into a
// destination of window size.  A reader that owns part of every tensor (a tensor-parallel rank, a pipeline stage) otherwise needs a
// full-size scratch tensor per entry and a second pass over the plaintext to cut its part out; every device read already moves each
// plaintext byte once, from the codec's staging to the caller's buffer, and the cut rides on that copy (k_window_copy, row_copy.hip,
// beside k_plane_copy and k_delta_copy).  The byte planes are joined and the base is XORed on the way.  Decided here, in one place: the
// window, the rule it has to pass, the map, the row table the kernel reads and what an item of it covers.  The index map of the stored
// side (plane_stored_index) and the element sizes (plane_elem_valid) are those of plane_copy_plan.h, the 16 KiB item, the search and the
// launches those of copy_rows_plan.h, the overlap rule is delta_copy_plan.h's, and none is restated.
// Plain C++17 like those headers: tools/hostfuzz builds this file with g++ under ASan + UBSan.
#pragma once
#include "delta_copy_plan.h"

namespace zpk {

// ---- the window ------------------------------------------------------------------------------------------------------------------------
// All in bytes.  row_bytes == 0: no window, the entry whole.  A slice [start, stop) along ONE dimension `dim` of a contiguous tensor of
// `shape` and `itemsize` is the window  row_bytes = shape[dim] * inner, row0 = 0, rows = prod(shape[:dim]), col0 = start * inner,
// cols = (stop - start) * inner  with inner = prod(shape[dim + 1:]) * itemsize.
struct Window { u64 row_bytes, row0, rows, col0, cols; };
// The rule for an entry of n plain bytes with element size k: whole rows of whole elements, the block inside the matrix, and no sum or
// product that wraps (differences only; rows * cols <= n follows).  A windowed entry has no tail: n is a multiple of row_bytes, so of k.
ZPK_HD static inline bool window_valid(u64 n, u32 k, const Window& w)
{
    if (!plane_elem_valid(k) || w.row_bytes == 0 || n % w.row_bytes) return false;
    if (w.row_bytes % k || w.col0 % k || w.cols % k) return false;
    if (w.col0 > w.row_bytes || w.cols > w.row_bytes - w.col0) return false;
    const u64 nrows = n / w.row_bytes;
    return w.row0 <= nrows && w.rows <= nrows - w.row0;
}
// bytes delivered; 0 is a legal window that delivers nothing
ZPK_HD static inline u64 window_bytes(const Window& w) { return w.rows * w.cols; }
// ---- the map ---------------------------------------------------------------------------------------------------------------------------
// For destination byte d in [0, window_bytes):
//     i(d)   = (row0 + d / cols) * row_bytes + col0 + d % cols                        the plain index
//     dst[d] = src[plane_stored_index(n, k, i(d))] ^ (base ? base[d] : 0)
// The base is indexed by DESTINATION byte: the caller holds its own shard of the previous checkpoint, of window size.
ZPK_HD static inline u64 window_plain_index(const Window& w, u64 d) { return (w.row0 + d / w.cols) * w.row_bytes + w.col0 + d % w.cols; }

// ---- the row table ---------------------------------------------------------------------------------------------------------------------
// src: the entry's stored bytes, n of them; dst, base: len = window_bytes bytes each (base 0: none).  A WORK ITEM is 16 KiB of the row's
// DESTINATION; items, item_base and the search are copy_rows_plan.h's.
struct WindowCopyRow { u64 src, dst, base, n, row_bytes, row0, col0, cols, len, item_base; u32 elem, pad; };
// Appends the row.  false: the table is full or the window fails window_valid — nothing is written.  A window of no bytes takes no row.
static inline bool window_copy_emit(u64 src, u64 dst, u64 base, u64 n, const Window& w, u32 elem, WindowCopyRow* rows, CopyPlan& p)
{
    if (!window_valid(n, elem, w)) return false;
    const u64 len = window_bytes(w);
    if (len == 0) return true;
    if (p.nrows >= ZPK_COPY_MAX_ROWS) return false;
    rows[p.nrows] = WindowCopyRow{ src, dst, base, n, w.row_bytes, w.row0, w.col0, w.cols, len, p.items, elem, 0 };
    p.nrows++; p.items += copy_items(len);
    return true;
}

// ---- what an item covers ---------------------------------------------------------------------------------------------------------------
// Item `piece` covers the destination bytes [from, to).  The window rows cut that range into SEGMENTS: the rest of the window row that
// `from` lies in (seg0 bytes from column c0 of window row r0), then nfull whole window rows of cols bytes, then the first `last` bytes
// of one more.  from is a multiple of 16384 and cols of k, so every segment begins on an element.  Inside a segment the whole groups of
// 16 elements, counted from the segment's start, take the wide path — 16 * k destination bytes against 16 bytes in each plane —, and
// what does not fill a group at its end goes byte by byte through the map.  Groups and loose bytes are numbered through the WHOLE item,
// segment after segment, so that the lanes are dealt over all of them: a window of 128-byte rows keeps every lane busy.
struct WindowPiece {
    u64 from, to, r0, c0, seg0;
    u32 nfull, last;                             // whole window rows behind the first segment, bytes of the one behind them
    u32 g0, gpr, glast, groups;                  // groups of the first segment, of a whole window row, of the last segment; all of them
    u32 l0, lpr, llast, loose;                   // the loose bytes, likewise
};
ZPK_HD static inline WindowPiece window_piece(u64 len, u64 cols, u32 k, u64 piece)
{
    WindowPiece P;
    const u32 gb = 16u * k;
    P.from = piece * ZPK_COPY_PIECE;
    P.to = len - P.from < ZPK_COPY_PIECE ? len : P.from + ZPK_COPY_PIECE;
    P.r0 = P.from / cols; P.c0 = P.from % cols;
    const u64 span = P.to - P.from;
    P.seg0 = cols - P.c0 < span ? cols - P.c0 : span;
    const u64 rest = span - P.seg0;                                                   // < 16384: the counts below fit 32 bits
    P.nfull = (u32)(rest / cols); P.last = (u32)(rest % cols);
    P.g0 = (u32)(P.seg0 / gb); P.l0 = (u32)(P.seg0 % gb);
    P.gpr = P.nfull ? (u32)(cols / gb) : 0u; P.lpr = P.nfull ? (u32)(cols % gb) : 0u;
    P.glast = P.last / gb; P.llast = P.last % gb;
    P.groups = P.g0 + P.nfull * P.gpr + P.glast;
    P.loose = P.l0 + P.nfull * P.lpr + P.llast;
    return P;
}
// Where a group or a loose byte of the item lies: window row r0 + row of the destination, byte `col` of that row's `cols`.
struct WindowAt { u32 row; u64 col; };
// group G in [0, P.groups): its first byte
ZPK_HD static inline WindowAt window_group_at(const WindowPiece& P, u32 k, u32 G)
{
    const u32 gb = 16u * k;
    if (G < P.g0) return WindowAt{ 0u, P.c0 + (u64)G * gb };
    const u32 g = G - P.g0;
    if (g < P.nfull * P.gpr) return WindowAt{ 1u + g / P.gpr, (u64)(g % P.gpr) * gb };
    return WindowAt{ 1u + P.nfull, (u64)(g - P.nfull * P.gpr) * gb };
}
// loose byte B in [0, P.loose)
ZPK_HD static inline WindowAt window_loose_at(const WindowPiece& P, u32 k, u32 B)
{
    const u32 gb = 16u * k;
    if (B < P.l0) return WindowAt{ 0u, P.c0 + (u64)P.g0 * gb + B };
    const u32 b = B - P.l0;
    if (b < P.nfull * P.lpr) return WindowAt{ 1u + b / P.lpr, (u64)P.gpr * gb + b % P.lpr };
    return WindowAt{ 1u + P.nfull, (u64)P.glast * gb + (b - P.nfull * P.lpr) };
}
// the destination byte of a place, and its plain index in the entry (the map above, with d / cols and d % cols known)
ZPK_HD static inline u64 window_dst_of(const WindowPiece& P, u64 cols, WindowAt a) { return (P.r0 + a.row) * cols + a.col; }
ZPK_HD static inline u64 window_plain_of(const WindowPiece& P, u64 row_bytes, u64 row0, u64 col0, WindowAt a) { return (row0 + P.r0 + a.row) * row_bytes + col0 + a.col; }

// ---- base and destination --------------------------------------------------------------------------------------------------------------
// base == dst EXACTLY is legal, by the argument of delta_copy_plan.h over the window's bytes: item t reads base[from, to) and writes
// dst[from, to), the items tile the destination, and a lane loads the base bytes of a step before it stores to the same addresses.
static inline bool window_overlap_ok(u64 base, u64 dst, const Window& w) { return delta_overlap_ok(base, dst, window_bytes(w)); }

}  // namespace zpk
