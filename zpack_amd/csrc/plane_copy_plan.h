// plane_copy_plan.h — BYTE-PLANE entries: the plaintext of an entry whose elements are k bytes wide (k in {2, 4, 8}: a float tensor),
// stored with byte 0 of every element first, then byte 1 of every element, and so on.  The bytes of a float that compress (sign and
// exponent) then lie together and those that are noise (mantissa) lie together.  The transposition happens inside the copies that move
// the plaintext between the caller's device buffers and the codec's staging anyway (k_plane_copy, row_copy.hip, beside k_span_copy):
// SPLIT on the way in, JOIN on the way out.  Decided here, in one place: the layout, the row table the kernel reads, what an item of it
// covers, and which element sizes there are.  The 16 KiB item, the search and the launches: copy_rows_plan.h.
// Plain C++17, pj_types.h and standard headers only: tools/hostfuzz builds this file with g++ under ASan + UBSan (g++ knows no HIP),
// which keeps it so.  The index map is also device code (k_plane_copy): ZPK_HD is empty on a CPU build.
#pragma once
#include "copy_rows_plan.h"

namespace zpk {

// ---- the layout ------------------------------------------------------------------------------------------------------------------------
// An entry of n bytes with element size k, m = n / k (floor) whole elements:
//     stored[p * m + j] = plain[j * k + p]      0 <= p < k, 0 <= j < m          (plane p holds byte p of every element)
//     stored[k * m + t] = plain[k * m + t]      the n - k * m bytes of the tail, which stay where they are
// k = 1 is the identity.  The .zpk format knows nothing of this: the grouped bytes ARE the entry's plaintext, its XXH3 is over them, and
// the element size is an argument the caller hands to both sides.
ZPK_HD static inline bool plane_elem_valid(u32 k) { return k == 1 || k == 2 || k == 4 || k == 8; }
// where byte i of the plain side lies on the stored side
ZPK_HD static inline u64 plane_stored_index(u64 n, u32 k, u64 i)
{
    const u64 m = n / k;
    return i < m * k ? (i % k) * m + i / k : i;
}

// ---- the row table ---------------------------------------------------------------------------------------------------------------------
// A WORK ITEM is 16 KiB of a row's INTERLEAVED (plain) side, one wave's — the source of a split, the destination of a join —, so it is
// 16384 / k whole elements, a multiple of the 1024 a wave takes in one step, except in the last item of a row, which also owns the tail.
// A row of no bytes takes no row and no item.
enum : u32 { PLANE_SPLIT = 0, PLANE_JOIN = 1 };
struct PlaneCopyRow { u64 src, dst, len, item_base; u32 elem, join; };               // src, dst: device addresses; elem in {1, 2, 4, 8}
// Appends the row to the table.  false: the table is full (ZPK_COPY_MAX_ROWS) or the element size is none — nothing is written.
static inline bool plane_copy_emit(u64 src, u64 dst, u64 len, u32 elem, u32 join, PlaneCopyRow* rows, CopyPlan& p)
{
    if (!plane_elem_valid(elem)) return false;
    if (len == 0) return true;
    if (p.nrows >= ZPK_COPY_MAX_ROWS) return false;
    rows[p.nrows] = PlaneCopyRow{ src, dst, len, p.items, elem, join ? PLANE_JOIN : PLANE_SPLIT };
    p.nrows++; p.items += copy_items(len);
    return true;
}
// What item `piece` of a row of `len` bytes with element size k covers: the plain bytes [from, to), of which [from, wide_end) are whole
// groups of 16 elements — the kernel's wide path, 16 * k plain bytes against 16 bytes in each of the k planes — and [wide_end, to) go
// byte by byte (the elements that do not fill a group, and the tail).  from is a multiple of 16384, so of k and of 16 * k.
struct PlanePiece { u64 from, wide_end, to; };
ZPK_HD static inline PlanePiece plane_piece(u64 len, u32 k, u64 piece)
{
    PlanePiece P;
    P.from = piece * ZPK_COPY_PIECE;
    P.to = len - P.from < ZPK_COPY_PIECE ? len : P.from + ZPK_COPY_PIECE;
    const u64 m = len / k;
    const u64 e1 = P.to / k < m ? P.to / k : m;                                       // whole elements end here
    P.wide_end = P.from + ((e1 * k - P.from) / (16u * k)) * (16u * k);
    return P;
}

}  // namespace zpk
