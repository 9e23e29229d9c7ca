// delta_copy_plan.h — DELTA entries: a tensor stored as its XOR against a BASE in device memory (the previous checkpoint, which the caller
// holds anyway), grouped into byte planes.  Most weights of a float tensor do not change in a step and those that do change in their low
// mantissa bits, so `new XOR old` is mostly zero bytes, and after the split the high planes are almost all zero.  The XOR rides on the
// copy that carries the plaintext between the caller's device buffers and the codec's staging anyway (k_delta_copy, row_copy.hip, beside
// k_plane_copy): one more read stream, no further pass over the plaintext, no second copy of it.  Decided here, in one place: the layout
// and the row table the kernel reads.  The index map (plane_stored_index), what an item covers (plane_piece) and the element sizes
// (plane_elem_valid) are those of plane_copy_plan.h, the 16 KiB item, the search and the launches those of copy_rows_plan.h.
// Plain C++17 like that header: tools/hostfuzz builds this file with g++ under ASan + UBSan.
#pragma once
#include "plane_copy_plan.h"

namespace zpk {

// ---- the layout ------------------------------------------------------------------------------------------------------------------------
// An entry of n bytes with element size k in {1, 2, 4, 8} and a base of n bytes:
//     stored = split_k(plain XOR base)          plain = join_k(stored) XOR base
// split_k / join_k: the layout of plane_copy_plan.h, so with j = plane_stored_index(n, k, i):   stored[j] = plain[i] ^ base[i].
// The base is indexed by PLAIN byte index; the tail bytes are XORed like the rest; k = 1 is the bare XOR.  An entry without a base is a
// byte-plane entry (k_plane_copy's).  Neither the element size nor the base is in the archive: the caller hands both to both sides.
ZPK_HD static inline u8 delta_byte(u8 a, u8 base) { return (u8)(a ^ base); }

// ---- the row table ---------------------------------------------------------------------------------------------------------------------
// PlaneCopyRow with the base beside the two ends; items, item_base and the search are copy_rows_plan.h's.  SPLIT: src plain, dst stored.
// JOIN: src stored, dst plain.  The base lies beside the PLAIN side either way.
struct DeltaCopyRow { u64 src, dst, base, len, item_base; u32 elem, join; };
// Appends the row.  false: the table is full, the element size is none, or a row with bytes has no base — nothing is written.
static inline bool delta_copy_emit(u64 src, u64 dst, u64 base, u64 len, u32 elem, u32 join, DeltaCopyRow* rows, CopyPlan& p)
{
    if (!plane_elem_valid(elem)) return false;
    if (len == 0) return true;
    if (base == 0 || p.nrows >= ZPK_COPY_MAX_ROWS) return false;
    rows[p.nrows] = DeltaCopyRow{ src, dst, base, len, p.items, elem, join ? PLANE_JOIN : PLANE_SPLIT };
    p.nrows++; p.items += copy_items(len);
    return true;
}

// ---- base and destination ----------------------------------------------------------------------------------------------------------------
// JOIN with base == dst EXACTLY is legal (the buffer that holds the previous checkpoint becomes the new one): item t reads
// base[from, to) and writes dst[from, to), the same plain range; the items tile the plain side, so no item writes what another reads; and
// inside an item a lane loads the base bytes of its groups before it stores to the same addresses (pc_item, row_copy.h).  Any OTHER overlap of
// [base, base + len) with [dst, dst + len) is refused: an item would read base bytes that another item has written or not.
static inline bool delta_overlap_ok(u64 base, u64 dst, u64 len)
{
    if (len == 0 || base == dst) return true;
    return base < dst ? dst - base >= len : base - dst >= len;
}

}  // namespace zpk
