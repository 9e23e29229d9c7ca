// pj_types.h — the block tables of the block-parallel readers (lz4_pj.h, zstd_pj.h), as the host builds them (host_walk.h) and the
// kernels read them.  Plain C++: one definition each for the device code, the host code and the sanitizer harness (tools/hostfuzz).
#pragma once
#include <stdint.h>

namespace zpk {

typedef uint8_t  u8;                             // (the typedefs of zpk_device.h)
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int16_t  i16;
typedef int32_t  i32;
typedef int64_t  i64;

#define XS_GROUP 64u                             // xxh3_span.h: 1 KiB blocks per wave of the partial pass (the stream steps plan their hash sections in these groups: stream_plan.h)

#define PJ_BLOCK 65536u                         // LZ4F block size of the frames this path takes (BD = 0x40: what the reference writes)
struct PjBlock { u32 comp_off, comp_size /* bit 31: stored */, rec_base, out_size, out_off, nrec; };

#define ZPJ_BLOCK (128u << 10)
#define ZPJ_NONE 0xFFFFFFFFu
#define ZPJ_TREE_ONLY 3u                           // ZpjBlock::type of a stream step's first table entry: a block of an earlier step, here only for its Huffman tree
struct ZpjBlock {
    u32 hdr_off;             // offset of the 3-byte block header in the compressed entry
    u32 size;                // Block_Size (Compressed / Raw: bytes of content; RLE: the regenerated size)
    u32 type;                // 0 Raw, 1 RLE, 2 Compressed
    u32 lit_type;            // Compressed: 0 Raw, 1 RLE, 2 Compressed, 3 Treeless
    u32 lit_size;            // ... regenerated literal bytes
    u32 lit_used;            // ... bytes of the block the literals section takes
    u32 lit_ref;             // ... reference of literal byte 0: offset in [compressed entry | literal arena]; RLE literals: the byte's offset
    u32 lit_base;            // ... decoded literals: their offset in the literal arena
    u32 tree_src;            // ... Treeless: the block whose tree description it uses
    u32 nseq;                // ... sequences
    u32 seq_base;            // ... index of its first sequence record (a block owns nseq + 1 slots: the last one stands for the trailing literals)
    u32 rep_in[3];           // device (k_zpj_reps): repeat offsets at the block's start
    u32 tab_off[3];          // ... a Repeat_Mode table (LL, OF, ML): where the table it inherits is described (offset in the compressed entry)
    u32 tab_modes;           // ... and how: 2 bits per kind (0 predefined, 1 RLE, 2 FSE description, 3 nowhere)
};

}  // namespace zpk
