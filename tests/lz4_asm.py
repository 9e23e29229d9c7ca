"""Hand-built LZ4 frames: the assembler (Block, Frame) and the case table of the block-parallel reader (zpack_amd/csrc/lz4_pj.h and its
host half decode_big_lz4_single / pj_finish in zpk_codec.hip).  Plain Python: nothing here needs a GPU, the library or liblz4.  Not a
test module.  tests/test_lz4_asm_cpu.py asks liblz4, the oracle and the compiled reference what every frame is and checks that each
frame sits where its label says; tests/test_gpu_lz4_asm_reader.py runs the device paths against that record.

A case is a dict:
  label, group   what it is for; the group letter is the part of the reader it aims at (A routing, B block sizes and offsets,
                 C sequences in a block, D matches, E chunks, F short outputs, G damage, L liblz4's end-of-block rule: CPU only)
  frame          the bytes of the archive entry (comp_size = len(frame))
  uncomp, cap    the entry's stated size and the capacity of its buffer
  hash_of        None: the entry's hash is the XXH3 of what the judges decode; a label: the XXH3 of THAT case's bytes (a damaged
                 copy keeps the hash of the intact frame)
  walk, nblocks  walk_lz4_single_to (zpack_amd/csrc/host_walk.h) accepts the frame, and the blocks it then counts (0 when it declines).
                 The rule, restated: magic 0x184D2204; FLG version 01 and none of the bits 0x17 (block checksum, content checksum,
                 reserved, dictionary id); BD 0x40; a header checksum byte that is right; a content size, where present, equal to the
                 entry's stated size; then block words until the EndMark, each 1 .. 65536 bytes (stored or not) and inside the entry;
                 nothing behind the EndMark; at least 4 blocks.  Set by the builders from how a frame was made, never by running the
                 walker; test_lz4_asm_cpu.py checks it against a Python restatement of the walker.
  reader         walk, and everything about the frame is regular (every block decodes, to at most 65536 bytes; no offset reaches in
                 front of the frame, or of its block in an independent frame; the sizes add up to `uncomp`): the reader must FINISH it.
  claims         what the label says about the geometry, checked from the frame itself by the block walker of test_lz4_asm_cpu.py

liblz4's input rule (measured with liblz4 1.9.3 through the reference's call loop): a block is refused when the literals of a sequence
that carries a match end less than 8 bytes before the block's end, and when the extension bytes of a match length end less than 5
bytes before it.  So `match, 00` — an empty last sequence behind a match — is refused whatever the match length: without extension
bytes by the first half, with them by the second.  The one empty last sequence liblz4 takes is the one-byte block 00 (group B).
Every frame of groups A to G stays inside the rule (the table asserts it of every block it builds); group L sits on both sides."""
import importlib.util
import os
import struct

import numpy as np

BLOCK_MAX = 65536
CHUNK_BLOCKS = 512                    # ZPK_PJ_CHUNK_BLOCKS (zpk_codec.hip)
MAX_CHUNKS = 64                       # ZPK_PJ_MAX_CHUNKS
MIN_BLOCKS = 4                        # ZPK_PJ_MIN_BLOCKS (host_walk.h)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    """tools/sim/lz4_asm_share.py: the CPU model of the one-wave decoder's chunking and of its assembly rule"""
    spec = importlib.util.spec_from_file_location("lz4_asm_share", os.path.join(ROOT, "tools", "sim", "lz4_asm_share.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


M = _model()


def xxh32(data, seed=0):
    """XXH32 (xxHash specification) of a short input: the header checksum of a frame, a block checksum"""
    P1, P2, P3, P4, P5, M = 2654435761, 2246822519, 3266489917, 668265263, 374761393, 0xFFFFFFFF        # (M: the 32-bit mask, here only)
    rot = lambda v, r: ((v << r) | (v >> (32 - r))) & M
    n, i = len(data), 0
    if n >= 16:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed & M, (seed - P1) & M]
        while i + 16 <= n:
            for k in range(4):
                v[k] = (rot((v[k] + struct.unpack_from("<I", data, i + 4 * k)[0] * P2) & M, 13) * P1) & M
            i += 16
        h = (rot(v[0], 1) + rot(v[1], 7) + rot(v[2], 12) + rot(v[3], 18)) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while i + 4 <= n:
        h = (rot((h + struct.unpack_from("<I", data, i)[0] * P3) & M, 17) * P4) & M
        i += 4
    while i < n:
        h = (rot((h + data[i] * P5) & M, 11) * P1) & M
        i += 1
    h ^= h >> 15; h = (h * P2) & M; h ^= h >> 13; h = (h * P3) & M; h ^= h >> 16
    return h


class Block:
    """one LZ4 block written sequence by sequence; only the LENGTH of the output is tracked (the judges supply the bytes)"""

    def __init__(self, seed, history=0):
        self.rng = np.random.default_rng(seed)
        self.d = bytearray()
        self.n = 0                    # output bytes of this block so far
        self.hist = history           # output bytes a match may reach in front of the block (linked blocks)
        self.off_pos = []             # block position of every offset field
        self.lit_end = []             # block position behind the literals of every sequence that carries a match
        self.ext_end = []             # block position behind the extension bytes of every match length that has some
        self.starts = []              # output position (in the block) at which every sequence that has bytes begins
        self.tail_pos = None          # block position of the last sequence's token
        self.nseq = 0

    def seq(self, ll, ml, off=None, lit=None, check=True):
        """lit: the literal bytes (default: random); check=False lets an offset reach in front of everything (an irregular frame)"""
        assert ml >= 4
        if off is None:               # a plain match somewhere in what exists, mostly near (so that batches depend on themselves)
            have = self.n + ll + self.hist
            off = int(self.rng.integers(ml, max(ml + 1, min(have, 300) + 1)))
            off = min(off, have)
        assert not check or 1 <= off <= self.n + ll + self.hist, (off, self.n, ll)
        self.d.append((min(ll, 15) << 4) | min(ml - 4, 15))
        self._ext(ll)
        self._lits(ll, lit)
        self.lit_end.append(len(self.d))
        self.off_pos.append(len(self.d))
        self.d += struct.pack("<H", off)
        self._ext(ml - 4)
        if ml - 4 >= 15:
            self.ext_end.append(len(self.d))
        self.starts.append(self.n)
        self.n += ll + ml
        self.nseq += 1
        return self

    def _lits(self, ll, lit):
        if lit is None:
            lit = self.rng.integers(0, 256, ll, dtype=np.uint8).tobytes()
        assert len(lit) == ll
        self.d += lit

    def _ext(self, v):
        if v >= 15:
            v -= 15
            while v >= 255:
                self.d.append(255); v -= 255
            self.d.append(v)

    def fill(self, count, ll=(0, 6), ml=(4, 10)):
        for _ in range(count):
            self.seq(int(self.rng.integers(ll[0], ll[1] + 1)), int(self.rng.integers(ml[0], ml[1] + 1)))
        return self

    def run(self):
        """a long byte run: the entry then compresses below 1/8 and k_classify routes it to k_lz4_left"""
        self.seq(1, 9 * (len(self.d) + 40), 1)
        return self

    def done(self, tail=16, lit=None):
        """the last sequence: `tail` literals and no match (tail = 0: the token 00)"""
        self.tail_pos = len(self.d)
        self.d.append(min(tail, 15) << 4)
        self._ext(tail)
        self._lits(tail, lit)
        if tail:
            self.starts.append(self.n)
        self.n += tail
        self.nseq += 1
        self.data = bytes(self.d)
        return self.data

    def in_rule(self):
        """liblz4 takes the block (the module's docstring; the case table asserts it of every block of groups A to G)"""
        return all(len(self.d) - p >= 8 for p in self.lit_end) and all(len(self.d) - p >= 5 for p in self.ext_end)


def literals(n, seed=0, lit=None):
    """a block of n literals and nothing else (n = 0: the one-byte block 00) -> a finished Block"""
    b = Block(seed)
    b.done(n, lit)
    return b


class Frame:
    """One frame, block by block.  block() hands out a Block that knows the history it may reach; add() takes a finished Block,
    stored() a stored block.  flg: bits to set beyond the version (0x20 independent, 0x10 block checksums, 0x08 content size — set by
    content_size —, 0x04 content checksum, 0x01 dictionary id: none of the optional fields but the block checksums is written)."""

    def __init__(self, linked=True, content_size=None, flg=0, bd=0x40):
        self.linked, self.content_size, self.flg, self.bd = linked, content_size, flg, bd
        self.blocks = []              # (word, payload, output bytes, the Block or None)
        self.out = 0

    def block(self, seed):
        return Block(seed, self.out if self.linked else 0)

    def add(self, b, out=None):
        """b: a finished Block, or the bytes of one with its output length"""
        data = b.data if isinstance(b, Block) else bytes(b)
        n = b.n if isinstance(b, Block) else out
        self.blocks.append((len(data), data, n, b if isinstance(b, Block) else None))
        self.out += n
        return self

    def lits(self, n, seed=0, lit=None):
        return self.add(literals(n, seed + 7919 * len(self.blocks), lit))

    def stored(self, data):
        self.blocks.append((len(data) | 0x80000000, bytes(data), len(data), None))
        self.out += len(data)
        return self

    def raw_word(self, word, payload=b""):
        """any block word with any bytes behind it (routing cases)"""
        self.blocks.append((word, bytes(payload), 0, None))
        return self

    def header(self):
        flg = 0x40 | (0 if self.linked else 0x20) | self.flg | (0x08 if self.content_size is not None else 0)
        desc = bytes([flg, self.bd]) + (struct.pack("<Q", self.content_size) if self.content_size is not None else b"")
        return b"\x04\x22\x4d\x18" + desc + bytes([(xxh32(desc) >> 8) & 0xFF])

    def build(self, behind=b""):
        """-> the frame; self.at = frame position of every block's payload"""
        f = bytearray(self.header())
        self.at = []
        for word, data, n, b in self.blocks:
            f += struct.pack("<I", word)
            self.at.append(len(f))
            f += data
            if self.flg & 0x10:
                f += struct.pack("<I", xxh32(data))
        f += struct.pack("<I", 0)
        return bytes(f) + behind

    def offsets(self):
        """frame position of every offset field (after build)"""
        return [a + p for a, (w, d, n, b) in zip(self.at, self.blocks) if b is not None for p in b.off_pos]

    def tokens(self):
        """frame position of every compressed block's last token (after build)"""
        return [a + b.tail_pos for a, (w, d, n, b) in zip(self.at, self.blocks) if b is not None]


def _frame(blocks, linked=False):
    """blocks: [("c" | "s", bytes)] -> (frame, frame position of every block's payload)"""
    f = Frame(linked)
    for kind, data in blocks:
        if kind == "s": f.stored(data)
        else: f.add(data, 0)
    return f.build(), f.at


# ---- the case table ---------------------------------------------------------------------------------------------------------------------

_CASES = []


def __getattr__(name):
    """CASES is built when it is first asked for (group C wraps the blocks of tests/lz4_overlap_blocks.py, which imports this module)"""
    if name == "CASES":
        if not _CASES:
            for g in (_group_a, _group_b, _group_c, _group_d, _group_e, _group_f, _group_g, _group_l):
                g()
        return _CASES
    raise AttributeError(name)


def _add(group, label, F, walk=True, reader=None, frame=None, uncomp=None, cap=None, hash_of=None, **claims):
    frame = F.build() if frame is None else frame
    reader = walk if reader is None else reader
    assert walk or not reader
    assert group == "L" or all(b.in_rule() for w, d, n, b in F.blocks if b is not None), (label, "liblz4 refuses a block of this frame")
    uncomp = F.out if uncomp is None else uncomp
    c = dict(label="%s: %s" % (group, label), group=group, frame=frame, uncomp=uncomp, cap=uncomp if cap is None else cap, hash_of=hash_of,
             walk=walk, reader=reader, nblocks=len(F.blocks) if walk else 0, independent=not F.linked, claims=claims, F=F)
    assert all(c["label"] != x["label"] for x in _CASES), label
    _CASES.append(c)
    return c


def sized(F, n, seed):
    """a block of F that decodes to n bytes: literals alone below 24 bytes, else 4 literals, one match at offset 1 to 4, 5 literals"""
    if n < 24:
        return F.lits(n, seed)
    b = F.block(seed)
    b.seq(4, n - 9, 1 + seed % 4)
    b.done(5)
    return F.add(b)


def _small(F, seed=1, count=4):
    for k in range(count):
        F.lits(9 + 4 * k, seed + k)
    return F


def _group_a():
    _add("A", "3 blocks", _small(Frame(), count=3), walk=False)
    _add("A", "4 blocks", _small(Frame()))
    _add("A", "a content size that is right", _small(Frame(content_size=9 + 13 + 17 + 21)))
    _add("A", "a content size that is wrong", _small(Frame(content_size=9 + 13 + 17 + 21 + 1)), walk=False)
    _add("A", "independent blocks", _small(Frame(linked=False)))
    _add("A", "BD 0x50", _small(Frame(bd=0x50)), walk=False)
    _add("A", "block checksums", _small(Frame(flg=0x10)), walk=False)
    F = _small(Frame())
    _add("A", "bytes behind the EndMark", F, walk=False, frame=F.build(behind=b"\x01\x02\x03"))
    F = _small(Frame(), count=2)
    F.raw_word(0x80000000 | 65537, bytes(65537))
    _small(F, 5, 2)
    _add("A", "a block word above 65536", F, walk=False, uncomp=9 + 13 + 65537 + 9 + 13)
    F = _small(Frame(), count=2)
    F.raw_word(0x80000000)
    _small(F, 5, 2)
    _add("A", "a stored block word of length 0", F, walk=False)
    F = _small(Frame())
    _add("A", "the entry cut inside a block", F, walk=False, frame=F.build()[:-10])


B_SIZES = (31, 1, 1, 0, 2, 3, 5, 31, 32, 33, 255, 256, 257, 65535, 65536, 7)      # block k + 1 begins where these add up to


def _unequal(F, count, seed):
    """`count` blocks of unequal sizes, every third with a match into the block before"""
    for i in range(count):
        n = 1 + (i * 7 + seed) % 23
        if i % 3 == 2:
            b = F.block(seed + i)
            b.seq(2, 6, 3 + i % 9).done(5)
            F.add(b)
        else:
            F.lits(n, seed + i)
    return F


def _group_b():
    F = Frame()
    for k, n in enumerate(B_SIZES):
        sized(F, n, 100 + k)
    _add("B", "mid-frame blocks of 0 .. 65536 bytes at every residue", F, sizes=list(B_SIZES), residues4=[0, 1, 2, 3], residues32=[31, 0, 1])
    for count in (64, 65, 128, 129):
        _add("B", "%d blocks of unequal sizes" % count, _unequal(Frame(), count, count), blocks=count)
    F = _small(Frame(), count=2)
    b = F.block(140)
    b.seq(4, 65528, 1).done(5)
    F.add(b)
    _small(F, 5, 2)
    _add("B", "a block that decodes to 65537 bytes", F, reader=False, sizes=[9, 13, 65537, 9, 13])


def _wrapped(data, n, seed=3):
    """a finished block (its matches stay inside it) unchanged as block 2 of a linked four-block frame"""
    F = Frame()
    F.lits(20, seed).lits(9, seed)
    F.add(data, n) if not isinstance(data, Block) else F.add(data)
    return F.lits(7, seed)


def _starts_block(seed, starts, total):
    """sequences that begin at the given output positions of the block (the first at 0), the last one literals up to `total`"""
    b = Block(seed)
    at = 0
    for nxt in starts[1:]:
        b.seq(3, nxt - at - 3, 1 + (seed + at) % 3)
        at = nxt
    b.done(total - at)
    return b


def _count_block(seed, nseq):
    b = Block(seed)
    for i in range(nseq - 1):
        b.seq(1 + i % 3, 4 + i % 5)
    b.done(6)
    return b


def _dense(F, seed):
    b = F.block(seed)
    for i in range(16382):
        b.seq(0, 4, 1 + (i * 5 + seed) % 11)
    b.done(8)
    assert b.n == BLOCK_MAX
    return F.add(b)


def _group_c():
    a = _starts_block(201, [0, 31, 64, 255, 8191], 8300)
    _add("C", "sequences that start at bit 31, bit 0, position 255 and 8191", _wrapped(a, a.n), block=2, starts=[31, 64, 255, 8191])
    a = _starts_block(202, [0, 32, 256, 8192], 8300)
    _add("C", "sequences that start at bit 32 (bit 0 of word 1), position 256 and 8192", _wrapped(a, a.n), block=2, starts=[32, 256, 8192])
    for nseq in (1, 63, 64, 65, 128, 575, 576, 577):
        _add("C", "%d sequences in a block" % nseq, _wrapped(_count_block(210 + nseq, nseq), 0), block=2, nseq=nseq)
    F = Frame()
    F.lits(20, 3)
    _dense(F, 221)
    _dense(F, 222)
    F.lits(7, 3)
    _add("C", "the densest block twice: ll = 0, ml = 4 up to 65536 bytes", F, dense=[1, 2])
    b = literals(65279, 230)
    assert len(b.data) == BLOCK_MAX
    _add("C", "the longest literal run of a block of 65536 compressed bytes", _wrapped(b, 0), block=2, comp=BLOCK_MAX, last_lit_pos=257)
    b = Block(231)
    b.seq(65271, 4, 9).done(5)
    assert len(b.data) == BLOCK_MAX
    _add("C", "a literal run of 65271 bytes, the last literals at 65531", _wrapped(b, 0), block=2, comp=BLOCK_MAX, last_lit_pos=65531)
    from tests import lz4_overlap_blocks as blocks
    for left in (False, True):
        for k, x in enumerate(blocks.all_blocks(left)):
            _add("C", "wrapped %s%s" % ("left: " if left else "", x["label"]), _wrapped(x["data"], x["blk"].n, k), block=2)


def _group_d():
    F = Frame()
    b = F.block(301); b.seq(8, 6, 8).done(6); F.add(b)
    F.lits(11, 1).lits(5, 2)
    b = F.block(302); b.seq(3, 9, F.out + 3).done(5); F.add(b)
    _add("D", "an offset equal to the whole history, from block 0 and from block 3", F, reach0=[0, 3])
    for k in (0, 3):
        F = Frame()
        b = F.block(303); b.seq(8, 6, 8 + (k == 0), check=False).done(6); F.add(b)
        F.lits(11, 1).lits(5, 2)
        b = F.block(304); b.seq(3, 9, F.out + 3 + (k == 3), check=False).done(5); F.add(b)
        _add("D", "an offset one beyond the whole history, from block %d" % k, F, reader=False, beyond=k)
    F = Frame()
    F.lits(30, 1).lits(10, 2).lits(10, 3).lits(10, 4)
    sized(F, 65499, 305)
    b = F.block(306); b.seq(4, 40, 65535).done(5); F.add(b)
    _add("D", "offset 65535 whose source lies across three small blocks", F, far=(5, 65535))
    for extra in (0, 1):
        F = _small(Frame(linked=False), count=2)
        b = F.block(307); b.seq(6, 5, 6 + extra, check=False).done(5); F.add(b)
        _small(F, 5, 2)
        _add("D", "independent blocks: an offset equal to the position in the block" + (" plus one" if extra else ""), F, reader=not extra,
             block=2, offset=6 + extra)
    F = Frame()
    for off in range(1, 17):
        b = F.block(310 + off); b.seq(16, 65500, off).done(5); F.add(b)
    _add("D", "offsets 1 to 16 with matches of 65500 bytes", F, offsets=list(range(1, 17)))
    F = Frame()
    F.lits(20, 320)
    for i in range(299):
        b = F.block(321 + i); b.seq(0, 15, 20).done(5); F.add(b)
    _add("D", "300 blocks, each a copy of the one before", F, blocks=300)
    F = Frame()
    F.lits(9, 1).stored(bytes(range(40, 73)))
    b = F.block(330); b.seq(2, 20, 30).done(5); F.add(b)
    b = F.block(331); b.seq(1, 60, 61).done(7); F.add(b)
    F.stored(bytes(range(5)))
    _add("D", "matches into a stored block", F, stored=[1, 4])
    F = Frame()
    F.lits(12, 1).lits(9, 2)
    b = F.block(332); b.seq(6, 20, 10).done(5); F.add(b)
    F.lits(7, 3)
    _add("D", "a match whose source straddles the block boundary and the seam behind its literals", F, block=2, offset=10)


def _chunked(count, residues, seed):
    """`count` blocks of 5 to 40 bytes; block 512 k begins at a byte offset of residues[k - 1] mod 4 with an offset-1 match, then a match
    whose source lies on both sides of the boundary; every other block copies from the block before it"""
    F = Frame()
    prev = 0
    for i in range(count):
        nxt = i + 1
        if i == 0:
            b = literals(20, seed)
        elif i % CHUNK_BLOCKS == 0:
            b = F.block(seed + i); b.seq(0, 5, 1).seq(0, 6, 8).done(5)
        else:
            ll = 1
            if nxt % CHUNK_BLOCKS == 0 and nxt < count:          # the block in front of a boundary: its literals put the boundary on its residue
                ll = 1 + (residues[nxt // CHUNK_BLOCKS - 1] - (F.out + 1 + 4 + i % 20 + 5)) % 4
            b = F.block(seed + i); b.seq(ll, 4 + i % 20, prev).done(5)
        F.add(b)
        assert 5 <= b.n <= 40
        prev = b.n
    return F


def _group_e():
    for count, res in ((513, [1]), (1024, [2]), (1025, [3, 1]), (1537, [1, 2, 3])):
        _add("E", "%d blocks of 5 to 40 bytes" % count, _chunked(count, res, 400 + count), blocks=count, boundaries4=res)
    F = Frame()
    for i in range(520):
        if i == 0:
            F.lits(129, 450)
        else:
            b = F.block(450 + i); b.seq(3, 121, 129).done(5); F.add(b)
    _add("E", "512 blocks of 129 bytes and 8 more: a hash section of one group in front of the last", F, blocks=520, boundary=66048)
    F = Frame()
    data = np.random.default_rng(460).integers(0, 256, 32769, dtype=np.uint8).tobytes()
    for i in range(32769):
        F.stored(data[i:i + 1])
    _add("E", "32769 stored blocks of one byte: chunks of 513 blocks", F, blocks=32769, chunk_blocks=513)
    F = Frame()
    for i in range(520):
        b = F.block(470 + i); b.seq(8, 33779, 1 + i % 8).done(5); F.add(b)
    _add("E", "520 blocks of 33 KiB", F, blocks=520, out=17571840, big=True)


F_SIZES = (1, 3, 4, 8, 9, 16, 17, 63, 64, 65, 128, 129, 240, 241, 242, 1023, 1024, 1025, 1026)


def _group_f():
    for n in F_SIZES:
        F = Frame()
        for k, part in enumerate((n // 4, n // 4, n // 4, n - 3 * (n // 4))):        # (the last block is never empty: group L says why)
            sized(F, part, 500 + n + k)
        _add("F", "four blocks that decode to %d bytes" % n, F, out=n)


DAMAGE = ("an offset set to 0", "a literal length that runs out of the block", "the entry one byte short", "the capacity one byte short")
DAMAGED = ("D: 300 blocks, each a copy of the one before", "D: matches into a stored block", "E: 513 blocks of 5 to 40 bytes")


def _group_g():
    for base in DAMAGED:
        c = [x for x in _CASES if x["label"] == base][0]
        F = c["F"]
        for dmg in DAMAGE:
            f = bytearray(c["frame"])
            uncomp, cap = c["uncomp"], c["cap"]
            if dmg == DAMAGE[0]:
                p = F.offsets()[len(F.offsets()) // 2]
                f[p:p + 2] = b"\0\0"
            elif dmg == DAMAGE[1]:
                toks = [p for p in F.tokens() if f[p] >> 4 < 14]               # (a length without extension bytes: one more than are there)
                p = toks[len(toks) // 2]
                f[p] += 0x10
            elif dmg == DAMAGE[2]:
                uncomp, cap = uncomp - 1, cap - 1
            else:
                cap -= 1
            # (liblz4 1.9.3 does not look at an offset of 0: it copies from the output position itself and the entry ends as a hash
            # mismatch, 15, where the oracle and the device decoders say DECOMPRESS_FAILED, 13: pinned by test_lz4_asm_cpu.py)
            claims = dict(liblz4_status=15) if dmg == DAMAGE[0] else {}
            _add("G", "%s: %s" % (dmg, base), F, reader=False, frame=bytes(f), uncomp=uncomp, cap=cap, hash_of=base, **claims)


def _group_l():
    def one(label, build, liblz4, last=False):
        F = Frame()
        F.lits(20, 3).lits(9, 3)
        b = F.block(600 + len(_CASES))
        build(b)
        if last:
            F.lits(7, 3).add(b)
        else:
            F.add(b).lits(7, 3)
        _add("L", label, F, liblz4=liblz4)
    for tail in (1, 4, 5):
        one("%d literals behind the last match" % tail, lambda b, t=tail: b.seq(3, 8, 5).done(t), tail >= 5)
    one("match, 00 with a short match length", lambda b: b.seq(3, 8, 5).done(0), False)
    one("match, 00 with four extension bytes", lambda b: b.seq(3, 1038, 5).done(0), False)
    one("match, 00 with five extension bytes", lambda b: b.seq(3, 1039, 5).done(0), False)
    one("a match length with extension bytes that end 2 bytes before the block's end", lambda b: b.seq(3, 1038, 5).done(1), False)
    one("a match length with an extension byte that ends 5 bytes before the block's end", lambda b: b.seq(3, 19, 5).done(4), True)
    one("the frame's last block ends 4 literals behind a match", lambda b: b.seq(3, 8, 5).done(4), False, last=True)
    one("the frame's last block ends 5 literals behind a match", lambda b: b.seq(3, 8, 5).done(5), True, last=True)
    # the path dependence: the literals of the second sequence end 7 bytes before the block's end, but a run of 10 to 14 literals with
    # room in the output goes through liblz4's shortcut, which does not look
    one("12 literals inside the zone, taken by the shortcut", lambda b: b.seq(3, 8, 5).seq(12, 4, 6).done(4), True)
    one("9 literals inside the zone", lambda b: b.seq(3, 8, 5).seq(9, 4, 6).done(4), False)
    # not the block rule but the call loop's: an empty block behind the last output byte is reached only with room left in the buffer
    # (lib/zpack_read.c:414 stops when the buffer is full, and the frame is then not at its end): BUFFER_TOO_SMALL at the exact capacity
    F = Frame()
    F.lits(20, 3).lits(9, 3).lits(7, 3).lits(0, 3)
    _add("L", "an empty block behind the last output byte", F, liblz4=False, liblz4_status=12)
