"""A Zstandard frame assembler written from RFC 8878, and the table of hand-built frames (CASES) that put the decoders on the edges of the
format and of their own private limits (table cells and packed sequences of zstd_fse4.h, the rings and windows of lx_ring.h / zstd_ring.h,
the inherited state of zstd_pj.h).  The assembler tracks only LENGTHS and CODES: which bytes a frame regenerates, whether it is valid and
how much it produces are decided by libzstd and the oracle (tests/test_zstd_asm_cpu.py), never here.

  Table / ncount_bytes     an FSE table from normalised counts, and its RFC 8878 4.1.1 description
  encode_seqs              the backward FSE sequence bitstream: last sequence first, initial states last, end mark
  Huf                      a Huffman code from weights: direct or FSE-compressed description, 1 or 4 streams
  lit_raw / lit_rle / lit_huf, nseq_bytes, Frame.comp / raw / rle, Frame.bytes

A sequence is (literal length, match length, Offset_Value): Offset_Value 1..3 are the repeat codes, offset + 3 otherwise.
"""
import random
import struct

LL, OF, ML = 0, 1, 2
PRE, RLE, FSE, REP = 0, 1, 2, 3
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
DEFAULT = {LL: ([4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6),
           OF: ([1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1], 5),
           ML: ([1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7, 6)}
MAX_AL = {LL: 9, OF: 8, ML: 9}
MAX_SYM = {LL: 35, OF: 31, ML: 52}
LL_MAX, ML_MAX = 131071, 131074
BLOCK_MAX = 128 << 10


def highbit(v):
    return v.bit_length() - 1


def ll_code(v):
    return max(c for c in range(36) if LL_BASE[c] <= v)


def ml_code(v):
    return max(c for c in range(53) if ML_BASE[c] <= v)


class Bits:
    """LSB-first container: what is added first ends up lowest"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def add(self, v, nb):
        assert 0 <= v < (1 << nb) or nb == 0 and v == 0, (v, nb)
        self.acc |= v << self.n
        self.n += nb

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


# ----------------------------------------------------------------------------- FSE

def ncount_bytes(counts, al):
    """RFC 8878 4.1.1: the description of normalised counts (-1 = "less than 1"); trailing zero counts are not written"""
    w = Bits()
    w.add(al - 5, 4)
    remaining, s = 1 << al, 0
    while remaining > 0:
        c = counts[s]
        s += 1
        v = c + 1
        nb = highbit(remaining + 1) + 1
        threshold = (1 << nb) - 1 - (remaining + 1)
        if v < threshold:
            w.add(v, nb - 1)
        elif v < (1 << (nb - 1)):
            w.add(v, nb)
        else:
            w.add(v + threshold, nb)
        remaining -= 1 if c < 0 else c
        if c == 0:
            z = 0
            while s + z < len(counts) and counts[s + z] == 0:
                z += 1
            s += z
            while z >= 3:
                w.add(3, 2)
                z -= 3
            w.add(z, 2)
    assert remaining == 0 and not any(counts[s:]), (remaining, counts[s:])
    return w.bytes()


class Table:
    """the decoding table of RFC 8878 4.1.1, and through it the one encoder state that leads to a given next state"""

    def __init__(self, counts, al):
        self.counts, self.al = list(counts), al
        size = 1 << al
        assert sum(abs(c) for c in counts) == size, (sum(abs(c) for c in counts), size)
        sym, high, nxt = [0] * size, size, {}
        for s, c in enumerate(counts):
            if c == -1:
                high -= 1
                sym[high] = s
                nxt[s] = 1
        step, pos = (size >> 1) + (size >> 3) + 3, 0
        for s, c in enumerate(counts):
            if c <= 0:
                continue
            nxt[s] = c
            for _ in range(c):
                sym[pos] = s
                pos = (pos + step) & (size - 1)
                while pos >= high:
                    pos = (pos + step) & (size - 1)
        assert pos == 0
        self.sym, self.nb, self.base = sym, [], []
        for i in range(size):
            n = nxt[sym[i]]
            nxt[sym[i]] += 1
            nb = al - highbit(n)
            self.nb.append(nb)
            self.base.append((n << nb) - size)

    @classmethod
    def rle(cls, s):
        t = object.__new__(cls)
        t.counts, t.al, t.sym, t.nb, t.base = None, 0, [s], [0], [0]
        return t

    def desc(self):
        return bytes([self.sym[0]]) if self.counts is None else ncount_bytes(self.counts, self.al)

    def states(self, s):
        return [i for i in range(len(self.sym)) if self.sym[i] == s]

    def last_state(self, s, most_bits=False):
        """a state for the last symbol of a stream (free choice): the lowest, or the one whose update reads the most bits"""
        st = self.states(s)
        assert st, ("symbol not in table", s)
        return max(st, key=lambda i: (self.nb[i], -i)) if most_bits else st[0]

    def prev_state(self, s, nxt):
        """the state that decodes `s` and can move to state `nxt` -> (state, update bits, number of bits)"""
        for i in self.states(s):
            if self.base[i] <= nxt < self.base[i] + (1 << self.nb[i]):
                return i, nxt - self.base[i], self.nb[i]
        raise AssertionError(("symbol not in table", s))


PREDEF = {k: Table(*DEFAULT[k]) for k in (LL, OF, ML)}


def counts_for(used, al, less_than_one=()):
    """normalised counts in which every code of `used` has a cell: 1 each (-1 for less_than_one), the first takes the rest"""
    used = sorted(set(used))
    c = [0] * (max(used) + 1)
    for s in used:
        c[s] = -1 if s in less_than_one else 1
    first = [s for s in used if s not in less_than_one][0]
    c[first] = (1 << al) - (len(used) - 1)
    return c


def seq_codes(seq):
    ll, ml, ofv = seq
    return ll_code(ll), highbit(ofv), ml_code(ml)


def encode_seqs(seqs, tll, tof, tml, most_bits=False, junk_bits=0, end_mark=True, positions=None):
    """the sequences bitstream.  The decoder reads: states LL, OF, ML; then per sequence the extra bits of OF, ML, LL and (except
    behind the last) the state updates of LL, ML, OF.  Everything is written in the reverse of that order."""
    w = Bits()
    w.add(0, junk_bits)                                        # bits the decoder never reads: the stream is then under-consumed
    sl = so = sm = None
    for i in range(len(seqs) - 1, -1, -1):
        ll, ml, ofv = seqs[i]
        lc, oc, mc = seq_codes(seqs[i])
        if sl is None:
            sl, so, sm = tll.last_state(lc, most_bits), tof.last_state(oc, most_bits), tml.last_state(mc, most_bits)
        else:
            so, bo, no = tof.prev_state(oc, so)
            sm, bm, nm = tml.prev_state(mc, sm)
            sl, bl, nl = tll.prev_state(lc, sl)
            w.add(bo, no)
            w.add(bm, nm)
            w.add(bl, nl)
        w.add(ll - LL_BASE[lc], LL_BITS[lc])
        w.add(ml - ML_BASE[mc], ML_BITS[mc])
        w.add(ofv - (1 << oc), oc)
        if positions is not None:
            positions.insert(0, w.n)                           # the stream position (in bits) at which the decoder begins sequence i
    w.add(sm, tml.al)
    w.add(so, tof.al)
    w.add(sl, tll.al)
    if end_mark:
        w.add(1, 1)
        return w.bytes()
    return w.bytes() + b"\x00"


def seq_bits(seq, tll, tof, tml):
    """the most bits one sequence can take: its extra bits plus three full state updates"""
    lc, oc, mc = seq_codes(seq)
    return LL_BITS[lc] + ML_BITS[mc] + oc + tll.al + tof.al + tml.al


def nseq_bytes(n, form=None):
    form = form or (1 if n < 128 else (2 if n < 0x7F00 else 3))
    if form == 1:
        assert n < 128
        return bytes([n])
    if form == 2:
        assert n < 0x7F00
        return bytes([128 + (n >> 8), n & 255])
    assert 0x7F00 <= n <= 0x7F00 + 0xFFFF
    return b"\xff" + struct.pack("<H", n - 0x7F00)


# ----------------------------------------------------------------------------- Huffman

class Huf:
    """weights[symbol] (the last non-zero one included) -> codes in the decoder's table order: weight classes ascending, natural
    symbol order inside a class"""

    def __init__(self, weights):
        while weights[-1] == 0:
            weights = weights[:-1]
        self.w = list(weights)
        total = sum(1 << (x - 1) for x in self.w if x)
        self.mb = highbit(total)
        assert total == 1 << self.mb, total
        self.code, pos = {}, 0
        for ww in range(1, self.mb + 1):
            for sy, x in enumerate(self.w):
                if x == ww:
                    self.code[sy] = (pos >> (ww - 1), self.mb + 1 - ww)
                    pos += 1 << (ww - 1)
        self.alphabet = sorted(self.code)

    def desc_direct(self):
        listed = self.w[:-1]
        assert len(listed) <= 128
        p = listed + [0] * (len(listed) & 1)
        return bytes([127 + len(listed)]) + bytes((p[i] << 4) | p[i + 1] for i in range(0, len(p), 2))

    def desc_fse(self, al=6):
        """the listed weights through two interleaved FSE states (RFC 8878 4.2.1.1); the stream ends when an update over-reads"""
        listed = self.w[:-1]
        n = len(listed)
        assert n >= 2
        hist = [listed.count(s) for s in range(max(listed) + 1)]
        counts = _normalise(hist, al)
        t = Table(counts, al)
        st = [None] * n
        w = Bits()
        st[n - 1] = t.last_state(listed[n - 1])
        st[n - 2] = t.last_state(listed[n - 2], most_bits=True)
        assert t.nb[st[n - 2]] > 0                              # its update must read below the stream's start
        for k in range(n - 3, -1, -1):
            st[k], b, nb = t.prev_state(listed[k], st[k + 2])
            w.add(b, nb)
        w.add(st[1], al)
        w.add(st[0], al)
        w.add(1, 1)
        body = ncount_bytes(counts, al) + w.bytes()
        assert len(body) < 128
        return bytes([len(body)]) + body

    def stream(self, syms):
        w = Bits()
        for sy in reversed(syms):
            c, nb = self.code[sy]
            w.add(c, nb)
        w.add(1, 1)
        return w.bytes()

    def streams4(self, syms):
        seg = (len(syms) + 3) // 4
        s = [self.stream(syms[i * seg:(i + 1) * seg]) for i in range(3)] + [self.stream(syms[3 * seg:])]
        return struct.pack("<HHH", len(s[0]), len(s[1]), len(s[2])) + b"".join(s)


def _normalise(hist, al):
    """counts proportional to hist that sum to 2^al, every present symbol at least 1"""
    size, total = 1 << al, sum(hist)
    c = [max(1, h * size // total) if h else 0 for h in hist]
    big = max(range(len(c)), key=lambda i: c[i])
    c[big] += size - sum(c)
    assert c[big] > 0
    return c


# ----------------------------------------------------------------------------- literals sections

def _lit_small_header(kind, n, fmt):
    fmt = fmt if fmt is not None else (0 if n < 32 else (1 if n < 4096 else 3))
    if fmt in (0, 2):
        assert n < 32
        return bytes([kind | (fmt << 2) | (n << 3)])
    if fmt == 1:
        assert n < 4096
        return (kind | (1 << 2) | (n << 4)).to_bytes(2, "little")
    assert n < (1 << 20)
    return (kind | (3 << 2) | (n << 4)).to_bytes(3, "little")


def lit_raw(data, fmt=None):
    return _lit_small_header(0, len(data), fmt) + bytes(data)


def lit_rle(byte, n, fmt=None):
    return _lit_small_header(1, n, fmt) + bytes([byte])


def lit_huf(huf, syms, fmt=None, treeless=False, fse=False):
    """Compressed (2) or Treeless (3) literals; fmt 0 = one stream, 1..3 = four streams with 10 / 14 / 18-bit sizes"""
    n = len(syms)
    tree = b"" if treeless else (huf.desc_fse() if fse else huf.desc_direct())
    if fmt is None:
        fmt = 0 if n < 64 else 1
    body = tree + (huf.stream(syms) if fmt == 0 else huf.streams4(syms))
    kind, c = (3 if treeless else 2), len(body)
    while fmt and (max(n, c) >> (10, 10, 14, 18)[fmt]):
        fmt += 1
    if fmt < 2:
        assert n < 1024 and c < 1024, (n, c)
        return (kind | (fmt << 2) | (n << 4) | (c << 14)).to_bytes(3, "little") + body
    if fmt == 2:
        assert n < 16384 and c < 16384
        return (kind | (2 << 2) | (n << 4) | (c << 18)).to_bytes(4, "little") + body
    assert n <= BLOCK_MAX and c < (1 << 18)
    return (kind | (3 << 2) | (n << 4) | (c << 22)).to_bytes(5, "little") + body


# ----------------------------------------------------------------------------- blocks and frames

class Frame:
    """blocks are added in order; the tables and the Huffman code in force travel with the frame as they do in a decoder"""

    def __init__(self, seed=1, fcs=None, single=True, window=None, did=None, checksum=False, reserved=False):
        self.rng = random.Random(seed)
        self.fcs, self.single, self.window, self.did, self.checksum, self.reserved = fcs, single, window, did, checksum, reserved
        self.blocks = []                       # (type, size field, payload)
        self.n = 0                             # bytes the frame regenerates, by the lengths
        self.tab = {LL: None, OF: None, ML: None}
        self.huf = None
        self.modes = []                        # per compressed block with sequences: (LL, OF, ML) modes

    def rand(self, n, alphabet=None):
        return bytes(self.rng.choice(alphabet) for _ in range(n)) if alphabet else bytes(self.rng.randrange(256) for _ in range(n))

    def raw(self, n):
        self.blocks.append((0, n, self.rand(n)))
        self.n += n
        return self

    def rle(self, n, byte=0x61):
        self.blocks.append((1, n, bytes([byte])))
        self.n += n
        return self

    def block(self, btype, size, payload, regen=0):
        self.blocks.append((btype, size, payload))
        self.n += regen
        return self

    def literals(self, n, kind="raw", fmt=None, huf=None, fse=False):
        if kind == "raw":
            return lit_raw(self.rand(n), fmt)
        if kind == "rle":
            return lit_rle(0x62, n, fmt)
        if kind == "huf":
            self.huf = huf or self.huf or Huf([4, 3, 2, 1, 1])
            return lit_huf(self.huf, self.rand(n, self.huf.alphabet), fmt, False, fse)
        assert kind == "treeless"
        h = self.huf or Huf([4, 3, 2, 1, 1])   # (in a first block there is none to inherit: the frame is malformed)
        return lit_huf(h, self.rand(n, h.alphabet), fmt, True)

    def seq_section(self, seqs, modes=(PRE, PRE, PRE), tables=None, al=None, form=None, reserved=0, **kw):
        """modes per kind; tables: {kind: Table} for FSE (default: counts_for the codes used), RLE needs one code per kind"""
        if not seqs:
            return nseq_bytes(0, form) if form != 2 else bytes([128, 0])
        codes = list(zip(*[seq_codes(s) for s in seqs]))
        out = bytearray(nseq_bytes(len(seqs), form))
        out.append((modes[LL] << 6) | (modes[OF] << 4) | (modes[ML] << 2) | reserved)
        for k in (LL, OF, ML):
            m = modes[k]
            if m == PRE:
                self.tab[k] = PREDEF[k]
            elif m == RLE:
                assert len(set(codes[k])) == 1
                self.tab[k] = Table.rle(codes[k][0])
                out += self.tab[k].desc()
            elif m == FSE:
                self.tab[k] = (tables or {}).get(k) or Table(counts_for(codes[k], (al or {}).get(k, 5)), (al or {}).get(k, 5))
                out += self.tab[k].desc()
            else:
                self.tab[k] = self.tab[k] or PREDEF[k]         # (nothing to repeat: malformed, any table serves to write the bits)
        self.modes.append(tuple(modes))
        return bytes(out + encode_seqs(seqs, self.tab[LL], self.tab[OF], self.tab[ML], **kw))

    def comp(self, seqs, tail=0, lit="raw", lit_fmt=None, huf=None, fse=False, short_lits=0, **kw):
        """one compressed block: literals for every sequence's literal length plus `tail` behind the last (minus short_lits)"""
        nlit = sum(s[0] for s in seqs) + tail - short_lits
        body = self.literals(nlit, lit, lit_fmt, huf, fse) + self.seq_section(seqs, **kw)
        self.blocks.append((2, len(body), body))
        self.n += nlit + sum(s[1] for s in seqs)
        return self

    def header(self, content_size):
        fcs = self.fcs if self.fcs is not None else (1 if content_size < 256 else (2 if content_size < 65536 + 256 else 4))
        single = self.single and fcs != 0
        dn, dv = self.did or (0, 0)
        fhd = ({0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs] << 6) | (single << 5) | (self.reserved << 3) | (bool(self.checksum) << 2) | {0: 0, 1: 1, 2: 2, 4: 3}[dn]
        h = struct.pack("<I", 0xFD2FB528) + bytes([fhd])
        if not single:
            h += bytes([self.window if self.window is not None else (7 << 3)])      # default 128 KiB
        h += dv.to_bytes(dn, "little")
        if fcs == 2:
            content_size -= 256
        return h + (content_size.to_bytes(fcs, "little") if fcs else b"")

    def bytes(self, content_size=None, xxh64=None):
        """content_size overrides the FCS; xxh64(frame without a checksum) -> the content's XXH64, needed for the checksum flag"""
        out = bytearray(self.header(self.n if content_size is None else content_size))
        for i, (t, size, payload) in enumerate(self.blocks):
            out += ((i == len(self.blocks) - 1) | (t << 1) | (size << 3)).to_bytes(3, "little") + payload
        if self.checksum:
            c = xxh64(self._without_checksum()) & 0xFFFFFFFF
            out += struct.pack("<I", c ^ (1 if self.checksum == "wrong" else 0))
        return bytes(out)

    def _without_checksum(self):
        keep, self.checksum = self.checksum, False
        try:
            return self.bytes()
        finally:
            self.checksum = keep


def _content_xxh64(frame):
    from tests._libs import oracle
    rc, plain = oracle().zstd_decode(frame, 1 << 19)
    assert rc == 0, rc
    return oracle().xxh64(plain)


# ----------------------------------------------------------------------------- the case table

CASES = []
_SEEN = set()


def case(group, label, f, two_stage=True, cap=None, uncomp=None, content_size=None, **expect):
    """two_stage: True = must finish on the two-stage path; a string = declined by design, with the file and line that declines it;
    None = not asserted (groups A, B and I, and every frame libzstd rejects).  expect: what the oracle's stats and trace must show."""
    assert label not in _SEEN, label
    _SEEN.add(label)
    frame = f.bytes(content_size, _content_xxh64) if isinstance(f, Frame) else f
    n = f.n if isinstance(f, Frame) else 0
    CASES.append(dict(group=group, label=label, frame=frame, uncomp=n if uncomp is None else uncomp, cap=cap, two_stage=two_stage,
                      modes=f.modes if isinstance(f, Frame) else [], expect=expect))


S = [(5, 6, 4 + 3), (2, 8, 1), (0, 9, 2 + 3)]            # three plain sequences: 7 literals, 23 match bytes (the two-stage path needs 8 output bytes per sequence)


def _group_a():
    for nb, n in ((1, 200), (2, 256), (2, 65791), (4, 70000), (8, 300)):
        f = Frame(10 + nb, fcs=nb)
        for k in range(0, n, BLOCK_MAX):
            f.raw(min(BLOCK_MAX, n - k))
        case("A", "FCS in %d bytes holding %d" % (nb, n), f, None, has_fcs=1, fcs_bytes=nb, single_segment=1, window_size=n, raw_blocks=(n + BLOCK_MAX - 1) // BLOCK_MAX)
    case("A", "no FCS, window mantissa 5", Frame(15, fcs=0, window=(2 << 3) | 5).raw(300).comp(S, 3), None,
         has_fcs=0, single_segment=0, window_size=4096 + 5 * 512)
    case("A", "smallest window", Frame(16, fcs=0, window=0).raw(900).comp(S, 3), None, has_fcs=0, window_size=1024)
    for dn in (1, 2, 4):
        case("A", "dictionary id of %d bytes holding 0" % dn, Frame(17 + dn, did=(dn, 0)).raw(100).comp(S, 3), None, has_fcs=1, dict_id_bytes=dn)
    case("A", "dictionary id 7", Frame(22, did=(1, 7)).raw(100).comp(S, 3), None, reject=True)
    case("A", "reserved bit set", Frame(23, reserved=True).raw(100).comp(S, 3), None, reject=True)
    case("A", "content checksum right", Frame(24, checksum=True).raw(100).comp(S, 3), None, has_checksum=1)
    case("A", "content checksum wrong", Frame(25, checksum="wrong").raw(100).comp(S, 3), None, reject=True)


def _group_b():
    case("B", "Raw, RLE and Compressed blocks in one frame", Frame(30).raw(50).rle(70).comp(S, 3).rle(9).raw(4), None,
         raw_blocks=2, rle_blocks=2, comp_blocks=1, blocks=5)
    case("B", "empty last Raw block", Frame(31).comp(S, 3, lit="raw").raw(0), None, raw_blocks=1, comp_blocks=1)
    case("B", "RLE block of 1 byte", Frame(32).rle(1), None, rle_blocks=1)
    case("B", "RLE block of 128 KiB", Frame(33).rle(BLOCK_MAX), None, rle_blocks=1)
    case("B", "Raw block of exactly Block_Maximum_Size", Frame(34).raw(BLOCK_MAX), None, raw_blocks=1)
    case("B", "Raw block one byte above Block_Maximum_Size", Frame(35).raw(BLOCK_MAX + 1), None, libzstd_decides=True)
    case("B", "RLE block one byte above Block_Maximum_Size", Frame(36).rle(BLOCK_MAX + 1), None, libzstd_decides=True)
    case("B", "block type 3", Frame(37).raw(20).block(3, 5, b"\0" * 5), None, reject=True)
    case("B", "compressed block that regenerates 0 bytes", Frame(38).raw(10).comp([], 0, lit_fmt=3).raw(5), None, comp_blocks=1, sequences=0)
    case("B", "compressed block of 2 bytes", Frame(41).raw(10).comp([], 0).raw(5), None, libzstd_decides=True)
    case("B", "blocks produce more than the FCS", Frame(39).raw(100).comp(S, 3), None, content_size=120, reject=True)
    case("B", "blocks produce less than the FCS", Frame(40).raw(100).comp(S, 3), None, content_size=130, uncomp=130, reject=True)


H5 = [4, 3, 2, 1, 1]


def _group_c():
    for n in (31, 32, 4095, 4096):
        fmt = 0 if n < 32 else (1 if n < 4096 else 3)          # Size_Format: 5, 12 and 20 bits
        case("C", "Raw literals of %d" % n, Frame(50 + n).comp([(n - 2, 4, 1 + 3)], 2), lit_raw=1, sequences=1, lit_small_fmt=fmt)
        case("C", "RLE literals of %d" % n, Frame(51 + n).comp([(n - 2, 4, 1 + 3)], 2, lit="rle"), lit_rle=1, sequences=1, lit_small_fmt=fmt)
    case("C", "Raw literals of 7 in the 3-byte size format", Frame(60).comp(S, 0, lit_fmt=3), lit_raw=1, lit_small_fmt=3)
    case("C", "Raw literals of 7 in the 2-byte size format", Frame(61).comp(S, 0, lit_fmt=1), lit_raw=1, lit_small_fmt=1)
    case("C", "Huffman literals, 1 stream", Frame(62).comp([(300, 4, 9)], 200, lit="huf", lit_fmt=0), lit_huf=1, lit_huf_1stream=1, huf_direct_weights=1)
    for n, fmt in ((1023, 1), (16383, 2), (40000, 3), (BLOCK_MAX - 8, 3)):
        case("C", "Huffman literals, 4 streams, %d in size format %d" % (n, fmt), Frame(63 + fmt + n).comp([(n - 8, 8, 20)], 8, lit="huf", lit_fmt=fmt),
             lit_huf=1, lit_huf_4stream=1, lit_fmt=fmt)
    for n in (3, 4, 6, 7, 40, 41, 42, 43):
        case("C", "Huffman literals, 4 streams of %d literals" % n, Frame(70 + n).comp([(3, 8, 2 + 3)], n - 3, lit="huf", lit_fmt=1),
             libzstd_decides=n < 8, lit_huf_4stream=1)
    h11 = Huf([1, 1] + list(range(2, 12)))
    h12 = Huf([1, 1] + list(range(2, 13)))
    for name, h in (("1", Huf([1, 1])), ("2", Huf([2, 1, 1])), ("11", h11), ("12", h12)):
        for fmt in (0, 1):
            case("C", "maximum code length %s, %s" % (name, "4 streams" if fmt else "1 stream"),
                 Frame(80 + fmt).comp([(500, 7, 100 + 3), (0, 5, 1)], 300, lit="huf", lit_fmt=fmt, huf=h), lit_huf=1, huf_max_bits=int(name))
    h256 = Huf([(3 if s % 4 == 0 else (2 if s % 4 == 1 else 1)) for s in range(256)])
    case("C", "256-symbol alphabet, FSE-compressed weights", Frame(90).comp([(900, 7, 100 + 3)], 100, lit="huf", huf=h256, fse=True),
         lit_huf=1, huf_fse_weights=1, huf_max_bits=9)
    h129 = Huf([2] * 127 + [1, 1])
    case("C", "direct weights at 128 symbols", Frame(91).comp([(900, 7, 100 + 3)], 100, lit="huf", huf=h129), lit_huf=1, huf_direct_weights=1, huf_max_bits=8)
    case("C", "FSE-compressed weights, small alphabet", Frame(92).comp([(400, 7, 100 + 3)], 100, lit="huf", huf=Huf([5, 4, 3, 0, 2, 1, 1]), fse=True),
         lit_huf=1, huf_fse_weights=1)
    case("C", "Treeless directly after a Huffman block", Frame(93).comp(S, 200, lit="huf", huf=Huf(H5)).comp(S, 300, lit="treeless"),
         lit_huf=1, lit_treeless=1)
    case("C", "Treeless with a Raw-literals block and a Raw block in between",
         Frame(94).comp(S, 200, lit="huf", huf=Huf(H5)).comp(S, 9).raw(33).comp(S, 300, lit="treeless"), lit_huf=1, lit_treeless=1, lit_raw=1, raw_blocks=1)
    case("C", "Treeless in the first block", Frame(95).comp(S, 200, lit="treeless"), None, reject=True)
    case("C", "no literals left behind the last sequence", Frame(96).comp(S, 0), sequences=3)
    case("C", "literals left behind the last sequence", Frame(97).comp(S, 77), sequences=3)
    case("C", "sum of literal lengths one above the literals present", Frame(98).comp(S, 0, short_lits=1), None, uncomp=29, reject=True)


# k_zstd_fse has one arena word per 8 bytes of the entry's output slot: an entry with more sequences than that stays with the fused decoder
# table descriptions without sequences are read by zstd_block (zstd_wg.h) alone: k_zstd_fse leaves the entry to the fused decoder
LONG_ZERO = "zpack_amd/csrc/zstd_fse4.h:403 (a Number_of_Sequences of 0 in the two-byte form: nseq == 0 -> ok = false)"
ARENA_ROOM = "zpack_amd/csrc/zstd_fse4.h:407 (nseq > seq_cap - seq_n: more than one sequence per 8 output bytes)"


def _group_d():
    def many(n):
        return [(2, 6 + (i % 5), 1 + 3 + (i % 3)) for i in range(n)]
    case("D", "0 sequences", Frame(100).comp([], 40), sequences=0, nseq_form=0)
    for n in (1, 63, 64, 65, 127, 128):
        case("D", "%d sequences" % n, Frame(100 + n).comp([(8, 4, 5)] + many(n - 1), 2), sequences=n, nseq_form=1 if n < 128 else 2)
    case("D", "2-byte form holding 5", Frame(110).comp([(8, 4, 5)] + many(4), 2, form=2), sequences=5, nseq_form=2)
    case("D", "2-byte form holding 0, nothing behind it", Frame(111).comp([], 40, form=2), None, libzstd_decides=True)
    body = lit_raw(bytes(range(40))) + b"\x80\x00" + bytes([FSE << 6]) + ncount_bytes([30, 1, 1], 5) + b"\x77\x01"
    # libzstd builds the tables such a block describes, but marks "tables in force" only in a block that has sequences: the next
    # Repeat_Mode block uses the NEW table if an earlier block had sequences, and is malformed if none had
    for first in (True, False):
        f = Frame(115).raw(9)
        if first:
            f.comp(S, 1)
        f.block(2, len(body), body, 40)
        f.tab[LL] = Table([30, 1, 1], 5)
        f.comp([(0, 4, 5), (1, 4, 5), (2, 4, 1)], 2, modes=(REP, PRE, PRE))
        case("D", "2-byte form holding 0 with a table description behind it, then Repeat_Mode" + (" (an earlier block has sequences)" if first else ""), f, LONG_ZERO if first else None,
             **(dict(sequences=6, comp_blocks=3) if first else dict(reject=True)))
    case("D", "0x7EFF sequences", Frame(112).raw(8).comp([(0, 3, 1)] * 0x7EFF, 2, modes=(RLE, RLE, PRE)), ARENA_ROOM, sequences=0x7EFF, nseq_form=2)
    # 0x7F00 sequences of 3 bytes regenerate 97 536 bytes: inside one block
    case("D", "0x7F00 sequences", Frame(114).raw(8).comp([(0, 3, 1)] * 0x7F00, 2, modes=(RLE, RLE, RLE)), ARENA_ROOM, sequences=0x7F00, nseq_form=3)


def _group_e():
    s2 = [(6, 5, 9), (6, 5, 9), (6, 5, 9)]                    # one code per kind: fit for RLE mode
    for m, name in ((PRE, "Predefined"), (RLE, "RLE"), (FSE, "FSE_Compressed")):
        case("E", "all three kinds %s" % name, Frame(120 + m).comp(s2 if m == RLE else S * 3, 4, modes=(m, m, m)), seq_modes=[(m, m, m)])
        case("E", "Repeat after %s" % name, Frame(124 + m).comp(s2, 4, modes=(m, m, m)).comp(s2, 4, modes=(REP, REP, REP)), seq_modes=[(m, m, m), (REP,) * 3])
    case("E", "mixed modes in one block", Frame(130).comp(s2 * 2, 4, modes=(FSE, RLE, PRE)).comp(s2, 1, modes=(RLE, PRE, FSE)).comp(s2, 1, modes=(PRE, FSE, RLE)),
         seq_modes=[(FSE, RLE, PRE), (RLE, PRE, FSE), (PRE, FSE, RLE)])
    case("E", "Repeat mixed with new tables", Frame(131).comp(S * 2, 4, modes=(FSE, FSE, FSE)).comp(S, 1, modes=(REP, PRE, REP)).comp(S, 1, modes=(REP, REP, FSE)),
         seq_modes=[(FSE,) * 3, (REP, PRE, REP), (REP, REP, FSE)])
    case("E", "Repeat across a Raw block", Frame(132).comp(S * 2, 4, modes=(FSE, FSE, FSE)).raw(17).comp(S, 1, modes=(REP, REP, REP)), seq_modes=[(FSE,) * 3, (REP,) * 3])
    case("E", "Repeat across a compressed block with 0 sequences", Frame(133).comp(S * 2, 4, modes=(FSE, FSE, FSE)).comp([], 17).comp(S, 1, modes=(REP, REP, REP)),
         seq_modes=[(FSE,) * 3, (REP,) * 3])
    case("E", "Repeat in the first block", Frame(134).comp(S, 4, modes=(REP, REP, REP)), None, reject=True)
    case("E", "Repeat of one kind in the first block", Frame(135).comp(S, 4, modes=(PRE, REP, PRE)), None, reject=True)
    case("E", "reserved mode bits set", Frame(136).comp(S, 4, reserved=1), libzstd_decides=True)         # libzstd 1.4.9 ignores them


def _group_f():
    base = [(800, 6, 30), (3, 9, 1), (0, 40, 700), (2, 3, 2)]
    for k, name in ((LL, "LL"), (OF, "OF"), (ML, "ML")):
        used = sorted(set(seq_codes(s)[k] for s in base))
        for al in (5, MAX_AL[k], MAX_AL[k] + 1):
            t = Table(counts_for(used, al), al)
            modes = tuple(FSE if j == k else PRE for j in range(3))
            ok = al <= MAX_AL[k]
            case("F", "%s accuracy log %d" % (name, al), Frame(140 + al).comp(base * 4, 5, modes=modes, tables={k: t}), True if ok else None,
                 **(dict(seq_modes=[modes]) if ok else dict(reject=True)))
        top = MAX_SYM[k] if k != OF else 17                    # (an offset code is also the number of extra bits: 17 stays inside the output)
        modes = tuple(FSE if j == k else PRE for j in range(3))
        t = Table(counts_for(used + [top], 6, less_than_one=[top]), 6)
        case("F", "highest legal %s symbol present in the description" % name, Frame(150 + k).comp(base * 2, 5, modes=modes, tables={k: t}), seq_modes=[modes])
        body = lit_raw(b"abcd") + b"\x01" + bytes([RLE << (6 - 2 * k), MAX_SYM[k] + 1]) + b"\x55\x01"
        case("F", "RLE-mode %s symbol above the kind's maximum" % name, Frame(153 + k).raw(40).block(2, len(body), body, 0), None, uncomp=48, reject=True)
    llused = sorted(set(seq_codes(s)[LL] for s in base))
    c = counts_for(llused + [30, 31, 33], 6, less_than_one=[30, 31, 33])
    case("F", "several less-than-1 symbols", Frame(160).comp(base * 3, 5, modes=(FSE, PRE, PRE), tables={LL: Table(c, 6)}), seq_modes=[(FSE, PRE, PRE)])
    c = [0] * 36
    c[0], c[20] = 63, 1                                        # symbols 1..19 are nineteen zeros: flags 3, 3, 3, 3, 3, 3, 0
    seqs = [(0, 4, 5), (24, 4, 5), (0, 4, 1)] * 3
    case("F", "one symbol owning all but one cell, zero-run flags chained", Frame(161).raw(40).comp(seqs, 5, modes=(FSE, PRE, PRE), tables={LL: Table(c, 6)}),
         seq_modes=[(FSE, PRE, PRE)])
    c = [0] * 36
    c[0], c[9], c[20] = 40, 23, 1                              # zeros 1..8 (flags 3, 3, 1) and 10..19 (flags 3, 3, 3, 0)
    seqs = [(0, 4, 5), (9, 4, 5), (24, 4, 1)] * 3
    case("F", "zero-run flags chained as 3, 3, 1", Frame(162).raw(40).comp(seqs, 5, modes=(FSE, PRE, PRE), tables={LL: Table(c, 6)}), seq_modes=[(FSE, PRE, PRE)])
    # a description that ends exactly on a byte: searched for among small count sets
    for a in range(1, 31):
        c = [a, 32 - a - 1, 1]
        if _ncount_bit_length(c, 5) % 8 == 0:
            seqs = [(0, 4, 5), (1, 4, 5), (2, 4, 1)] * 3
            case("F", "description ending exactly on a byte", Frame(163).raw(40).comp(seqs, 5, modes=(FSE, PRE, PRE), tables={LL: Table(c, 5)}),
                 seq_modes=[(FSE, PRE, PRE)], ncount_on_byte=1)
            break
    # counts cannot overshoot the table in this description: a value is read in just enough bits for "what remains + 1".  The nearest
    # malformed descriptions: more symbols than the kind has, and a description cut short
    body = lit_raw(b"abcd") + b"\x01" + bytes([FSE << 6]) + ncount_bytes([31] + [0] * 36 + [1], 5) + b"\x55\x01"
    case("F", "description with a symbol above the kind's maximum", Frame(164).raw(40).block(2, len(body), body, 0), None, uncomp=48, reject=True)


def _ncount_bit_length(counts, al):
    """bits the description takes (the writer pads to a byte)"""
    n, remaining, s = 4, 1 << al, 0
    while remaining > 0:
        c = counts[s]
        s += 1
        nb = highbit(remaining + 1) + 1
        n += nb - 1 if c + 1 < (1 << nb) - 1 - (remaining + 1) else nb
        remaining -= 1 if c < 0 else c
        assert c != 0
    return n


# k_zstd_fse pre-decodes such a block, k_zstd_exec gives the entry up and the fused decoder finishes it
BLOCK_ABOVE_MAX = "zpack_amd/csrc/zstd_ring.h:119 (LX_E_BLOCKMAX: a block that regenerates more than 128 KiB is zstd_block's)"


def _group_g():
    for bits in (0, 1):
        seqs = [(LL_BASE[c] + bits * ((1 << LL_BITS[c]) - 1), 4, 3 + 7) for c in range(16, 32)]         # 16..31: up to 8191; 32..35 below
        case("G", "LL codes 16..31, extra bits all %d" % bits, Frame(170 + bits).comp(seqs, 3), ll_values=[s[0] for s in seqs])
        seqs = [(1, ML_BASE[c] + bits * ((1 << ML_BITS[c]) - 1), 3 + 5) for c in range(32, 49)]
        case("G", "ML codes 32..48, extra bits all %d" % bits, Frame(172 + bits).raw(10).comp(seqs, 3), ml_values=[s[1] for s in seqs])
        for c in range(32, 36):
            v = LL_BASE[c] + bits * ((1 << LL_BITS[c]) - 1)
            if v + 8 <= BLOCK_MAX:
                case("G", "LL code %d, extra bits all %d" % (c, bits), Frame(174 + c).comp([(v, 4, 3 + 7)], 0, lit="rle"),
                     ll_values=[v])
        for c in range(49, 53):
            v = ML_BASE[c] + bits * ((1 << ML_BITS[c]) - 1)
            if v + 8 <= BLOCK_MAX:
                case("G", "ML code %d, extra bits all %d" % (c, bits), Frame(180 + c).raw(8).comp([(2, v, 3 + 7)], 0), ml_values=[v])
    # libzstd 1.4.9 accepts both: nothing in it holds what a block regenerates to Block_Maximum_Size
    case("G", "the largest LL the format expresses", Frame(190).comp([(LL_MAX, 4, 3 + 7)], 0, lit="rle"), BLOCK_ABOVE_MAX, libzstd_decides=True,
         ll_values=[LL_MAX], block_regen_above_max=True)
    case("G", "the largest ML the format expresses", Frame(191).raw(8).comp([(2, ML_MAX, 3 + 7)], 0), BLOCK_ABOVE_MAX, libzstd_decides=True,
         ml_values=[ML_MAX], block_regen_above_max=True)
    # repeat codes: history after the first two sequences is (20, 11, 1)... walked through every order
    head = [(30, 4, 3 + 11), (0, 4, 3 + 20)]
    case("G", "repeat codes 1, 2, 3 with LL > 0", Frame(192).comp(head + [(1, 4, 1), (1, 4, 2), (1, 4, 3)], 3), repcode_uses=3)
    case("G", "repeat codes 1, 2, 3 with LL = 0", Frame(193).comp(head + [(0, 4, 1), (0, 4, 2), (0, 4, 3)], 3), repcode_uses=3)
    case("G", "LL = 0 and code 3: rep0 - 1", Frame(194).comp(head + [(0, 4, 3), (1, 5, 1)], 3), repcode_uses=2, offsets={2: 19, 3: 19})
    case("G", "LL = 0 and code 3 where rep0 - 1 is 0", Frame(195).comp([(30, 4, 3 + 1), (0, 4, 3)], 3), libzstd_decides=True, repcode_uses=1, offsets={1: 1})
    # rotate (code 3, or code 2 at LL = 0), rotate, swap (code 2, or code 1 at LL = 0), rotate, rotate: all six orders, then code 1
    walk = [(1, 4, 3), (0, 4, 2), (1, 4, 2), (0, 4, 2), (1, 4, 3), (0, 4, 1), (1, 4, 1)]
    case("G", "a run of repeat codes through every order of the history", Frame(196).comp([(40, 4, 3 + 31)] + head + walk, 3), repcode_uses=len(walk), all_orders=True)
    case("G", "initial history 1, 4, 8 used by the first sequences", Frame(197).comp([(9, 4, 1), (1, 4, 2), (1, 4, 3)], 3), repcode_uses=3, offsets={0: 1, 1: 4, 2: 8})
    case("G", "initial history: offset 8 with 7 bytes of output", Frame(198).comp([(7, 4, 3)], 3), None, uncomp=14, reject=True)
    case("G", "initial history: offset 4 behind 3 literals", Frame(199).comp([(3, 4, 2)], 3), None, uncomp=10, reject=True)
    case("G", "offset equal to the output so far", Frame(200).raw(50).comp([(10, 9, 3 + 60)], 3), offsets={0: 60})
    case("G", "offset one more than the output so far", Frame(201).raw(50).comp([(10, 9, 3 + 61)], 3), None, reject=True)
    case("G", "offset above the declared window but inside the output", Frame(202, fcs=0, window=0).raw(1500).comp([(10, 9, 3 + 1400)], 3),
         libzstd_decides=True, window_size=1024, offsets={0: 1400})
    # One sequence that needs the most bits the format allows in a frame of at most 256 KiB: LL code 35 and ML code 52 (16 + 16 extra
    # bits), offset code 17 (an offset of 128 KiB: the literal run itself is what it reaches back over) and three full state updates of
    # 9 / 8 / 9 bits = 75 bits, at three places of the backward stream.  Its block regenerates 192 KiB, which libzstd accepts and the
    # execute stage hands to the fused decoder: so the same three places once more with 15 + 15 + 16 + 26 = 72 bits in a block that
    # stays below 128 KiB and finishes two-stage.
    al = {LL: 9, OF: 8, ML: 9}
    for bits, big, front, fill, first, verdict in (
            (75, (LL_MAX, ML_BASE[52] + 2, (1 << 17) + 5), 64, (0, 3, 3 + 37), (0, 4, 8), BLOCK_ABOVE_MAX),
            (72, (LL_BASE[34] + 1, ML_BASE[51] + 2, (1 << 16) + 5), BLOCK_MAX + 4, (1, 3, 3 + 37), (9, 4, 8), True)):
        filler = [fill] * 200                                 # sequences of 5 extra bits each, in front or behind

        def frame():
            f = Frame(203)
            for k in range(0, front, BLOCK_MAX):
                f.raw(min(BLOCK_MAX, front - k))
            return f
        nfill = 0
        for n in range(100, 200):                             # so many behind it that its bits lie across bit 512 k of the stream
            pos = []
            frame().comp([first] + filler[:100] + [big] + filler[:n], 0, lit="rle", modes=(FSE, FSE, FSE), al=al, positions=pos)
            if (pos[101] - 1) >> 9 != pos[102] >> 9 and 16 <= (pos[101] & 511) <= 56:
                nfill = n
                break
        assert nfill
        for where, seqs in (("at the low end of the stream", [first] + filler + [big]), ("directly under the end mark", [big] + filler),
                            ("in the middle, across the 64-byte chunks", [first] + filler[:100] + [big] + filler[:nfill])):
            f = frame()
            f.comp(seqs, 0, lit="rle", modes=(FSE, FSE, FSE), al=al, most_bits=where.startswith("at the low"))
            assert seq_bits(big, *[f.tab[k] for k in (LL, OF, ML)]) == bits
            case("G", "a %d-bit sequence %s" % (bits, where), f, verdict, big_seq=(big[2] - 3, big[1], big[0]),
                 big_seq_at=where.split()[0].replace("at", "low").replace("directly", "top"), big_seq_bits=bits, seq_modes=[(FSE, FSE, FSE)],
                 **(dict(block_regen_above_max=True) if bits == 75 else {}))
    case("G", "a stream whose last byte is 0", Frame(206).comp(S, 3, end_mark=False), None, uncomp=33, reject=True)
    case("G", "a stream with unread bits left over", Frame(207).comp(S, 3, junk_bits=40), None, uncomp=33, reject=True)


def _group_h():
    for v in (1023, 1024, 1025):
        case("H", "LL of %d" % v, Frame(210).comp([(40, 4, 9), (v, 5, 3 + 30), (3, 4, 1)], 5), ll_values=[40, v, 3])
        case("H", "ML of %d" % v, Frame(211).comp([(40, 4, 9), (2, v, 3 + 30), (3, 4, 1)], 5), ml_values=[4, v, 4])
    for off in (1023, 1024, 1025, 4095, 4096, 4097):
        pre = off + 50
        case("H", "offset %d, no overlap" % off, Frame(212).comp([(pre, 4, 3 + 2), (3, 300, 3 + off), (1, 5, 1)], 5), offsets={1: off})
        case("H", "offset %d, the match overlaps itself" % off, Frame(213).comp([(pre, 4, 3 + 2), (3, off + 700, 3 + off), (1, 5, 1)], 5), offsets={1: off})
    for start in (900, 3900):                                  # across a 1 KiB line, across the 4 KiB ring's wrap
        seqs = [(start, 4, 3 + 2)] + [(1, 40 + p, 3 + p) for p in range(1, 17)]
        case("H", "overlapping matches of period 1..16 from output position %d" % start, Frame(214).comp(seqs, 5), offsets={p: p for p in range(1, 17)},
             crosses=1024 if start < 1024 else 4096)
    case("H", "a source that starts in flushed memory and ends in the ring", Frame(215).comp([(6000, 4, 9), (100, 3000, 3 + 5000), (1, 5, 1)], 5), offsets={1: 5000}, far_source=True)
    for n in (3071, 3072, 3073):
        case("H", "an entry of %d bytes" % n, Frame(216).comp([(1500, 200, 3 + 700), (5, 300, 1)], n - 2005), produced=n)
    case("H", "literal runs crossing the 1 KiB literal window", Frame(217).comp([(1000, 4, 9), (48, 4, 1), (1500, 6, 3 + 100), (1024, 4, 1), (1, 4, 1)], 3000, lit="huf"),
         ll_values=[1000, 48, 1500, 1024, 1])
    f = Frame(218).comp([(500, 200, 3 + 300), (5, 300, 1)], 77)
    case("H", "an entry that fills dst_capacity exactly", f, cap=f.n, produced=f.n)
    # (uncomp_size one short as well: an entry whose capacity is below its stated size never reaches a decoder, lib/zpack_read.c:328)
    case("H", "an entry that overflows dst_capacity by one byte", Frame(218).comp([(500, 200, 3 + 300), (5, 300, 1)], 77), None, cap=f.n - 1, uncomp=f.n - 1, reject=True)


def _group_i():
    # each frame: 2 to 6 compressed blocks; the block-parallel reader hands the repeat offsets, the Huffman code and the tables
    # in force from block to block
    b1 = [(60, 5, 3 + 33), (2, 6, 3 + 17), (4, 4, 3 + 50)]    # leaves the history (50, 17, 33)
    rep0 = [(0, 5, 1), (0, 4, 2), (0, 6, 3), (3, 4, 1)]       # LL = 0: codes 1, 2, 3 mean rep1, rep2, rep0 - 1
    case("I", "a block that begins with repeat codes at LL = 0", Frame(230).comp(b1, 9).comp(rep0, 9).comp(rep0, 0), None, comp_blocks=3, repcode_uses=8,
         offsets={3: 17, 4: 33, 5: 32})
    case("I", "history through a zero-sequence block, a Raw block and an RLE block",
         Frame(231).comp(b1, 9).comp([], 30).comp(rep0, 2).raw(21).comp(rep0, 2).rle(300).comp(rep0, 2), None, comp_blocks=5, raw_blocks=1, rle_blocks=1,
         repcode_uses=12)
    f = Frame(232).comp(b1 + rep0 + b1, 200, lit="huf", huf=Huf(H5), modes=(FSE, FSE, FSE)).raw(40).comp([], 10).rle(5)
    f.comp(b1 + rep0, 300, lit="treeless", modes=(REP, REP, REP)).comp(rep0, 100, lit="treeless", modes=(REP, PRE, REP))
    case("I", "Treeless and Repeat_Mode blocks that inherit across Raw, RLE and zero-sequence blocks", f, None, lit_treeless=2, comp_blocks=4,
         seq_modes=[(FSE,) * 3, (REP,) * 3, (REP, PRE, REP)])
    case("I", "a last block that is empty", Frame(233).comp(b1, 9).comp(rep0, 9).comp([], 0, lit_fmt=3), None, comp_blocks=3)
    case("I", "a last Raw block that is empty", Frame(234).comp(b1, 9).comp(rep0, 9).raw(0), None, comp_blocks=2, raw_blocks=1)
    big = [(3000, 40000, 3 + 2000), (100, 30000, 3 + 90000)]
    case("I", "large blocks, far offsets inherited", Frame(235).raw(100000).comp(big, 50, lit="rle").comp([(0, 9, 1), (0, 9, 1), (7, 30000, 3 + 150000)], 9), None,
         comp_blocks=2, offsets={2: 2000, 3: 90000, 4: 150000})
    # (the host paths give the reader only entries that are worth a turn of the whole chip, pj_choose in zpk_codec.hip: this one is)
    case("I", "two blocks of 120 KiB, repeat codes at LL = 0 inherited: large enough to be worth the reader",
         Frame(238).comp([(3000, 60000, 3 + 2000), (100, 60000, 3 + 50000)], 50, lit="rle").comp([(0, 9, 1), (0, 9, 1), (7, 60000, 3 + 100000), (5, 60000, 1)], 9), None,
         comp_blocks=2, offsets={2: 2000, 3: 50000, 4: 100000, 5: 100000}, reader=True)
    case("I", "a frame with a content checksum: not the block-parallel reader's (host_walk.h: zpj_parse_frame_header)",
         Frame(236, checksum=True).comp(b1, 9).comp(rep0, 9).comp(rep0, 0), None, comp_blocks=3, has_checksum=1, block_parallel=False)
    case("I", "a block that regenerates more than 128 KiB: given up inside the reader (zstd_pj.h: k_zpj_pos)",
         Frame(237).comp(b1, 9).comp([(2, ML_MAX, 3 + 7)] + rep0, 0).comp(rep0, 0), None, comp_blocks=3, block_regen_above_max=True, zpj_err=True)
    # An inherited offset near 2^27 - 1 needs 128 MiB of output in front of it: no frame of at most 256 KiB can express a VALID one
    # (an offset beyond the output is rejected by every decoder before it is inherited), so the case table has none.


for _g in (_group_a, _group_b, _group_c, _group_d, _group_e, _group_f, _group_g, _group_h, _group_i):
    _g()
