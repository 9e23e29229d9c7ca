"""tests/lz4_frames.py is not vacuous: it accepts the frames of the oracle's encoder and of the reference writer (the golden archive), and
turns down hand-built frames of a few dozen bytes that break ONE rule each, naming that rule."""
import os
import struct

import pytest

from benchdata import datagen as dg
from tests import lz4_frames, zpk
from tests._libs import oracle

SIZES = (0, 1, 12, 13, 14, 100, 65535, 65536, 65537, 200000)


@pytest.mark.parametrize("cls", [dg.TEXT, dg.RUNS, dg.RANDOM], ids=["text", "runs", "random"])
def test_accepts_the_oracle_encoders_frames(cls):
    """30 inputs: three classes at the ten sizes.  Also what the walk returns: the blocks' plain sizes, and that text and runs of the
    larger sizes really went out compressed (else nothing but stored blocks would have been walked)."""
    o = oracle()
    for k, n in enumerate(SIZES):
        plain = dg.fill(cls, 1400, k, n)
        frame = o.lz4f_encode(plain)
        blocks = lz4_frames.walk(frame, n)
        assert [b[1] for b in blocks] == [min(65536, n - at) for at in range(0, n, 65536)], (cls, n)
        assert sum(4 + b[2] for b in blocks) + 11 == len(frame)
        if cls != dg.RANDOM and n >= 65535:
            assert not any(b[0] for b in blocks if b[1] >= 100), (cls, n)
            assert all(len(b[3]) > 1 for b in blocks if b[1] >= 100)


def test_accepts_the_reference_writers_frames(golden_dir):
    arc = open(os.path.join(golden_dir, "ref_workdir", "archive_lz4.zpk"), "rb").read()
    entries = [e for e in zpk.parse(arc) if e["method"] == 2]
    assert entries
    for e in entries:
        blocks = lz4_frames.walk(arc[e["offset"]:e["offset"] + e["comp_size"]], e["uncomp_size"])
        assert sum(b[1] for b in blocks) == e["uncomp_size"]


# ---- hand-built frames ------------------------------------------------------------------------------------------------------------------

def seq(lits, off=None, ml=None, raw_off=None):
    """one sequence: the literals, then (unless off is None: the block's last sequence) a match"""
    ll = len(lits)
    mlc = 0 if off is None else ml - 4
    out = bytearray([(min(ll, 15) << 4) | min(mlc, 15)])

    def ext(v):
        if v >= 15:
            v -= 15
            out.extend(b"\xff" * (v // 255) + bytes([v % 255]))
    ext(ll)
    out += lits
    if off is not None:
        out += struct.pack("<H", off) if raw_off is None else raw_off
        ext(mlc)
    return bytes(out)


def header(flg=0x40, bd=0x40, hc=None, magic=0x184D2204):
    d = bytes([flg, bd])
    return struct.pack("<I", magic) + d + bytes([(oracle().xxh32(d) >> 8) & 0xFF if hc is None else hc])


def block(body, stored=False, word=None):
    return struct.pack("<I", (len(body) | (0x80000000 if stored else 0)) if word is None else word) + body


END = b"\0\0\0\0"
L = b"abcdefghijklmnopqrstuvwxyz"
GOOD = seq(L[:4], 4, 8) + seq(L[:8])                    # 4 literals, 8 bytes from 4 back, 8 literals: 20 plain bytes in 16


def test_the_base_of_the_hand_built_frames_is_accepted():
    """... and decodes: the rejects below differ from it in one respect each."""
    f = header() + block(GOOD) + END
    assert lz4_frames.walk(f, 20) == [(False, 20, 16, [(4, 8, 4), (8, 0, 0)])]
    assert oracle().lz4f_decode(f, 20) == (0, b"abcdabcdabcdabcdefgh")
    two = header() + block(bytes(65536), stored=True) + block(GOOD) + END
    assert [b[:3] for b in lz4_frames.walk(two, 65556)] == [(True, 65536, 65536), (False, 20, 16)]
    d = bytes([0x40 | 0x10 | 0x08 | 0x04, 0x40])                            # block checksums, content size, content checksum
    d += struct.pack("<Q", 20)
    sums = struct.pack("<I", 0x184D2204) + d + bytes([(oracle().xxh32(d) >> 8) & 0xFF])
    sums += block(GOOD) + struct.pack("<I", oracle().xxh32(GOOD)) + END + b"\1\2\3\4"
    assert [b[:3] for b in lz4_frames.walk(sums, 20)] == [(False, 20, 16)]


REJECTS = [
    ("offset zero", header() + block(seq(L[:4], 0, 8) + seq(L[:8])) + END, 20),
    ("offset beyond history", header() + block(seq(L[:4], 5, 8) + seq(L[:8])) + END, 20),
    ("offset beyond history", header(flg=0x60) + block(bytes(range(30)), stored=True) + block(seq(L[:4], 5, 8) + seq(L[:8])) + END, 50),   # independent blocks
    ("block end", header() + block(seq(L[:4], 4, 16)) + END, 20),                                     # a match running to the block's end
    ("block end", header() + block(seq(L[:4], 4, 8) + seq(L[:8])[:-1]) + END, 19),                    # literals cut off
    ("block end", header() + block(seq(L[:4], 4, 8) + bytes([0x81]) + L[:8]) + END, 20),              # a last token with a match length
    ("last literals", header() + block(seq(L[:4], 4, 12) + seq(L[:4])) + END, 20),
    ("last match start", header() + block(seq(L[:4], 4, 6) + seq(L[:5])) + END, 15),                  # it starts 11 bytes before the end
    ("short block compressed", header() + block(seq(L[:1], 1, 6) + seq(L[:5])) + END, 12),
    ("compressed not smaller", header() + block(seq(L[:8], 4, 4) + seq(L[:8])) + END, 20),            # 20 bytes for 20
    ("length extension", header() + block(seq(L[:4], 4, 8) + bytes([0xF0]) + b"\xff" * 9) + END, 20),
    ("EndMark", header() + block(GOOD), 20),
    ("EndMark", header() + block(GOOD) + END[:3], 20),
    ("HC", header(hc=(oracle().xxh32(bytes([0x40, 0x40])) >> 8) & 0xFF ^ 0x10) + block(GOOD) + END, 20),
    ("trailing bytes", header() + block(GOOD) + END + b"\0", 20),
    ("magic", header(magic=0x184D2203) + block(GOOD) + END, 20),
    ("FLG version", header(flg=0x80) + block(GOOD) + END, 20),
    ("FLG reserved", header(flg=0x42) + block(GOOD) + END, 20),
    ("BD reserved", header(bd=0x41) + block(GOOD) + END, 20),
    ("BD block size", header(bd=0x30) + block(GOOD) + END, 20),
    ("block size word", header() + block(bytes(65537), stored=True) + END, 65537),
    ("block truncated", header() + block(GOOD, word=17), 20),
    ("stored size", header() + block(L[:21], stored=True) + END, 20),
    ("plain length", header() + block(GOOD) + END, 21),
    ("block not full", header() + block(L[:10], stored=True) + block(L[:10], stored=True) + END, 20),
    ("content checksum", header(flg=0x44) + block(GOOD) + END, 20),
]


@pytest.mark.parametrize("k", range(len(REJECTS)), ids=["%02d-%s" % (k, r[0].replace(" ", "-")) for k, r in enumerate(REJECTS)])
def test_rejects(k):
    rule, frame, plain_len = REJECTS[k]
    assert len(frame) < 100 or rule == "block size word"
    with pytest.raises(AssertionError, match="rule '%s' violated" % rule):
        lz4_frames.walk(frame, plain_len)


def test_every_rule_the_walker_states_is_reached_by_a_reject():
    """... but for 'match length' (the encoding cannot express a match below 4), 'header truncated', 'content size' and 'block checksum'
    (flags the project's own frames never set; accepted above)."""
    assert set(lz4_frames.RULES) - {r[0] for r in REJECTS} == {"match length", "header truncated", "content size", "block checksum"}
