"""The verdict block of seq_exec_batch (seq_exec.h, "1. output positions") gives a batch of 64 sequences the verdict of the FIRST
offending sequence in stream order, with one sequence's checks in a serial decoder's order (malformed token / literals do not fit /
bad offset / match does not fit).  Single LZ4 entries of a few hundred bytes whose offending sequence is the first, a middle and the
64th of a batch; the verdict is the oracle's (entry_decode), produced size and bytes too where the entry decodes:

  * dst_capacity exact, one short inside a literal run, one short inside a match;
  * offset 0; offset equal to the distance to the slot's start, and one more;
  * a bad offset in front of a sequence that would also not fit, and the reverse order;
  * literal and match lengths whose extension bytes sum beyond 2^23 (the decoder clamps them).

(The 32-bit form of these compares was measured and not taken, profiles/r35; the cases stand for whichever form the block has.)"""
import struct

import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests._libs import oracle
from tests.test_gpu_lz4_asm_batches import Block, _frame, _judge, _run

pytestmark = pytest.mark.gpu
AT = (0, 31, 63)


def _block(seed, giant=None):
    """70 short sequences; -> (Block, bytes, [(output position, literal length, match length, offset field position)] per sequence).
    giant = (k, "literal" | "match"): sequence k carries a length beyond 2^23"""
    b = Block(seed)
    seqs = []
    for i in range(70):
        ll, ml = int(b.rng.integers(1, 4)), int(b.rng.integers(4, 9))
        if giant and giant[0] == i and giant[1] == "match":
            ml = (1 << 23) + 1000
        if giant and giant[0] == i and giant[1] == "literal":           # the token and its extension bytes by hand: no such run exists
            b.d.append(0xF4)
            b.d += b"\xff" * 33000 + b"\x07"
            seqs.append((b.n, (1 << 23), 0, len(b.d)))
            b.d += bytes(40)
            return b, bytes(b.d), seqs
        start = b.n
        b.seq(ll, ml)
        seqs.append((start, ll, ml, b.off_pos[-1]))
    return b, b.done(), seqs


def _entries():
    o = oracle()
    out = []
    for k in AT:
        b, data, s = _block(40 + k)
        frame, at = _frame([("c", data)])
        rc, plain = o.lz4f_decode(frame, 1 << 16)
        assert rc == 0 and 300 < len(plain) < 2000, (rc, len(plain))
        h = dg.xxh3(np.frombuffer(plain, dtype=np.uint8))
        st, ll, ml, op = s[k]
        st1, ll1, ml1, op1 = s[k + 1]

        def entry(label, cap, patch=()):
            d = bytearray(data)
            for pos, off in patch:
                d[pos:pos + 2] = struct.pack("<H", off)
            f, _ = _frame([("c", bytes(d))])
            out.append(dict(label="%s, sequence %d" % (label, k), frame=f, plain=plain, hash=h, cap=cap))
        n = len(plain)
        entry("capacity exact", n)
        entry("one short inside the literal run", st + ll - 1)
        entry("one short inside the match", st + ll + ml - 1)
        entry("offset 0", n, [(op, 0)])
        entry("offset = distance to the slot's start", n, [(op, st + ll)])
        entry("offset one more than the distance", n, [(op, st + ll + 1)])
        entry("bad offset, then a sequence that does not fit", st1 + ll1 + 1, [(op, 0)])
        entry("a sequence that does not fit, then a bad offset", st + ll + ml - 1, [(op1, 0)])
        for side in ("literal", "match"):
            _, gd, _ = _block(40 + k, (k, side))
            f, _ = _frame([("c", gd)])
            out.append(dict(label="%s length beyond 2^23, sequence %d" % (side, k), frame=f, plain=bytes(4096), hash=0, cap=4096))
    return out


@pytest.fixture(scope="module")
def codec():
    return zpack_amd.Codec(0)


def test_verdicts_are_the_oracles(codec):
    cs = _entries()
    assert len(cs) == 3 * 10
    caps = [c["cap"] for c in cs]
    uncomp = list(caps)                   # (the directory's size is the capacity: a smaller capacity is refused before any decoding)
    arc, offs, desc, r, out, st = _run(codec, cs, uncomp, caps)
    assert _judge(cs, arc, offs, desc, r, out, uncomp, caps) == []
    status = {c["label"]: int(r[i]["status"]) for i, c in enumerate(cs)}
    for k in AT:
        assert status["capacity exact, sequence %d" % k] == 0, status
        for label in ("one short inside the literal run", "one short inside the match", "offset 0", "offset one more than the distance"):
            assert status["%s, sequence %d" % (label, k)] != 0, (label, k)
        # the two orders give two different verdicts: the first offender's
        assert status["bad offset, then a sequence that does not fit, sequence %d" % k] != status["a sequence that does not fit, then a bad offset, sequence %d" % k], status
