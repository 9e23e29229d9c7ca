"""seq_exec_batch assembles a batch that holds self-overlapping matches of at most 32 bytes (the piece rule, seq_exec.h section 3a): the
match's lane copies it in pieces off, off, 2 off, 4 off ... through the round body.  The hand-built blocks of tests/lz4_overlap_blocks.py
— every length with every offset below it, first, in the middle and last in the batch; first periods that straddle the batch's start or
lie wholly before it; readers inside and behind a first period; periods that are another match's tail; a chain of 64 matches of 32 bytes
at offset 1, about 380 rounds — run once through k_lz4_wave and once, behind a trailing run, through k_lz4_left.  What is right is
decided by the oracle: status, produced size, XXH3 and every byte; the model says that each block sits where it means to."""
import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests._libs import oracle
from tests import lz4_overlap_blocks as blocks
from tests.test_gpu_lz4_asm_batches import M, _case, _judge, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    return zpack_amd.Codec(0)


@pytest.fixture(scope="module")
def cases():
    o = oracle()
    out = []
    for left in (False, True):
        cs = []
        for b in blocks.all_blocks(left):
            blocks.check_plan(b)
            c = _case(b["label"], b["blk"], b["data"], left)
            c["target"], c["want_asm"] = b["target"], b["want_asm"]
            rc, plain = o.lz4f_decode(c["frame"], 1 << 17)
            assert rc == 0 and 0 < len(plain) <= 65536, (c["label"], rc, len(plain))
            c["plain"] = plain
            c["hash"] = dg.xxh3(np.frombuffer(plain, dtype=np.uint8))
            assert (len(c["frame"]) < (len(plain) >> 3)) == left, (c["label"], len(c["frame"]), len(plain))
            cs.append(c)
        out.append(cs)
    return out


def test_the_blocks_sit_where_they_mean_to(cases):
    for cs in cases:
        labels = [c["label"] for c in cs]
        assert len(cs) >= 150 and len(set(labels)) == len(cs)
        assert sum(1 for c in cs if not c["want_asm"]) == 3 * 10                    # length 33: ten offsets, three places
        for c in cs:
            p = c["plan"][c["target"]]
            assert M.assembled(p, "next", True, True) == c["want_asm"] and not M.assembled(p, "next", True), (c["label"], p)
        ch = [c for c in cs if c["label"].startswith("chain")]
        assert len(ch) == 1 and ch[0]["target"] >= 12 and ch[0]["plan"][ch[0]["target"]]["self_steps"] == 6


@pytest.mark.parametrize("which", ["k_lz4_wave", "k_lz4_left"])
def test_intact_frames_decode_to_the_oracles_bytes(codec, cases, which):
    cs = cases[0] if which == "k_lz4_wave" else cases[1]
    uncomp = [len(c["plain"]) for c in cs]
    arc, offs, desc, r, out, st = _run(codec, cs)
    assert st["lz4_handed_over"] == 0 and st["retried_lz4"] == 0 and st["lz4_general"] == 0, st
    assert st["lz4_long_runs"] == (len(cs) if which == "k_lz4_left" else 0), st
    assert (r["status"] == 0).all(), [(cs[i]["label"], int(r[i]["status"])) for i in np.nonzero(r["status"])[0][:5]]
    assert _judge(cs, arc, offs, desc, r, out, uncomp, uncomp) == []
    for i, c in enumerate(cs):
        assert int(r[i]["produced"]) == len(c["plain"]) and int(r[i]["hash"]) == c["hash"], c["label"]
        a = int(desc[i]["dst_offset"])
        assert out[a:a + uncomp[i]].tobytes() == c["plain"], c["label"]


@pytest.mark.parametrize("which", ["k_lz4_wave", "k_lz4_left"])
@pytest.mark.parametrize("damage", ["offset 0", "offset beyond the output", "output one byte short", "entry one byte short"])
def test_damaged_frames_get_the_oracles_verdict(codec, cases, which, damage):
    cs = []
    for c in (cases[0] if which == "k_lz4_wave" else cases[1]):
        c = dict(c)
        if damage.startswith("offset"):
            k = 64 * c["target"] + 31                                               # an offset field in the middle of the batch under test
            f = bytearray(c["frame"])
            f[c["offs"][k]:c["offs"][k] + 2] = b"\x00\x00" if damage == "offset 0" else b"\xff\xff"
            c["frame"] = bytes(f)
        cs.append(c)
    n = [len(c["plain"]) for c in cs]
    uncomp = [x - 1 for x in n] if damage == "entry one byte short" else n
    caps = [x - 1 for x in n] if damage.endswith("short") else n
    arc, offs, desc, r, out, st = _run(codec, cs, uncomp, caps)
    assert (r["status"] != 0).sum() >= len(cs) - 8, "the damage was not felt"
    assert _judge(cs, arc, offs, desc, r, out, uncomp, caps) == []
