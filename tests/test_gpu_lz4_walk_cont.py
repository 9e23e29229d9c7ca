"""The fix-up rounds of the LZ4 chunk parse with the one-successor continuation (lz4_block_wave, lz4_wave.h), on the device: hand-built
plain frames (tests/lz4_walk_cases.py) whose walks sit on the rule's edges — phase-locked false chains over more than two chunks, a
literal run that jumps over the successor's segment, blocks of one chunk +- 1 / 59 / 61 bytes (a short or an inactive successor), the
block's last sequence and long lengths (the general token decoder) inside a continued segment, the same blocks damaged inside a
continued stretch, and one entry that k_lz4_left takes.  Bytes, status and produced size of every entry are the oracle's."""
import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests import lz4_walk_cases as W
from tests._libs import oracle
from tests.test_gpu_lz4_asm_batches import _frame, _judge, _run

pytestmark = pytest.mark.gpu
M = W.model()


@pytest.fixture(scope="module")
def codec():
    return zpack_amd.Codec(0)


def _entry(c, data=None):
    frame, at = _frame([("c", c["data"] if data is None else data)])
    return dict(label=c["label"], frame=frame, at=at[0], left=bool(c.get("left")))


@pytest.fixture(scope="module")
def cases():
    o = oracle()
    hot, left = [], []
    for c in W.intact_cases(M):
        e = _entry(c)
        rc, plain = o.lz4f_decode(e["frame"], 1 << 18)
        assert rc == 0 and len(plain) > 0, (c["label"], rc)
        e["plain"] = plain
        e["hash"] = dg.xxh3(np.frombuffer(plain, dtype=np.uint8))
        e["src"] = c
        assert (len(e["frame"]) < (len(plain) >> 3)) == e["left"], (c["label"], len(e["frame"]), len(plain))
        (left if e["left"] else hot).append(e)
    return hot, left


def _check_intact(codec, cs, long_runs):
    uncomp = [len(c["plain"]) for c in cs]
    arc, offs, desc, r, out, st = _run(codec, cs)
    assert st["lz4_handed_over"] == 0 and st["retried_lz4"] == 0 and st["lz4_general"] == 0 and st["lz4_long_runs"] == long_runs, st
    assert (r["status"] == 0).all(), [(cs[i]["label"], int(r[i]["status"])) for i in np.nonzero(r["status"])[0][:5]]
    assert _judge(cs, arc, offs, desc, r, out, uncomp, uncomp) == []
    for i, c in enumerate(cs):
        assert int(r[i]["produced"]) == len(c["plain"]) and int(r[i]["hash"]) == c["hash"], c["label"]
        a = int(desc[i]["dst_offset"])
        assert out[a:a + uncomp[i]].tobytes() == c["plain"], c["label"]


def test_intact_blocks_decode_to_the_oracles_bytes(codec, cases):
    hot, left = cases
    assert len(hot) == 11 and len(left) == 1
    _check_intact(codec, hot, 0)


def test_the_long_run_entry_goes_to_the_left_kernel(codec, cases):
    _check_intact(codec, cases[1], 1)


def _damaged(cases):
    """(a), (d), (e) damaged inside a stretch that a continuation walks: an offset field zeroed, a token byte changed"""
    out = []
    for e in cases[0]:
        c = e["src"]
        if c["label"][0] not in "ade":
            continue
        seen = set()
        for ch in M.parse_block(list(c["data"]), "call"):
            seen |= ch["cont_visits"]
        # a 3-byte sequence whose token a continuation visits, well inside the block: its offset field is the two bytes behind the token
        toks = sorted(p for p in seen if p + 1 in set(c["off_pos"]) and p > 600)
        assert len(toks) >= 4, c["label"]
        t = toks[len(toks) // 2]
        for kind in ("offset zeroed", "token changed"):
            d = bytearray(c["data"])
            if kind == "offset zeroed":
                d[t + 1:t + 3] = b"\x00\x00"
            else:
                d[t] ^= 0x35                                      # a literal run appears where there was none: the chain leaves its phase
            x = _entry(c, bytes(d))
            x.update(label="%s, %s at %d" % (c["label"], kind, t), plain=e["plain"], hash=e["hash"])
            out.append(x)
    return out


def test_damaged_blocks_get_the_oracles_verdict(codec, cases):
    cs = _damaged(cases)
    assert len(cs) == 6
    n = [len(c["plain"]) for c in cs]
    arc, offs, desc, r, out, st = _run(codec, cs, n, n)
    assert (r["status"] != 0).sum() >= 3, "the damage was not felt"
    assert _judge(cs, arc, offs, desc, r, out, n, n) == []
