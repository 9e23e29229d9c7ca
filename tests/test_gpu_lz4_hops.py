"""The hop loops of lz4_walk (lz4_wave.h) carry no live flag: a lane is live while its position lies before its segment's end and, in
a re-walk, on no position the previous walk visited.  Hand-built plain frames (tests/lz4_hop_cases.py) put walks on the edges of that
rule, each under both cuts of the chunk boundary (the case's chunk at cpos = 0, and at cpos = 3919 behind a chunk that is one literal
run), and decode through decode_batch_device; status, bytes, produced size and XXH3 of every entry are the oracle's.

  * a re-walk that merges on position 0 of its segment (a continuation that enters the successor's segment on the successor's own entry),
    one that merges on the last token position of its segment, re-walks that never merge (phase-locked false chains: case (a) of
    tests/lz4_walk_cases.py and the same block behind the second cut);
  * a chain that jumps over a whole segment (a literal run of 70 bytes, a match with a length extension): a lane that never starts;
  * run-ins that meet the block's last sequence, or a malformed token, and give up;
  * length extensions of 254, of 255 + 0 (exactly 255) and of 255 + 255 + 0, on either side, met by a run-in and met inside a segment;
  * a token whose offset field ends exactly at the staged limit (chunk + 64 bytes of slack), and one byte past it;
  * chunks of 1 segment, of 64 segments and of 64 segments + 1 byte.

The CPU model (lz4_hop_cases.trace, the rounds of tools/sim/lz4_walk_cont_sim.py) says what the walks of every block do, and the test
asserts that the blocks sit on the events they mean to.  The seeds of the two merging blocks were found by running that model over
seeds 1..; the assertion below keeps them honest."""
import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests import lz4_hop_cases as H
from tests import lz4_walk_cases as W
from tests._libs import oracle
from tests.test_gpu_lz4_asm_batches import _frame, _judge, _run

pytestmark = pytest.mark.gpu
M = W.model()
MERGE_SEED = {"first": 2, "second": 1}


def _blocks():
    out = []
    for cut in H.CUTS:
        b, data = H.merging(cut, MERGE_SEED[cut])
        out.append(H.case("short sequences, seed %d" % MERGE_SEED[cut], cut, b, data,
                          [("cont", "merged", 0), "merged_on_last_token", "never_merged"]))
        out.append(H.phase_locked(cut))
        out.append(H.jumped(cut))
        out += [H.runin_meets(cut, what) for what in ("last", "malformed")]
        out += [H.ext255(cut, side, where, kind) for side in ("literal", "match") for where in ("run-in", "segment") for kind in H.EXT]
        out += [H.staged_limit(cut, d) for d in (0, 1)]
        out += [H.sized(cut, n) for n in (H.SEG, H.CHUNK, H.CHUNK + 1)]
    a = W.false_chains()                                   # case (a) as the existing walk tests build it
    out.append(dict(label=a["label"], data=a["data"], want=(("own", "never_merged"), ("cont", "never_merged")), off_pos=a["off_pos"]))
    return out


@pytest.fixture(scope="module")
def codec():
    return zpack_amd.Codec(0)


@pytest.fixture(scope="module")
def cases():
    o = oracle()
    good, bad = [], []
    for c in _blocks():
        frame, at = _frame([("c", c["data"])])
        rc, plain = o.lz4f_decode(frame, 1 << 18)
        e = dict(label=c["label"], frame=frame, src=c)
        if rc == 0:
            assert len(plain) > 0, c["label"]
            e.update(plain=plain, hash=dg.xxh3(np.frombuffer(plain, dtype=np.uint8)))
            assert len(frame) >= (len(plain) >> 3), (c["label"], "would go to k_lz4_left")
            good.append(e)
        else:                                              # (the block cut short: only the verdict is compared)
            e.update(plain=bytes(4096), hash=0)
            bad.append(e)
    return good, bad


def test_the_blocks_sit_on_the_events_they_mean_to(cases):
    good, bad = cases
    assert len(good) == 2 * 21 + 1 and len(bad) == 2, (len(good), len(bad))       # per cut 22 blocks, one of them cut short
    for e in good + bad:
        c = e["src"]
        ev = H.events(M, c["data"])
        assert all(w in ev for w in c["want"]), (c["label"], [w for w in c["want"] if w not in ev])
    # the chunk sizes: the case's chunk has 1 / 64 / 64 active lanes (the byte behind the 64th segment is staged, not walked: it
    # belongs to the block's last sequence)
    for cut, first in (("first", 0), ("second", 1)):
        for n, lanes in ((H.SEG, 1), (H.CHUNK, 64), (H.CHUNK + 1, 64)):
            t = H.trace(M, H.sized(cut, n)["data"])
            assert t[first][0] == (0, 3919)[first] and t[first][1] == lanes and len(t) == first + 1, (cut, n, [x[:2] for x in t])


def test_intact_blocks_decode_to_the_oracles_bytes(codec, cases):
    cs = cases[0]
    uncomp = [len(c["plain"]) for c in cs]
    arc, offs, desc, r, out, st = _run(codec, cs)
    assert st["lz4_handed_over"] == 0 and st["retried_lz4"] == 0 and st["lz4_general"] == 0 and st["lz4_long_runs"] == 0, st
    assert (r["status"] == 0).all(), [(cs[i]["label"], int(r[i]["status"])) for i in np.nonzero(r["status"])[0][:5]]
    assert _judge(cs, arc, offs, desc, r, out, uncomp, uncomp) == []
    for i, c in enumerate(cs):
        assert int(r[i]["produced"]) == len(c["plain"]) and int(r[i]["hash"]) == c["hash"], c["label"]
        a = int(desc[i]["dst_offset"])
        assert out[a:a + uncomp[i]].tobytes() == c["plain"], c["label"]


def test_blocks_cut_short_get_the_oracles_verdict(codec, cases):
    cs = cases[1]
    n = [len(c["plain"]) for c in cs]
    arc, offs, desc, r, out, st = _run(codec, cs, n, n)
    assert (r["status"] != 0).all()
    assert _judge(cs, arc, offs, desc, r, out, n, n) == []
