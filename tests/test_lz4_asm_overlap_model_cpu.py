"""The piece rule of seq_exec_batch (seq_exec.h, section 3a): in an assembled batch a self-overlapping match of at most 32 bytes is
copied by its own lane in pieces off, off, 2 off, 4 off ... through the round body.  tools/sim/lz4_exec_sim.py executes one assembled
batch in plain Python under that rule — the dependency sets and the re-pointing of the kernel, the early matches, the rounds with all
loads of a round ahead of its stores, the round guard — and the bytes it produces must be the oracle's.  No GPU.

Three sets of blocks: the hand-built ones of tests/lz4_overlap_blocks.py (the device test runs the same), every batch of the benchmark's
text and records frames that the model assembles under the rule, and seeded random blocks in which nearly every batch chains."""
import importlib.util
import os

import numpy as np
import pytest

from benchdata import datagen as dg
from tests._libs import oracle
from tests import lz4_overlap_blocks as blocks
from tests.test_gpu_lz4_asm_batches import Block, M, _frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sim():
    spec = importlib.util.spec_from_file_location("lz4_exec_sim", os.path.join(ROOT, "tools", "sim", "lz4_exec_sim.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


X = _sim()


def _with_literals(d):
    """-> [(literal bytes, ml, off)] of one well-formed block (the last sequence has ml = 0)"""
    out = []
    d = bytes(d)
    for t0, ll, ml, off, nxt in M.sequences(np.frombuffer(d, dtype=np.uint8)):
        p = t0 + 1
        if ll >= 15:
            p += 1 + (ll - 15) // 255
        out.append((d[p:p + ll], ml, off))
    return out


def _check_block(data, plain, label, only=None, stats=None):
    """every batch of the block that the model assembles under the piece rule (only: just that batch), executed on the oracle's
    history, gives the oracle's bytes within the guard.  -> number of batches executed"""
    seqs = _with_literals(data)
    n = 0
    for k, p in enumerate(M.plan(np.frombuffer(data, dtype=np.uint8))):
        if (only is not None and k != only) or not M.assembled(p, "next", True, True):
            continue
        bs = seqs[p["first"]:p["first"] + p["count"]]
        got, rounds = X.exec_assembled(plain[:p["out"]], bs)
        assert got is not None, (label, k, "guard or no progress after %d rounds" % rounds)
        assert rounds <= X.ROUND_GUARD
        assert got == plain[p["out"]:p["out"] + p["total"]], (label, k)
        if stats is not None:
            stats.append((rounds, p["self_short"], p["self_steps"]))
        n += 1
    return n


def _decode(data):
    frame, _ = _frame([("c", data)])
    rc, plain = oracle().lz4f_decode(frame, 1 << 17)
    assert rc == 0 and len(plain) <= 65536 + 64
    return plain


def test_the_guard_is_the_one_of_the_kernel():
    src = open(os.path.join(ROOT, "zpack_amd", "csrc", "seq_exec.h")).read()
    assert "#define SEQ_ASM_ROUNDS_SELF (64u * 6u + 16u)" in src and X.ROUND_GUARD == 64 * 6 + 16
    assert [M.pieces(32, 1), M.pieces(32, 31), M.pieces(4, 3), M.pieces(17, 16), M.pieces(31, 8), M.pieces(8, 8)] == [6, 2, 2, 2, 3, 1]


@pytest.mark.parametrize("left", [False, True])
def test_hand_built_blocks(left):
    cs = blocks.all_blocks(left)
    assert len(cs) >= 150
    ran = 0
    for c in cs:
        blocks.check_plan(c)
        plain = _decode(c["data"])
        st = []
        n = _check_block(c["data"], plain, c["label"], only=c["target"], stats=st)
        assert n == (1 if c["want_asm"] else 0), c["label"]
        ran += n
        if c["label"].startswith("chain"):            # one lane moves per round: 64 x 6 pieces, less the first lane's early piece
            assert 378 <= st[0][0] <= 64 * 6, st
    assert ran == len(cs) - 3 * 10                      # all but the matches of 33 bytes: ten offsets, three places


@pytest.mark.parametrize("mix", [dg.TEXT, dg.RECORDS])
def test_benchmark_frames(mix):
    spec = importlib.util.spec_from_file_location("lz4_walk_sim", os.path.join(ROOT, "tools", "sim", "lz4_walk_sim.py"))
    w = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(w)
    b = dg.Batch(8, 65536, 65536, method=dg.LZ4, level=0, seed=1, mix=mix)
    o = oracle()
    st = []
    for e in range(8):
        fr = b.archive[int(b.offsets[e]):int(b.offsets[e]) + int(b.comp_sizes[e])]
        rc, plain = o.lz4f_decode(fr.tobytes(), 1 << 17)
        assert rc == 0 and len(plain) == 65536
        blks = w.blocks_of(fr)
        assert len(blks) == 1                           # (one block per entry: batch positions are entry positions)
        _check_block(blks[0].tobytes(), plain, "mix %d entry %d" % (mix, e), stats=st)
    moved = [s for s in st if s[1]]
    assert len(st) >= 400 and len(moved) >= 40, (len(st), len(moved))      # the rule moves about an eighth / a tenth of the batches
    assert max(s[0] for s in st) <= 70


def test_random_chains():
    """sequences (ll 0..3, ml 4..32, off 1..31): nearly every match reads the few bytes in front of it, and most feed themselves"""
    rng = np.random.default_rng(30)
    st = []
    for blk in range(6):
        b = Block(500 + blk)
        b.seq(14, 4)
        b.fill(63, ll=(10, 12), ml=(4, 6))
        short = blk >= 3                                # half of the blocks: periods of 1..3 bytes only, the longest chains
        for _ in range(64 * 10):
            ll, ml = int(rng.integers(0, 4)), int(rng.integers(4, 33)) if not short else int(rng.integers(24, 33))
            b.seq(ll, ml, int(rng.integers(1, 4 if short else 32)))
        data = b.done()
        _check_block(data, _decode(data), "random %d" % blk, stats=st)
    assert len(st) >= 30, len(st)                       # (of 60: a chunk's first batches have no room)
    assert max(s[0] for s in st) > 70, sorted(s[0] for s in st)[-5:]       # the old guard would have refused a legal batch
    assert max(s[0] for s in st) <= X.ROUND_GUARD
