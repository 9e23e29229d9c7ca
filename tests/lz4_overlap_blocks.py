"""Hand-built LZ4 blocks for the piece rule of seq_exec_batch (seq_exec.h, section 3a, SELF_ASM): a self-overlapping match of at most 32
bytes no longer keeps a batch out of the LDS assembly, its lane copies it in pieces off, off, 2 off, 4 off ...  Every block is one block
of at most 64 KiB of output whose first batch is 64 literal-heavy sequences, so that the batch under test has the room; the CPU model
(tools/sim/lz4_asm_share.py) says whether it is assembled.  Used by tests/test_lz4_asm_overlap_model_cpu.py (a Python execution of the
batch against the oracle's bytes) and tests/test_gpu_lz4_asm_overlap.py (the device).  Not a test module."""
import numpy as np

from tests.lz4_asm import Block, M

LENGTHS = (4, 5, 16, 17, 31, 32, 33)                 # 33: still the direct path
OFFSETS = (1, 2, 3, 7, 8, 15, 16, 17, 31)            # and length - 1


def _finish(label, b, target, want_asm, left):
    b.fill(20)
    if left: b.run()
    data = b.done()
    return dict(label=label, blk=b, data=data, target=target, want_asm=want_asm, left=left)


def _head(seed):
    b = Block(seed)
    b.seq(14, 4)
    b.fill(63, ll=(10, 12), ml=(4, 6))                # batch 1: its input is the room of batch 2
    return b


def _one(label, seed, at, special, left, want_asm=True):
    """batch 2 = 64 sequences (1, 4, plain) with `special` = [(ll, ml, off)] in place of the ones from position `at` on"""
    b = _head(seed)
    i = 0
    while i < 64:
        if i == at:
            for ll, ml, off in special: b.seq(ll, ml, off)
            i += len(special)
        else:
            b.seq(1, 4); i += 1
    return _finish(label, b, 1, want_asm, left)


def matrix(left):
    """every length with every offset below it, the match first, in the middle and last in the batch.  First in the batch its source
    lies in its own two literals (offsets 1, 2) or straddles the batch's start (the 32 history bytes)"""
    out, seed = [], 1000
    for at in (0, 31, 63):
        for n in LENGTHS:
            for off in sorted(set(o for o in OFFSETS + (n - 1,) if o < n)):
                seed += 1
                out.append(_one("self %d off %d at %d" % (n, off, at), seed, at, [(2, n, off)], left, want_asm=n <= 32))
    return out


def shapes(left):
    out = []
    # at batch output position 0 with no literals: the first period lies wholly before the batch (early, then on from its own output)
    for k, (n, off) in enumerate(((32, 1), (17, 3), (31, 16), (5, 4), (32, 31))):
        out.append(_one("self %d off %d at batch position 0, no literals" % (n, off), 2000 + k, 0, [(0, n, off)], left))
    # a short match inside the first period of an earlier self-overlapping match (re-pointed), and one behind it (waits for all of it)
    out.append(_one("reader inside the first period", 2010, 20, [(2, 24, 6), (1, 4, 24)], left))
    out.append(_one("reader behind the first period", 2011, 20, [(2, 24, 6), (1, 8, 12)], left))
    out.append(_one("reader of the last byte", 2012, 20, [(2, 32, 1), (0, 4, 1), (0, 9, 3)], left))
    # a self-overlapping match whose first period is the tail of another's output
    out.append(_one("period is the tail of another's output", 2013, 30, [(2, 24, 6), (0, 20, 4)], left))
    out.append(_one("three in a row", 2014, 40, [(1, 32, 1), (0, 32, 2), (0, 31, 5)], left))
    # its own first period inside an earlier PLAIN match: the source is re-pointed (older output: early), then it goes on from its start
    out.append(_one("period inside an earlier plain match", 2015, 10, [(1, 20, 200), (0, 12, 5)], left))
    out.append(_one("period inside an earlier plain match of the batch's literals", 2016, 10, [(9, 8, 8), (0, 30, 4)], left))
    return out


def chain(left):
    """64 sequences (0, 32, 1), each reading the last byte of the one before: one lane moves per round, 6 pieces each.  The batch sits
    behind twelve batches of three-byte sequences, far enough into its chunk to have the room"""
    b = Block(2100)
    b.seq(14, 4)
    for _ in range(12 * 64 - 1):
        b.seq(0, int(b.rng.integers(4, 13)))
    for _ in range(64):
        b.seq(0, 32, 1)
    c = _finish("chain of 64 x (0, 32, 1)", b, 12, True, left)
    return [c]


def all_blocks(left):
    out = matrix(left) + shapes(left) + chain(left)
    for c in out:
        c["plan"] = M.plan(np.frombuffer(c["data"], dtype=np.uint8))
    return out


def check_plan(c):
    """the block sits where it means to: the batch under test begins at a multiple of 64 sequences, has the room, and the model assembles
    it exactly under the piece rule (a match of 33 bytes keeps it direct)"""
    p = c["plan"][c["target"]]
    assert p["chunk"] == 0 and p["index"] == c["target"] and p["first"] == 64 * c["target"] and p["count"] == 64, (c["label"], p)
    assert p["total"] + 48 <= p["room_next"], (c["label"], p)
    assert p["self_short"] or p["self_long"], (c["label"], p)
    assert not M.assembled(p, "next", True), (c["label"], p)
    assert M.assembled(p, "next", True, True) == c["want_asm"], (c["label"], p)
