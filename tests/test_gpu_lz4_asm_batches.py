"""seq_exec_batch assembles a batch of 64 LZ4 sequences in the dead part of the staged input when the batch's output fits there.  The
dead part runs up to the NEXT batch's first token (the chain's exit for a chunk's last batch), so an assembly overwrites the batch's
own tokens and literals in the stage.  Hand-built plain frames put batches on both sides of every edge of that rule — tools/sim/
lz4_asm_share.py (the CPU model of the chunking and of the rule) says where each batch of a block sits, and the tests assert that the
blocks sit where they mean to.  What is right is decided by the oracle: bytes, status and produced size of every entry."""
import os

import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests._libs import oracle
from tests.lz4_asm import Block, M, _frame, _model        # (the assembler lives there now; these names are used by other test modules)
from tests.test_gpu_lz4_lean import _assemble, _device_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(label, blk, data, left=False):
    """one compressed block as a frame; the damage positions are offset fields inside the block"""
    frame, at = _frame([("c", data)])
    return dict(label=label, frame=frame, offs=[at[0] + p for p in blk.off_pos], left=left, plan=M.plan(np.frombuffer(data, dtype=np.uint8)))


def _tuned(label, build, batch, rule, d, left=False):
    """build(knob) -> (Block, bytes).  The knob is turned until batch `batch` of the block has total + 48 == room + d"""
    def miss(knob):
        blk, data = build(knob)
        p = M.plan(np.frombuffer(data, dtype=np.uint8))
        return p[batch]["total"] + 48 - p[batch]["room_" + rule], blk, data
    d0, d1 = miss(0)[0], miss(1)[0]
    guess = (d - d0) // (d1 - d0) if d1 != d0 else 0                  # (one step of the knob is one byte)
    for knob in range(max(0, guess - 2), guess + 3):
        got, blk, data = miss(knob)
        if got == d:
            c = _case("%s d=%+d" % (label, d), blk, data, left)
            c["target"] = batch
            return c
    raise AssertionError("no knob puts %s at %+d" % (label, d))


def _room_cases(left):
    out = []

    def three_batches(knob, a, m):            # batch 1: its input decides the room of batch 2, whose first match straddles its start
        b = Block(11)
        b.seq(14, 4)
        for i in range(63):
            b.seq((knob + i) // 63, 4)
        b.seq(a, m, a + 6)
        for _ in range(63):
            b.seq(a, m)
        b.fill(10)
        if left: b.run()
        return b, b.done()

    def last_batch(knob):                     # batch 2 is the chunk's last: its room ends at the chain's exit
        b = Block(12)
        b.seq(14, 4)
        b.fill(63, ll=(0, 2), ml=(4, 4))
        for i in range(30):
            b.seq(2, 4 + (knob + i) // 30)
        if left: b.run()
        return b, b.done()

    def second_chunk(knob):                   # the same in a block's second chunk (cpos != 0)
        b = Block(13)
        b.seq(3900, 4)                            # (a literal run longer than a chunk: the first chunk is this one sequence)
        b.fill(64, ll=(0, 2), ml=(4, 4))
        for i in range(30):
            b.seq(2, 4 + (knob + i) // 30)
        if left: b.run()
        return b, b.done()

    for d in (-1, 0, 1):
        out.append(_tuned("next room, own tokens overwritten", lambda k: three_batches(k, 3, 8), 1, "next", d, left))
        out.append(_tuned("old room", lambda k: three_batches(k, 2, 4), 1, "own", d, left))
        if not left:                                          # (behind a run the run's batch is the last one)
            out.append(_tuned("chunk's last batch", last_batch, 1, "next", d))
            out.append(_tuned("last batch of the second chunk", second_chunk, 2, "next", d))
            assert [x["chunk"] for x in out[-1]["plan"]] == [0, 1, 1] and out[-1]["plan"][1]["cpos"] > 3840
    return out


def _window_cases(left):
    """minimal 3-byte sequences: more than 576 in a chunk, the token list refills in mid-chunk; batch 9 begins exactly at the window
    boundary and batch 8 ends at it"""
    b = Block(14)
    b.seq(14, 4)
    n = 1279 if left else 2600
    for i in range(n):
        b.seq(0, int(b.rng.integers(4, 13)))
    if left: b.run()
    data = b.done()
    c = _case("3-byte sequences", b, data, left)
    p = c["plan"]
    assert max(x["index"] for x in p) >= 18 and p[9]["first"] == 576 and p[9]["chunk"] == 0, p[:2]
    assert p[8]["room_next"] == p[8]["room_own"] and p[9]["room_next"] > p[9]["room_own"]
    return [c]


def _straddle_cases():
    """a stored block of 31 / 32 / 33 bytes in front of a linked compressed block whose first match begins in the stored bytes and
    ends in the batch's own literals: op - dst_lo is 31, 32, 33 at the batch start.  These cases run the DIRECT path, and nothing else
    can: the executor's guard `op - dst_lo >= SEQ_ASM_PRE` (a straddling source needs 32 bytes of history in front of an assembly) is
    never at its edge in an assembled LZ4 batch.  dst_lo is fixed for a block, so only a block's first batch begins less than 32 bytes
    behind it, and a chunk's first batch is never assembled (its output + 48 is more than its input: lz4_wave.h); every later batch
    begins at least 64 x 4 bytes of output further on.  test_the_blocks_sit_on_the_edges_they_mean_to asserts both on the model.  The
    assembled straddle (history bytes loaded, op - dst_lo large) is batch 2 of the room cases."""
    out = []
    for n in (31, 32, 33):
        b = Block(15 + n, history=n)
        b.seq(6, 14, 16).seq(3, 8, 30).fill(40)
        data = b.done()
        frame, at = _frame([("s", bytes(range(n))), ("c", data)], linked=True)
        out.append(dict(label="straddle, %d bytes in front" % n, frame=frame, offs=[at[1] + p for p in b.off_pos], left=False, straddle=True,
                        plan=M.plan(np.frombuffer(data, dtype=np.uint8))))
    return out


def _piece_cases(left):
    """pieces of 32, 33, 48, 64, 65 bytes — a literal run, a plain match, a self-overlapping match — first, in the middle and last in
    batch 2 of a block whose batch 2 has the room"""
    out = []

    def block(kind, n, off, at, seed):
        b = Block(seed)
        b.seq(14, 4)
        b.fill(63, ll=(10, 12), ml=(4, 6))
        for i in range(64):
            if i != at: b.seq(1, 4)
            elif kind == "lit": b.seq(n, 4)
            else: b.seq(2, n, off)
        b.fill(20)
        if left: b.run()
        data = b.done()
        c = _case("%s %d off %s at %d" % (kind, n, off, at), b, data, left)
        p = c["plan"][1]
        assert p["first"] == 64 and p["total"] + 48 <= p["room_next"], p
        return c
    seed = 100
    for at in (0, 31, 63):
        for n in (32, 33, 48, 64, 65):
            seed += 1
            out.append(block("lit", n, None, at, seed))
            out.append(block("match", n, 200, at, seed))
            for off in (1, 2, 7, 15, 16, 17, n - 1):
                out.append(block("self", n, off, at, seed))
    # two pieces in one batch, the second reading the first
    for n in (33, 48, 65):
        for second in ("match", "self16", "self7"):
            b = Block(300 + n)
            b.seq(14, 4)
            b.fill(63, ll=(10, 12), ml=(4, 6))
            for i in range(64):
                if i == 10: b.seq(n, 4)                                          # a long literal run ...
                elif i == 11 and second == "match": b.seq(1, n, n + 5)           # ... copied whole by a long plain match
                elif i == 11 and second == "self16": b.seq(1, 2 * n, 16)         # ... its tail repeated with period 16
                elif i == 11: b.seq(1, 2 * n, 7)
                elif i == 12: b.seq(0, 20, 24)                                   # and a short match reading the second piece
                else: b.seq(1, 4)
            b.fill(20)
            if left: b.run()
            out.append(_case("literal %d then %s" % (n, second), b, b.done(), left))
    return out


@pytest.fixture(scope="module")
def codec():
    return zpack_amd.Codec(0)


@pytest.fixture(scope="module")
def cases():
    hot = _room_cases(False) + _window_cases(False) + _straddle_cases() + _piece_cases(False)
    left = _room_cases(True) + _window_cases(True) + _piece_cases(True)
    o = oracle()
    for c in hot + left:
        rc, plain = o.lz4f_decode(c["frame"], 1 << 17)
        assert rc == 0 and 0 < len(plain) <= 65536 + 64, (c["label"], rc, len(plain))
        c["plain"] = plain
        c["hash"] = dg.xxh3(np.frombuffer(plain, dtype=np.uint8))
        assert (len(c["frame"]) < (len(plain) >> 3)) == c["left"], (c["label"], len(c["frame"]), len(plain))
    return hot, left


def test_the_blocks_sit_on_the_edges_they_mean_to(cases):
    """the model's verdict on the tuned blocks: on both sides of `total + 48 <= room`, for the room of this rule and for the old one"""
    hot, left = cases
    seen = set()
    for c in hot + left:
        if "target" in c:
            p = c["plan"][c["target"]]
            rule = "own" if c["label"].startswith("old room") else "next"
            d = p["total"] + 48 - p["room_" + rule]
            assert d in (-1, 0, 1) and not (p["lit_long"] or p["match_long"] or p["self16"] or p["self1"]), (c["label"], p)
            assert M.assembled(p, "next", True) == (d <= 0 or rule == "own"), (c["label"], p)
            if rule == "next" and d <= 0:            # the assembly covers the batch's own input: it ends 16 bytes short of the room
                assert p["total"] + 32 > p["room_own"] + 64, (c["label"], p)
            seen.add((c["label"].split(" d=")[0], d, c["left"]))
    assert len(seen) == 3 * 4 + 3 * 2, sorted(seen)
    # the 32 history bytes at the front of the assembly buffer never hold input of a batch that is assembled, and an assembled batch
    # begins at least 256 bytes of output behind the block's start (so `op - dst_lo >= SEQ_ASM_PRE` is never at its edge)
    for c in hot + left:
        for p in c["plan"]:
            assert not M.assembled(p, "next", True) or (p["room_own"] >= 32 and p["out"] >= 256), (c["label"], p)
    straddle = [c for c in hot if c.get("straddle")]
    assert len(straddle) == 3
    for c in straddle:          # one batch, the chunk's first: direct
        assert len(c["plan"]) == 1 and c["plan"][0]["room_own"] == 0 and not M.assembled(c["plan"][0], "next", True), c["plan"]


def _run(codec, cs, uncomp=None, caps=None):
    frames = [c["frame"] for c in cs]
    uncomp = uncomp or [len(c["plain"]) for c in cs]
    caps = caps or uncomp
    hashes = [c["hash"] for c in cs]
    arc, offs = _assemble(frames, uncomp, hashes)
    desc, r, out, st = _device_batch(codec, arc, offs, [len(f) for f in frames], uncomp, caps, hashes, 0, fill=0)
    return arc, offs, desc, r, out, st


def _judge(cs, arc, offs, desc, r, out, uncomp, caps):
    """status of every entry, and bytes and produced size of every entry that decodes, are the oracle's"""
    o = oracle()
    bad = []
    for i, c in enumerate(cs):
        rc, want, got, _ = o.entry_decode(arc, offs[i], len(c["frame"]), uncomp[i], c["hash"], 2, caps[i])
        a = int(desc[i]["dst_offset"])
        if int(r[i]["status"]) != rc:
            bad.append((c["label"], "status", int(r[i]["status"]), rc))
        elif rc in (0, 15):
            if int(r[i]["produced"]) != got:
                bad.append((c["label"], "produced", int(r[i]["produced"]), got))
            elif out[a:a + uncomp[i]].tobytes() != want[:uncomp[i]]:
                w = np.frombuffer(want[:uncomp[i]], dtype=np.uint8)
                bad.append((c["label"], "first bad byte", int(np.nonzero(out[a:a + uncomp[i]] != w)[0][0]), "of", uncomp[i]))
    return bad


@pytest.mark.parametrize("which", ["k_lz4_wave", "k_lz4_left"])
def test_intact_frames_decode_to_the_oracles_bytes(codec, cases, which):
    cs = cases[0] if which == "k_lz4_wave" else cases[1]
    assert len(cs) >= 150
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
            # an offset field of the batch under test (the second batch: sequences 64 ..), or of the block's middle
            k = min(len(c["offs"]) - 1, 64 + 31) if len(c["offs"]) > 80 else len(c["offs"]) // 2
            f = bytearray(c["frame"])
            f[c["offs"][k]:c["offs"][k] + 2] = b"\x00\x00" if damage == "offset 0" else b"\xff\xff"
            c["frame"] = bytes(f)
        cs.append(c)
    n = [len(c["plain"]) for c in cs]
    uncomp = [x - 1 for x in n] if damage == "entry one byte short" else n
    caps = [x - 1 for x in n] if damage.endswith("short") else n
    arc, offs, desc, r, out, st = _run(codec, cs, uncomp, caps)
    assert (r["status"] != 0).sum() >= len(cs) - 8, "the damage was not felt"      # (offset 0xFFFF is legal once 65535 bytes exist)
    assert _judge(cs, arc, offs, desc, r, out, uncomp, caps) == []
