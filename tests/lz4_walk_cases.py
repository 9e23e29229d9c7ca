"""Hand-built LZ4 blocks that put the fix-up rounds of the chunk parse (lz4_block_wave, lz4_wave.h) on the edges of the one-successor
continuation.  Shared by tests/test_lz4_walk_model_cpu.py (the CPU model, tools/sim/lz4_walk_cont_sim.py) and
tests/test_gpu_lz4_walk_cont.py (the device against the oracle).  Not a test module.

The blocks are made of 3-byte sequences (no literals, match 4..18, offset below 256): the high offset byte 0x00 reads as a valid token
of another 3-byte sequence, so a walk that starts on it stays on a false chain for good.  The head sequence is 16 bytes long, so the
true tokens sit at positions = 1 (mod 3) and every lane's run-in (a multiple of 60 bytes into the chunk) starts on a 0x00: every
segment behind lane 0 is mis-synced, the truth moves on by re-walks that never merge, and the continuation carries it one lane
further in each round."""
import importlib.util
import os

from tests.test_gpu_lz4_asm_batches import Block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG, CHUNK = 60, 3840


def model():
    spec = importlib.util.spec_from_file_location("lz4_walk_cont_sim", os.path.join(ROOT, "tools", "sim", "lz4_walk_cont_sim.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert (m.SEG, m.CHUNK) == (SEG, CHUNK)
    return m


def _head(seed):
    """a block that begins with a 16-byte sequence: 13 literals, a match of 4"""
    return Block(seed).seq(13, 4, 7)


def _threes(b, n):
    for _ in range(n):
        b.seq(0, int(b.rng.integers(4, 19)), int(b.rng.integers(1, min(b.n, 255) + 1)))
    return b


def _threes_to(b, pos):
    """3-byte sequences until the next token sits at block position `pos`"""
    assert pos >= len(b.d) and (pos - len(b.d)) % 3 == 0, (pos, len(b.d))
    return _threes(b, (pos - len(b.d)) // 3)


def _case(label, b, data, want, **marks):
    return dict(label=label, blk=b, data=data, want=want, off_pos=list(b.off_pos), **marks)


def false_chains(seed=1, nbytes=2 * CHUNK + 600):
    """(a) more than two chunks of phase-locked false chains"""
    b = _threes(_head(seed), (nbytes - 16) // 3)
    return _case("a: 3-byte sequences, %d bytes" % nbytes, b, b.done(), ("continued", "ran_to_end"))


def jumped_over(seed=2, lane=20, run=100):
    """(b) behind a mis-synced stretch a literal run that starts in lane `lane` and ends two lanes on: the re-walk's new exit lies behind
    the successor's whole segment and the continuation is refused"""
    assert 61 <= run <= 130
    b = _threes_to(_head(seed), SEG * lane + 40)
    tok = len(b.d)
    b.seq(run, 5)
    assert tok // SEG == lane and len(b.d) // SEG == lane + 2, (tok, len(b.d))
    _threes(b, 900)
    return _case("b: literal run of %d from lane %d to lane %d" % (run, lane, lane + 2), b, b.done(), ("refused",), long_tok=tok)


def one_chunk(delta, seed=3):
    """(c) a block of CHUNK + delta bytes: the chunk's last active lane is a short segment, or the lane behind it is not active"""
    total = CHUNK + delta
    tail = 5 + (total - 16 - 1 - 5) % 3                         # 16 + 3 n + 1 + tail == total
    b = _threes(_head(seed + (delta & 0xFF)), (total - 16 - 1 - tail) // 3)
    data = b.done(tail)
    assert len(data) == total, (len(data), total)
    return _case("c: one chunk %+d" % delta, b, data, ("continued",), total=total)


def last_sequence_in_successor(seed=4, lane=20):
    """(d) the block's last (literal-only) sequence lies in lane `lane`'s segment; the caller picks a lane that a continuation reaches"""
    b = _threes_to(_head(seed), SEG * lane + 31)
    tok = len(b.d)
    return _case("d: last sequence in lane %d" % lane, b, b.done(12), ("continued", "met_flag"), last_tok=tok)


def long_lengths_in_successor(seed=5, lane=20):
    """(e) a literal run of 300 and, two lanes on behind it, a match of 300 (two length-extension bytes each: the general token decoder)"""
    b = _threes_to(_head(seed), SEG * lane + 10)
    t1 = len(b.d)
    b.seq(300, 6)
    _threes(b, 60)
    t2 = len(b.d)
    b.seq(0, 300, 200)
    _threes(b, 700)
    return _case("e: literal run 300 in lane %d, match 300" % lane, b, b.done(), ("continued",), long_toks=(t1, t2))


def long_run(seed=6):
    """(g) false chains, then one long byte run: the entry compresses below an eighth"""
    b = _threes(_head(seed), 1400)
    b.run()
    return _case("g: false chains and a long run", b, b.done(), ("continued", "ran_to_end"), left=True)


def reached_by_continuation(M, build, lanes, key):
    """the first of build(lane=...) whose marked token(s) `key` the model's continuations visit"""
    for lane in lanes:
        c = build(lane=lane)
        seen = set()
        for ch in M.parse_block(list(c["data"]), "call"):
            seen |= ch["cont_visits"]
        toks = c[key] if isinstance(c[key], tuple) else (c[key],)
        if any(t in seen for t in toks):
            c["cont_visits"] = seen
            return c
    raise AssertionError("no lane of %s puts %s on a continuation" % (list(lanes), key))


def intact_cases(M):
    cs = [false_chains(), jumped_over()]
    cs += [one_chunk(d) for d in (0, 1, -1, 59, -59, 61, -61)]
    cs.append(reached_by_continuation(M, last_sequence_in_successor, (20, 21, 22, 23), "last_tok"))
    cs.append(reached_by_continuation(M, long_lengths_in_successor, (20, 21, 22, 23), "long_toks"))
    cs.append(long_run())
    return cs
