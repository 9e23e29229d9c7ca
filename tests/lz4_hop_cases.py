"""Hand-built LZ4 blocks for the hop loops of lz4_walk (lz4_wave.h): where a re-walk merges, lanes that never start, run-ins that give
up, length extensions of exactly 255, an offset field at the staged limit, chunks of 1 / 64 / 64 + segments.  Shared by
tests/test_gpu_lz4_hops.py; not a test module.

Every block is built under BOTH CUTS of the chunk boundary the existing walk cases use (tests/lz4_walk_cases.py, tests/
test_gpu_lz4_asm_batches.py): "first" puts the case in the block's first chunk (cpos = 0, behind a 16-byte head sequence), "second"
behind a literal run of 3900 bytes, which is a chunk of its own, so the case's chunk starts at cpos = 3919: segment boundaries,
run-in starts and the staged limit all move by 19 bytes (mod 60) against the tokens.

trace() is a CPU model of the parse that RECORDS what the walks do (the rounds are those of tools/sim/lz4_walk_cont_sim.py, rule
"call"; hop() is the model's), so that every case can assert it sits on the event it means to."""
import numpy as np

from tests import lz4_walk_cases as W
from tests.test_gpu_lz4_asm_batches import Block

SEG, CHUNK, NL = W.SEG, W.CHUNK, 64
CUTS = ("first", "second")


def _walk(hop, d, C, frm, s, e, old, ev, kind, lane):
    """lz4_walk_sim.walk with a record of events: (kind, lane, what, position relative to s)"""
    p, vis, entry = frm, set(), None
    if frm >= e:
        ev.append((kind, lane, "never_started", frm - s))
    while p < e:
        if p >= s:
            if entry is None:
                entry = p
            if old is not None and p in old[0]:
                last = max(x for x in old[0])
                ev.append((kind, lane, "merged", p - s))
                if p == last:
                    ev.append((kind, lane, "merged_on_last_token", p - s))
                return vis | {x for x in old[0] if x >= p}, old[1], entry
            vis.add(p)
        nx, fl = hop(d, C, p)
        if fl and p < s:
            ev.append((kind, lane, "runin_gave_up_malformed" if fl == 1 else "runin_gave_up_last", p - s))
            nx = s
        elif fl:
            ev.append((kind, lane, "flagged_malformed" if fl == 1 else "flagged_last", p - s))
            p = nx
            break
        p = nx
    if old is not None and frm < e:
        ev.append((kind, lane, "never_merged", frm - s))
    if entry is None:
        entry = p
    return vis, p, entry


def trace(M, data):
    """-> [(cpos, number of active lanes, events)] per chunk of the block `data`"""
    d = list(data)
    C = len(d)
    out, cpos = [], 0
    while cpos < C:
        tok_end = min(C, cpos + CHUNK)
        ev, lanes = [], []
        for l in range(NL):
            s = cpos + l * SEG
            if s >= tok_end:
                break
            e = min(s + SEG, tok_end)
            vis, ex, entry = _walk(M.hop, d, C, s if l == 0 else max(cpos, s - SEG), s, e, None, ev, "first", l)
            lanes.append([s, e, vis, ex, entry])
        for _ in range(200):
            es = [cpos] + [lanes[k - 1][3] for k in range(1, len(lanes))]
            ch = [k for k in range(len(lanes)) if es[k] != lanes[k][4]]
            if not ch:
                break
            start = [list(x) for x in lanes]
            hand = {}
            for k in ch:
                s, e, vis, ex, _ = start[k]
                nv, nex, _ = _walk(M.hop, d, C, es[k], s, e, (vis, ex), ev, "own", k)
                lanes[k] = [s, e, nv, nex, es[k]]
                if nex == ex or k + 1 >= len(lanes) or nex >= start[k + 1][1]:
                    continue
                s2, e2, vis2, ex2, _ = start[k + 1]
                hv, hex_, _ = _walk(M.hop, d, C, nex, s2, e2, (vis2, ex2), ev, "cont", k + 1)
                hand[k + 1] = [s2, e2, hv, hex_, nex]
            for k, rec in hand.items():
                lanes[k] = rec
        out.append((cpos, len(lanes), ev))
        nxt = lanes[-1][3]
        assert nxt > cpos
        if nxt >= C:
            break
        cpos = nxt
    return out


def events(M, data, chunk=None):
    """the set of (kind, what) and (kind, what, rel) over the block's chunks (or of chunk number `chunk`)"""
    seen = set()
    for i, (_, _, ev) in enumerate(trace(M, data)):
        if chunk is None or i == chunk:
            for kind, _, what, rel in ev:
                seen.add((kind, what))
                seen.add((kind, what, rel))
                seen.add(what)
    return seen


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def start(seed, cut):
    """-> (Block, base): the case's chunk starts at block position `base`; the next token sits at base + 1 (mod 3), so that behind
    3-byte sequences every run-in (a multiple of 60 bytes into the chunk) starts on the high offset byte 0x00: a false chain for good"""
    assert cut in CUTS
    if cut == "first":
        return Block(seed).seq(13, 4, 7), 0
    b = Block(seed).seq(3900, 4, 7)
    base = len(b.d)
    assert base == 3919
    return b.seq(1, 4, 3), base


def three(b):
    return b.seq(0, int(b.rng.integers(4, 19)), int(b.rng.integers(1, min(b.n, 255) + 1)))


def threes_to(b, pos):
    """3-byte sequences until the next token sits at block position `pos` (same phase)"""
    assert pos >= len(b.d) and (pos - len(b.d)) % 3 == 0, (pos, len(b.d))
    while len(b.d) < pos:
        three(b)
    return b


def mixed(b, n):
    """n short sequences of 3..7 bytes with random literals: false chains that join the true one after a few hops, anywhere"""
    for _ in range(n):
        b.seq(int(b.rng.integers(0, 5)), int(b.rng.integers(4, 19)), int(b.rng.integers(1, min(b.n, 255) + 1)))
    return b


def case(label, cut, b, data, want, chunk=None):
    return dict(label="%s [%s cut]" % (label, cut), data=data, want=tuple(want), chunk=chunk, off_pos=list(b.off_pos))


def phase_locked(cut, seed=1):
    """more than a chunk of phase-locked false chains: re-walks that never merge"""
    b, base = start(seed, cut)
    threes_to(b, len(b.d) + 3 * ((CHUNK + 600) // 3))
    return case("phase-locked 3-byte sequences", cut, b, b.done(), [("own", "never_merged"), ("cont", "never_merged")])


def merging(cut, seed):
    """short sequences with random literal bytes: the search in the test module's comment picked seeds whose re-walks merge on position
    0 of a segment and on a segment's last token position"""
    b, base = start(seed, cut)
    mixed(b, 700)
    return b, b.done()


def jumped(cut, seed=3, lane=20):
    """a literal run of 70 bytes and a match with a length extension: the chain jumps over a whole segment, whose lane never starts"""
    b, base = start(seed, cut)
    threes_to(b, base + SEG * lane + 58)                 # the token two bytes before the segment's end: run and match fields cover lane + 1
    b.seq(70, 40)
    threes_to(b, len(b.d) + 900)
    return case("literal run of 70 over lane %d" % (lane + 1), cut, b, b.done(), ["never_started"])


def in_phase(b):
    """one 5-byte sequence: the true chain moves from position 1 to position 0 (mod 3) of the chunk, where the run-ins start — from here
    on every run-in walks the true chain"""
    return b.seq(2, 4, int(b.rng.integers(1, min(b.n, 255) + 1)))


EXT = {"254": 254, "255 + 0": 255, "255 + 255 + 0": 510}


def ext255(cut, side, where, kind, seed=4, lane=12):
    """a length whose extension bytes are 254 (the last the branch-free decode takes), 255 + 0 (exactly 255: the general decoder), 255
    + 255 + 0, on the literal or the match side.  `run-in`: the true chain is in phase with the run-ins, so the next lane's run-in
    meets the token before its segment; `segment`: behind phase-locked false chains only walks inside the segment (re-walks) meet it"""
    b, base = start(seed + len(kind) + (2 if side == "match" else 0), cut)
    if where == "run-in":
        in_phase(b)
        threes_to(b, base + SEG * lane + 39)
    else:
        threes_to(b, base + SEG * lane + 4)
    n = 15 + EXT[kind]
    if side == "literal":
        b.seq(n, 5)
    else:
        b.seq(0, n + 4, 200)
    mixed(b, 300)
    return case("%s length extension %s in a %s" % (side, kind, where), cut, b, b.done(), [])


def runin_meets(cut, what, seed=6):
    """a block that ends behind a run-in that walks the true chain: lane 10's run-in meets the block's last sequence (`last`) or a token
    whose literal run does not fit the block (`malformed`: the block cut six bytes short) and gives up"""
    b, base = start(seed, cut)
    in_phase(b)
    threes_to(b, base + SEG * 9 + 30)
    data = b.done(40)                                    # the last sequence's token sits in lane 9, its literals end in lane 10
    if what == "malformed":
        data = data[:-6]
    return case("run-in meets %s" % what, cut, b, data, [("first", "runin_gave_up_" + what)])


def staged_limit(cut, delta, seed=7):
    """a sequence whose offset field ends `delta` bytes past the end of the staged bytes (chunk + 64 bytes of slack): 0 = exactly at
    the limit (the branch-free decode takes it), 1 = one byte past (the general decoder reads memory)"""
    b, base = start(seed, cut)
    lim = base + CHUNK + 64
    # a token in the chunk's last lane with a literal run that carries its offset field to the limit
    threes_to(b, base + SEG * 63 + 40)
    tok = len(b.d)
    ll = lim + delta - 2 - (tok + 1)                      # token, ll literals (ll < 15: no extension byte), offset at [lim + delta - 2, lim + delta)
    ext = 0 if ll < 15 else 1 + (ll - 15) // 255
    ll -= ext
    b.seq(ll, 6)
    assert b.off_pos[-1] + 2 == lim + delta, (b.off_pos[-1], lim, delta)
    mixed(b, 200)
    return case("offset field ends %d past the staged limit" % delta, cut, b, b.done(), [])


def sized(cut, nbytes, seed=8):
    """a case chunk of exactly `nbytes` bytes (1 segment, 64 segments, 64 segments + 1 byte)"""
    b, base = start(seed + nbytes % 97, cut)
    total = base + nbytes
    tail = 5 + (total - len(b.d) - 1 - 5) % 3
    threes_to(b, total - 1 - tail)
    data = b.done(tail)
    assert len(data) == total, (len(data), total)
    return case("chunk of %d bytes" % nbytes, cut, b, data, [])
