#!/usr/bin/env python3
"""CPU model of the fix-up rounds of the LZ4 chunk parse (lz4_block_wave, lz4_wave.h) with the ONE-SUCCESSOR CONTINUATION: a re-walk
that leaves its own segment unmerged, with a new exit inside the next lane's segment, goes on through that segment against the
successor's visited mask as of the round's start and hands the result over (the successor's record and entry are replaced at the end
of the round; the hand-over wins over the successor's own re-walk of that round, which started from an exit that has just changed).
Counts wave iterations (a wave iterates max-over-lanes times) per chunk.  Developer tool, no GPU.

  rule "parent"  the fix-up rounds without continuation (lz4_walk_sim.py's "neigh", -DLZ4W_FIX_CONT=0)
  rule "call"    the continuation as a second pass through the walk, behind the lanes' own re-walks (the form that is built)
  rule "loop"    the continuation inside the same walk loop (a lane's hops of both segments add up)

Per chunk the model ASSERTS that the union of the lanes' masks is the serial chain and that the last lane's exit is the chain's.
It counts four events: a continuation, a merge inside the successor, a run to the successor's end (or a flagged hop there), and a
refusal (the new exit jumps over the successor's segment, or there is no active successor); per chunk it also keeps the positions the
continuations visited (`cont_visits`) and how many of them met the block's last sequence or a malformed one (`met_flag`).

  tools/sim/lz4_walk_cont_sim.py [mix] [entries]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lz4_walk_sim import SEG, NL, CHUNK, blocks_of, hop, walk          # noqa: E402

RULES = ("parent", "call", "loop")
EVENTS = ("continued", "merged_in_successor", "ran_to_end", "refused")


def serial_chain(d, C):
    """token positions of the block's chain, and where it ends (C for a well-formed block)"""
    pos, p = [], 0
    while p < C:
        pos.append(p)
        p, fl = hop(d, C, p)
        if fl:
            break
    return pos, p


def parse_block(d, rule, runin=SEG):
    """d: list of the block's bytes.  -> list of per-chunk dicts (cpos, it_first, it_fix, rounds, calls, the four events, met_flag,
    cont_visits)"""
    assert rule in RULES
    C = len(d)
    chain, chain_end = serial_chain(d, C)
    chain_set = set(chain)
    out, cpos = [], 0
    while cpos < C:
        tok_end = min(C, cpos + CHUNK)
        st = dict(cpos=cpos, it_first=0, it_fix=0, rounds=0, calls=0, met_flag=0, cont_visits=set(), **{k: 0 for k in EVENTS})
        lanes = []                                                # [start, end, visited, exit, entry]
        for l in range(NL):
            s = cpos + l * SEG
            if s >= tok_end:
                break
            e = min(s + SEG, tok_end)
            vis, ex, it, entry = walk(d, C, s if l == 0 else max(cpos, s - runin), s, e, None)
            lanes.append([s, e, vis, ex, entry])
            st["it_first"] = max(st["it_first"], it)
        while True:
            st["rounds"] += 1
            es = [cpos] + [lanes[k - 1][3] for k in range(1, len(lanes))]
            ch = [k for k in range(len(lanes)) if es[k] != lanes[k][4]]
            if not ch:
                break
            start = [list(x) for x in lanes]                      # the records as of the round's start
            own_it, cont_it, hand = {}, {}, {}
            for k in ch:
                s, e, vis, ex, _ = start[k]
                nv, nex, it, _ = walk(d, C, es[k], s, e, (vis, ex))
                lanes[k] = [s, e, nv, nex, es[k]]
                own_it[k] = it
                if rule == "parent" or nex == ex:                 # (an exit that did not change leaves the successor's entry right)
                    continue
                if k + 1 >= len(lanes) or nex >= start[k + 1][1]:
                    st["refused"] += 1
                    continue
                s2, e2, vis2, ex2, _ = start[k + 1]
                hv, hex_, it2, _ = walk(d, C, nex, s2, e2, (vis2, ex2))
                st["continued"] += 1
                merged, seen, flagged = _continuation(d, C, nex, s2, e2, vis2)
                st["merged_in_successor" if merged else "ran_to_end"] += 1
                st["met_flag"] += flagged
                st["cont_visits"] |= seen
                cont_it[k] = it2
                hand[k + 1] = [s2, e2, hv, hex_, nex]
            for k, rec in hand.items():                           # the hand-over wins over the successor's own re-walk
                lanes[k] = rec
            if rule == "loop":
                st["it_fix"] += max(own_it[k] + cont_it.get(k, 0) for k in ch)
                st["calls"] += 1
            else:
                st["it_fix"] += max(own_it.values()) + (max(cont_it.values()) if cont_it else 0)
                st["calls"] += 2 if cont_it else 1
        # the fixed point is the serial chain
        union = set()
        for s, e, vis, ex, _ in lanes:
            assert all(s <= p < e for p in vis)
            union |= vis
        want = {p for p in chain_set if cpos <= p < tok_end}
        assert union == want, ("masks differ from the serial chain", cpos, sorted(union ^ want)[:8])
        nxt = [p for p in chain if p >= tok_end]
        want_exit = nxt[0] if nxt else chain_end
        ncp = lanes[-1][3]
        assert ncp == want_exit, ("the last lane's exit is not the chain's", cpos, ncp, want_exit)
        assert ncp > cpos
        out.append(st)
        if not nxt:
            break
        cpos = ncp
    return out


def _continuation(d, C, frm, s, e, vis):
    """the walk from `frm` through [s, e) against `vis` -> (it merged, the positions it visited itself, it met a flagged hop: the block's last
    sequence or a malformed one)"""
    p, seen = frm, set()
    while p < e:
        if p in vis:
            return True, seen, 0
        seen.add(p)
        p, fl = hop(d, C, p)
        if fl:
            return False, seen, 1
    return False, seen, 0


def totals(chunks):
    t = dict(chunks=len(chunks))
    for k in ("it_first", "it_fix", "rounds", "calls", "met_flag") + EVENTS:
        t[k] = sum(c[k] for c in chunks)
    t["max_rounds"] = max(c["rounds"] for c in chunks)
    return t


def entry_blocks(mix, n, seed=1, size=65536):
    from benchdata import datagen as dg
    b = dg.Batch(n, size, size, method=dg.LZ4, level=0, seed=seed, mix=mix)
    for i in range(n):
        fr = b.archive[int(b.offsets[i]):int(b.offsets[i]) + int(b.comp_sizes[i])]
        for blk in blocks_of(fr):
            yield blk.tolist()


def run(mix, n, rule):
    chunks = []
    for d in entry_blocks(mix, n):
        chunks += parse_block(d, rule)
    t = totals(chunks)
    c = t["chunks"]
    print("mix %d %-6s: chunks %d  first-walk its/chunk %.1f  fix its/chunk %.1f  rounds/chunk %.2f  walk calls/chunk %.2f  all its/chunk %.1f" % (
        mix, rule, c, t["it_first"] / c, t["it_fix"] / c, t["rounds"] / c, t["calls"] / c, (t["it_first"] + t["it_fix"]) / c))
    if rule != "parent":
        print("           per chunk: continued %.2f  merged in the successor %.2f  ran to its end %.2f  refused %.2f" % tuple(t[k] / c for k in EVENTS))
    return t


if __name__ == "__main__":
    mix = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    for rule in RULES:
        run(mix, n, rule)
