"""The CPU model of the chunk parse's fix-up rounds with the one-successor continuation (tools/sim/lz4_walk_cont_sim.py): a re-walk
that leaves its segment unmerged with a new exit inside the next lane's segment goes on through that segment and hands the result
over.  The model itself asserts, per chunk, that the lanes' masks are the serial chain and that the last lane's exit is the chain's;
here it runs over seeded benchmark entries of both classes and over the hand-built blocks of tests/lz4_walk_cases.py, for the form
that is built ("call": the continuation as a second pass through the walk) and the in-loop form ("loop")."""
import pytest

from tests import lz4_walk_cases as W

M = W.model()


@pytest.fixture(scope="module")
def seeded():
    """mix -> rule -> per-chunk results of four 64 KiB entries (text = 0, records = 1)"""
    out = {}
    for mix in (0, 1):
        blocks = list(M.entry_blocks(mix, 4))
        out[mix] = {rule: [c for d in blocks for c in M.parse_block(d, rule)] for rule in M.RULES}      # (asserts the chain per chunk)
    return out


@pytest.fixture(scope="module")
def built():
    cs = W.intact_cases(M)
    for c in cs:
        c["chunks"] = {rule: M.parse_block(list(c["data"]), rule) for rule in M.RULES}
    return cs


def test_seeded_entries_fewer_iterations_and_bounded_rounds(seeded):
    for mix in (0, 1):
        t = {rule: M.totals(seeded[mix][rule]) for rule in M.RULES}
        print(mix, t)
        assert t["parent"]["chunks"] == t["call"]["chunks"] == t["loop"]["chunks"] >= 30
        for rule in M.RULES:
            assert t[rule]["max_rounds"] <= 64, (mix, rule, t[rule])
            assert t[rule]["it_first"] == t["parent"]["it_first"]
        assert t["call"]["it_fix"] < t["parent"]["it_fix"] and t["loop"]["it_fix"] < t["parent"]["it_fix"], (mix, t)
        assert t["call"]["rounds"] < t["parent"]["rounds"], (mix, t)
        assert t["parent"]["continued"] == 0 and t["call"]["continued"] > 0
        # every continuation either merges or runs to the successor's end
        assert t["call"]["continued"] == t["call"]["merged_in_successor"] + t["call"]["ran_to_end"]
    # the four events all occur on seeded data
    both = M.totals(seeded[0]["call"] + seeded[1]["call"])
    assert all(both[k] > 0 for k in M.EVENTS), both


def test_hand_built_blocks_produce_their_events(built):
    assert len(built) == 12
    for c in built:
        for rule in M.RULES:
            t = M.totals(c["chunks"][rule])
            assert t["max_rounds"] <= 64, (c["label"], rule, t)
        t, p = M.totals(c["chunks"]["call"]), M.totals(c["chunks"]["parent"])
        print(c["label"], t, "parent rounds", p["rounds"], "iterations", p["it_fix"])
        for ev in c["want"]:
            assert t[ev] >= 1, (c["label"], ev, t)
        # (a pure false chain costs a whole segment's hops per call under either rule: fewer rounds, not fewer iterations)
        assert t["rounds"] < p["rounds"], (c["label"], t, p)


def test_hand_built_blocks_sit_where_they_mean_to(built):
    by = {c["label"][0]: [] for c in built}
    for c in built:
        by[c["label"][0]].append(c)
    assert sorted(by) == ["a", "b", "c", "d", "e", "g"] and len(by["c"]) == 7
    a = by["a"][0]
    assert len(a["data"]) > 2 * W.CHUNK and len(a["chunks"]["call"]) >= 3
    # (a) phase-locked: the parent's rule needs a round per lane in a whole chunk, the continuation halves them
    first = a["chunks"]["parent"][0], a["chunks"]["call"][0]
    assert first[0]["rounds"] >= 60 and first[1]["rounds"] <= first[0]["rounds"] // 2 + 2, first
    # (b) the long literal run is hopped over by a re-walk whose continuation is refused
    b = by["b"][0]
    d = list(b["data"])
    nxt, fl = M.hop(d, len(d), b["long_tok"])
    assert fl == 0 and b["long_tok"] // W.SEG + 2 == nxt // W.SEG
    # (c) the last active lane of the first chunk: 60, 60 (+1: a second chunk), 59, 59 (+59), 1, 1 (+61), 59 bytes in lane 62
    for c in by["c"]:
        n = c["total"]
        first_end = min(n, W.CHUNK)
        lanes = -(-first_end // W.SEG)
        assert (lanes, first_end - (lanes - 1) * W.SEG) == {3840: (64, 60), 3841: (64, 60), 3839: (64, 59), 3899: (64, 60), 3781: (64, 1),
                                                            3901: (64, 60), 3779: (63, 59)}[n], c["label"]
        # (+1: the last sequence's token still lies in the first chunk, its literals end the block)
        assert len(c["chunks"]["call"]) == (2 if n > W.CHUNK + 8 else 1), c["label"]
    # (d) the last sequence's token, (e) one of the two long tokens is visited by a continuation
    assert by["d"][0]["last_tok"] in by["d"][0]["cont_visits"]
    e = by["e"][0]
    assert any(t in e["cont_visits"] for t in e["long_toks"])
    d = list(e["data"])
    t1, t2 = e["long_toks"]                                       # two length-extension bytes each: 15 + 255 + ...
    assert d[t1] >> 4 == 15 and d[t1 + 1] == 255 and M.hop(d, len(d), t1)[0] - t1 >= 270
    assert d[t2] == 0x0F and d[t2 + 3] == 255 and M.hop(d, len(d), t2)[0] == t2 + 5
    assert by["g"][0]["left"]
