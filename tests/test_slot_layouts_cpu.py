"""tests/slot_layouts.py before it goes near a GPU: the layouts are what they say, the guard check reports a single stray byte wherever it
falls — and keeps quiet about the inside of a live slot — and the case lists of tests/test_gpu_slot_confinement.py are inputs on which
the oracle alone has a verdict, mostly intact, with enough damage among them."""
import numpy as np
import pytest

import zpack_amd
from tests import slot_layouts as S


@pytest.fixture(scope="module")
def groups(golden_dir):
    return S.groups(golden_dir)


@pytest.fixture(scope="module")
def batches(groups):
    return {name: S.assemble(cs) for name, cs in groups.items()}


# ---- the layouts ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", S.LAYOUTS)
def test_layouts_are_what_they_say(batches, layout):
    for name, (arc, desc) in batches.items():
        caps = desc["dst_capacity"].astype(np.int64)
        p = S.lay_out(caps, layout)
        lo = p.dst_offset.astype(np.int64)
        hi = lo + caps
        assert p.lead >= S.GUARD and p.tail >= S.GUARD
        assert lo.min() >= 0 and hi.max() <= p.dst_size, (name, "a slot leaves the slice")
        order = np.argsort(lo, kind="stable")
        live = order[caps[order] > 0]                                    # (an empty slot overlaps nothing)
        assert (hi[live][:-1] <= lo[live][1:]).all(), (name, "two slots overlap")
        gaps = lo[live][1:] - hi[live][:-1]
        if layout == "aligned":
            assert (lo % 256 == 0).all() and p.lead % 256 == 0 and (gaps >= 64).all() and p.dst_size - hi.max() >= 256
            continue
        assert p.dst_size == hi.max(), (name, "bytes behind the last slot inside dst")
        assert p.lead % 2 == 1, (name, "the slice itself begins at an odd address")
        assert S.covers(lo + p.lead), name
        if layout == "gapped":
            assert lo[0] == 1 and gaps.min() == 1 and set(gaps.tolist()) >= set(S.GAPS) - {0}, name
            assert [int(lo[i + 1] - hi[i]) for i in range(len(S.GAPS))] == list(S.GAPS), name
        else:
            assert lo.min() == 0 and caps.sum() == p.dst_size and (gaps == 0).all(), (name, "a packed layout has no byte between two slots")
            step = lo[1:] - lo[:-1]
            assert (step >= 0).all() if layout == "packed" else (step <= 0).all(), name


def test_a_small_batch_has_to_opt_out_of_the_residue_rule():
    big = S.big_cases()
    caps = [c["cap"] for c in big]
    with pytest.raises(AssertionError):
        S.lay_out(caps, "gapped")                                            # twelve entries cannot reach 32 residues mod 128 ...
    p = S.lay_out(caps, "gapped", cover=False)                               # ... and say so
    lo = p.dst_offset.astype(np.int64) + p.lead
    # what is asked of it instead: the slots of the entries worth the whole chip begin and end off a 4-byte boundary
    partial = {c["label"] for c, a, n in zip(big, lo.tolist(), caps) if a % 4 and (a + n) % 4}
    assert partial >= set(S.BIG_WHOLE_CHIP) and all(any(c["label"] == x for c in big) for x in S.BIG_WHOLE_CHIP), partial
    with pytest.raises(AssertionError):
        S.lay_out([256] * 64, "packed")                             # a batch that stays on a grid is turned away


def test_refuse_takes_every_second_entry_and_moves_nothing(batches):
    arc, desc = batches["stored"]
    d0 = S.placed_desc(desc, S.lay_out(desc["dst_capacity"], "packed"))
    seen = np.zeros(len(d0), dtype=int)
    for which in ("even", "odd"):
        d = S.refuse(d0, which)
        assert np.array_equal(d["dst_offset"], d0["dst_offset"])
        changed = np.nonzero(d["dst_capacity"] != d0["dst_capacity"])[0]
        assert all(int(i) % 2 == (0 if which == "even" else 1) for i in changed)
        assert np.array_equal(changed, np.nonzero(~S.is_live(d))[0])
        assert (d["dst_capacity"][changed] == d["uncomp_size"][changed] - 1).all()
        seen[changed] += 1
    assert ((seen == 1) == (d0["uncomp_size"] > 0)).all() and (seen == 0).sum() > 0          # an empty entry cannot be refused


# ---- the guard check bites ---------------------------------------------------------------------------------------------------------------

def _synthetic():
    """five entries in the gapped layout (gaps 1, 3, 8, 15), entry 2 refused"""
    caps = [40, 7, 100, 1, 33]
    p = S.lay_out(caps, "gapped", cover=False)
    d = np.zeros(len(caps), dtype=zpack_amd.DECODE_DESC)
    d["dst_capacity"] = caps
    d["uncomp_size"] = caps
    d = S.refuse(S.placed_desc(d, p), "even")
    d["dst_capacity"][[0, 4]] = d["uncomp_size"][[0, 4]]                                  # ... and only entry 2
    image = np.full(p.lead + p.dst_size + p.tail, 0xA5, dtype=np.uint8)
    return p, d, image


def test_the_guard_check_reports_one_stray_byte_wherever_it_falls():
    p, d, image = _synthetic()
    lo = [p.lead + int(x) for x in d["dst_offset"]]
    hi = [a + c for a, c in zip(lo, (40, 7, 100, 1, 33))]
    assert list(S.is_live(d)) == [True, True, False, True, True]
    assert S.outside_untouched(image, p.lead, d, 0xA5) == []
    for a, b in ((lo[0], hi[0]), (lo[1], hi[1]), (lo[3], hi[3]), (lo[4], hi[4])):           # a decoder writes its live slots: never reported
        image[a:b] = 0x11
    assert S.outside_untouched(image, p.lead, d, 0xA5) == []
    where = [("the last guard byte in front of a slot", lo[4] - 1, 4, 1, "front"),
             ("the first byte behind a slot", hi[1], 1, 1, "behind"),
             ("the one-byte gap", hi[0], 0, 1, "behind"),                                   # (both neighbours are 1 away: the first is named)
             ("the first byte of the front guard zone", 0, 0, lo[0], "front"),
             ("the last byte of the rear guard zone", len(image) - 1, 4, len(image) - hi[4], "behind"),
             ("the first byte of the refused slot", lo[2], 1, lo[2] - hi[1] + 1, "behind"),
             ("the last byte of the refused slot", hi[2] - 1, 3, lo[3] - (hi[2] - 1), "front"),
             ("the middle of the refused slot", lo[2] + 50, 1, lo[2] + 50 - hi[1] + 1, "behind"),
             ("the byte in front of the first slot: dst itself begins there", lo[0] - 1, 0, 1, "front")]
    for what, k, entry, dist, side in where:
        for value in (0xA4, 0x5A, 0x00):
            img = image.copy()
            img[k] = value
            assert S.outside_untouched(img, p.lead, d, 0xA5) == [(k, value, entry, dist, side)], what
            assert S.outside_untouched(img, p.lead, d, 0xA5, labels=list("abcde")) == [(k, value, "abcde"[entry], dist, side)], what
    # a stray byte that equals one fill is seen under the other: that is why every batch runs with both
    img = image.copy()
    img[hi[1]] = 0xA5
    assert S.outside_untouched(img, p.lead, d, 0xA5) == []
    img[image == 0xA5] = 0x5A                                                               # the same run under the other fill ...
    img[hi[1]] = 0xA5                                                                       # ... and the same stray byte
    assert S.outside_untouched(img, p.lead, d, 0x5A) == [(hi[1], 0xA5, 1, 1, "behind")]
    # in the packed layout the refused slot is the only thing between two live entries
    caps = [40, 7, 100]
    q = S.lay_out(caps, "packed", cover=False)
    e = np.zeros(3, dtype=zpack_amd.DECODE_DESC)
    e["dst_capacity"] = caps
    e["uncomp_size"] = caps
    e = S.refuse(S.placed_desc(e, q), "odd")
    img = np.full(q.lead + q.dst_size + q.tail, 0x5A, dtype=np.uint8)
    img[q.lead + 40] = 0
    img[q.lead + 46] = 0
    assert S.outside_untouched(img, q.lead, e, 0x5A) == [(q.lead + 40, 0, 0, 1, "behind"), (q.lead + 46, 0, 2, 1, "front")]
    assert S.outside_untouched(img, q.lead, e, 0x5A, limit=1) == [(q.lead + 40, 0, 0, 1, "behind")]


# ---- the inputs, by the oracle alone -----------------------------------------------------------------------------------------------------

def test_the_oracle_has_a_verdict_for_every_case_and_refusal_changes_exactly_the_refused(batches):
    for name, (arc, desc) in batches.items():
        base = S.verdicts(arc, desc, 0xA5)
        assert len(base) == len(desc) and all(0 <= v.status <= 24 for v in base), name
        for v, d in zip(base, desc):
            assert (v.bytes is not None and len(v.bytes) == int(d["uncomp_size"])) == (v.status in (S.OK, S.HASH_MISMATCH)), name
        for which in ("even", "odd"):
            d2 = S.refuse(desc, which)
            v2 = S.verdicts(arc, d2, 0xA5)
            for i in range(len(desc)):
                if d2[i]["dst_capacity"] == desc[i]["dst_capacity"]:
                    a, b = v2[i], base[i]
                    assert a[:3] == b[:3] and (a.bytes is None) == (b.bytes is None) and (a.bytes is None or np.array_equal(a.bytes, b.bytes)), (name, i)
                elif int(desc[i]["comp_size"]) == 0:                         # (an entry without compressed bytes is OK before its capacity is looked at)
                    assert v2[i].status == S.OK, (name, i)
                else:
                    assert v2[i][:3] == (S.BUFFER_TOO_SMALL, 0, 0) and v2[i].bytes is None, (name, i, v2[i][:3])


def test_the_fill_decides_a_verdict_only_where_a_frame_ends_early(batches):
    """the two fills give the same status, produced size and hash wherever the frame fills its entry; the entries where they differ are
    the reason the oracle's buffer is pre-filled like the device's"""
    differ = 0
    for name, (arc, desc) in batches.items():
        a, b = S.verdicts(arc, desc, S.FILLS[0]), S.verdicts(arc, desc, S.FILLS[1])
        for i, (x, y) in enumerate(zip(a, b)):
            if x[:3] != y[:3]:
                differ += 1
                assert x.produced == y.produced < int(desc[i]["uncomp_size"]) and {x.status, y.status} <= {S.OK, S.HASH_MISMATCH}, (name, i, x[:3], y[:3])
    print("entries whose verdict depends on the fill:", differ)


def test_most_live_entries_are_intact_and_enough_are_damaged(groups, batches):
    """in every run — all live, even refused, odd refused — at least 80 % of the live entries of a batch decode (their neighbours write
    all of their slots), and at least 25 live entries of every run's batches together are damaged"""
    for which in (None, "even", "odd"):
        damaged = 0
        for name, (arc, desc) in batches.items():
            d = desc if which is None else S.refuse(desc, which)
            v = S.verdicts(arc, d, 0xA5)
            live = [i for i in range(len(d)) if S.is_live(d)[i] and int(d[i]["comp_size"]) > 0]
            intact = sum(1 for i in live if v[i].status == S.OK)
            damaged += len(live) - intact
            assert len(live) >= 40 and intact >= 0.8 * len(live), (name, which, intact, len(live))
        assert damaged >= 25, (which, damaged)


def test_every_kernel_family_is_in_the_lists(groups):
    fam = {}
    for name, cs in groups.items():
        for c in cs:
            fam.setdefault(S.family(c), set()).add(name)
    assert sorted(fam) == ["k_lz4_general", "k_lz4_left", "k_lz4_wave", "k_stored", "k_zstd_fse / k_zstd_exec"], fam
    assert len(fam["k_lz4_general"] & {"mixed", "lz4 batches, general, generated"}) == 2
    assert len({S.family(c) for c in groups["mixed"]}) == 5
    big = S.big_cases()
    assert sum(1 for c in big if c["method"] == S.ZSTD) >= 6 and [c["uncomp"] for c in big if c["method"] != S.ZSTD] == [3 * 65536 + 1, 65536 + 5, 1025]
    assert max(c["uncomp"] for cs in groups.values() for c in cs) <= 512 << 10           # small inputs: a batch is a few MiB
