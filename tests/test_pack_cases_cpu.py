"""tests/pack_cases.py judged on the CPU alone: the reference is the serial loop it claims to be, the checker reports what it should, the
short-buffer masks are right at the byte, and the case builders hold every boundary index, residue pair and run length that
tests/test_gpu_pack_alone.py relies on — asserted here, so that a later edit of a builder cannot quietly empty the device tests."""
import numpy as np
import pytest

import zpack_amd
from tests import pack_cases as P


def _batch(rows, gap=3):
    """rows: (status, comp_size, slot capacity) -> (desc, res, slots image): slots `gap` bytes apart, entry i's slot filled with i + 1"""
    desc = np.zeros(len(rows), dtype=zpack_amd.ENCODE_DESC)
    at, parts = 0, []
    for i, (status, size, cap) in enumerate(rows):
        parts += [np.full(gap, P.GAP_BYTE, dtype=np.uint8), np.full(cap, i + 1, dtype=np.uint8)]
        desc[i]["dst_offset"], desc[i]["dst_capacity"] = at + gap, cap
        at += gap + cap
    return desc, P.results([r[0] for r in rows], [r[1] for r in rows]), np.concatenate(parts + [np.full(P.SLOT_PAD, P.GAP_BYTE, dtype=np.uint8)])


HAND = {
    "plain": [(0, 5, 5), (0, 0, 0), (0, 17, 20), (0, 1, 1)],
    "failed in the middle, garbage sizes": [(0, 3, 3), (14, 9, 9), (12, 2, 40), (0, 4, 4), (-1, 7, 7)],
    "failed first and last, empty neighbours": [(14, 6, 6), (0, 0, 0), (0, 0, 3), (0, 16, 16), (0, 33, 33), (12, 1, 1)],
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_reference_is_the_serial_loop(name):
    desc, res, slots = _batch(HAND[name])
    write_offset, offsets, image = 0, [], bytearray()
    for i, (status, size, cap) in enumerate(HAND[name]):
        offsets.append(write_offset)
        if status != 0:
            continue
        a = int(desc[i]["dst_offset"])
        image += slots[a:a + size].tobytes()
        write_offset += size
    offsets.append(write_offset)
    ref = P.reference(desc, res, slots)
    assert ref.offsets.dtype == np.uint64 and ref.offsets.tolist() == offsets
    assert ref.image.tobytes() == bytes(image) and ref.must.all() and not ref.may.any()
    assert P.reference(None, res).offsets.tolist() == offsets and P.reference(None, res).image is None


def test_reference_keeps_the_high_half():
    """sizes around 2^32 and 2^40: python integers against the uint64 cumsum"""
    sizes = [2**32 - 1, 1, 2**32, 2**40 + 7, 0, 2**32 + 1, 5]
    status = [0, 0, 14, 0, 0, 0, 0]
    want, at = [], 0
    for st, sz in zip(status, sizes):
        want.append(at)
        at += sz if st == 0 else 0
    assert P.reference(None, P.results(status, sizes)).offsets.tolist() == want + [at]


def _left_behind(desc, res, slots, lead, fill, tail=100):
    """the allocation a faultless call would leave"""
    ref = P.reference(desc, res, slots)
    whole = np.full(lead + len(ref.image) + tail, fill, dtype=np.uint8)
    whole[lead:lead + len(ref.image)] = ref.image
    return ref.offsets.copy(), whole


@pytest.mark.parametrize("fill", P.FILLS)
def test_checker_reports_a_flipped_status_a_changed_size_and_a_flipped_byte(fill):
    desc, res, slots = _batch(HAND["failed in the middle, garbage sizes"])
    ref = P.reference(desc, res, slots)
    offsets, whole = _left_behind(desc, res, slots, 7, fill)
    assert P.check(ref, offsets, whole, 7, fill) == []
    assert P.check(ref, offsets, None, 0, fill) == []
    # a failed entry that was given room, a live one that was given none
    for i, status in ((1, 0), (3, 14)):
        r2 = res.copy()
        r2[i]["status"] = status
        o2, w2 = _left_behind(desc, r2, slots, 7, fill)
        said = P.check(ref, o2, None, 0, fill)
        assert len(said) == 1 and "first at entry %d" % (i + 1) in said[0], said
    r2 = res.copy()
    r2[0]["comp_size"] = 2
    o2, w2 = _left_behind(desc, r2, slots, 7, fill)
    assert "first at entry 1" in P.check(ref, o2, w2, 7, fill)[0]
    assert any("packed byte 2 (entry 0, its byte 2)" in s for s in P.check(ref, o2, w2, 7, fill))
    # one payload byte, one byte in front of the base, the byte behind offsets[n], the last byte of the allocation
    for k, word in ((7 + 4, "packed byte 4 (entry 3, its byte 1)"), (6, "front guard, 1 in front"), (0, "front guard, 7 in front"),
                    (7 + 7, "0 behind offsets[n]"), (len(whole) - 1, "99 behind offsets[n]")):
        w2 = whole.copy()
        w2[k] ^= 0x40
        said = P.check(ref, offsets, w2, 7, fill)
        assert len(said) == 1 and word in said[0], (k, said)
    o2 = offsets.copy()
    o2[-1] += np.uint64(2**32)
    assert "first at entry 5" in P.check(ref, o2, whole, 7, fill)[0]


def test_short_cap_masks_at_the_byte():
    """entries of 10, 0, 6 and 8 bytes at 0, 10, 10 and 16: an entry that ends exactly at the cap is `must`, one byte further `may`"""
    desc, res, slots = _batch([(0, 10, 10), (0, 0, 0), (14, 5, 5), (0, 6, 6), (0, 8, 8)])
    full = P.reference(desc, res, slots)
    assert full.offsets.tolist() == [0, 10, 10, 10, 16, 24]
    for cap, must, may in ((24, range(24), ()), (23, range(16), range(16, 23)), (17, range(16), (16,)), (16, range(16), ()),
                           (15, range(10), range(10, 15)), (10, range(10), ()), (9, (), range(9)), (0, (), ()), (40, range(24), ())):
        r = P.reference(desc, res, slots, cap)
        assert np.array_equal(r.offsets, full.offsets) and np.array_equal(r.image, full.image)
        assert np.nonzero(r.must)[0].tolist() == list(must) and np.nonzero(r.may)[0].tolist() == list(may), cap
    # the checker under a cap of 15: entry 3's five bytes in front of the cap may be the payload or the fill, nothing else;
    # nothing at or behind the cap may be written
    fill = P.FILLS[0]
    r = P.reference(desc, res, slots, 15)
    whole = np.full(4 + 24 + 50, fill, dtype=np.uint8)
    whole[4:4 + 10] = r.image[:10]
    assert P.check(r, r.offsets, whole, 4, fill, 15) == []
    whole[4 + 10:4 + 15] = r.image[10:15]
    assert P.check(r, r.offsets, whole, 4, fill, 15) == []
    w2 = whole.copy()
    w2[4 + 12] = 0x11
    assert "may stay the fill" in P.check(r, r.offsets, w2, 4, fill, 15)[0]
    w2 = whole.copy()
    w2[4 + 15] = r.image[15]
    assert "at or behind the cap 15" in P.check(r, r.offsets, w2, 4, fill, 15)[0]
    w2 = whole.copy()
    w2[4 + 3] = fill
    assert "packed byte 3 (entry 0, its byte 3)" in P.check(r, r.offsets, w2, 4, fill, 15)[0]


def test_scan_cases_hold_every_boundary():
    cases = P.scan_cases()
    assert len(cases) == 4 * len(P.SCAN_N)
    assert P.SCAN_N == (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 262144, 262145, 263171)
    assert -(-263171 // P.PK_BLOCK) == 258 and 263171 - 257 * P.PK_BLOCK == 3          # two blocks in the second trip, three entries in the last
    assert P.SPIKE_AT == (3, 4, 255, 256, 1023, 1024, 262143, 262144)
    for n in P.SCAN_N:
        st, sz = cases["n = %d, small" % n]
        assert len(st) == n and (st == 0).all() and int(sz.max()) <= 4096
        # spikes: one of the four values at every boundary index the batch has; the values around 2^32 all occur in the large batches
        st, sz = cases["n = %d, spikes" % n]
        at = [i for i in P.SPIKE_AT + (0, n - 1) if i < n]
        assert (st == 0).all() and all(int(sz[i]) in P.SPIKES for i in at) and int((sz > 4096).sum()) == len(set(at))
        if n > P.PK_BLOCK:
            assert {int(sz[i]) for i in at} == set(P.SPIKES)
            assert int(P.reference(None, P.results(st, sz)).offsets[-1]) > 2**40
        # holes: failed entries whose garbage would be seen, the runs named
        st, sz = cases["n = %d, holes" % n]
        runs = P.hole_runs(n)
        failed = np.zeros(n, dtype=bool)
        for a, k in runs:
            assert (st[a:a + k] != 0).all() and (sz[a:a + k] > 0).all()
            failed[a:a + k] = True
        assert np.array_equal(failed, st != 0) and st[0] != 0 and st[n - 1] != 0
        assert all(not failed[a - 1] for a, k in runs if a > 0) and all(not failed[a + k] for a, k in runs if a + k < n)
        if n >= P.TRIP:
            B = P.PK_BLOCK
            for k in P.HOLE_RUNS:
                assert any(j == k and a % B == 0 for a, j in runs) and any(j == k and a % B != 0 for a, j in runs), k
            assert (16 * B, B + 5) in runs and (21 * B - 5, B + 5) in runs             # a whole block of failed entries, twice
            assert sum(1 for a, k in runs if k == 1) >= 4
            assert (n >= P.TRIP + 32) == any(a < P.TRIP < a + k for a, k in runs)      # a run across the trips, where it fits
        st, sz = cases["n = %d, all failed" % n]
        assert (st != 0).all() and (sz > 0).all()
        assert not P.reference(None, P.results(st, sz)).offsets.any()
        for kind in ("small", "spikes", "holes"):
            st, sz = cases["n = %d, %s" % (n, kind)]
            assert int(np.where(st == 0, sz, 0).astype(object).sum()) < 2**60
    assert len(P.hole_runs(1025)) >= 8 and {k for a, k in P.hole_runs(1025)} == {1, 4, 64, 256}


def test_gather_cases_hold_every_size_residue_and_run():
    g = P.gather_cases()
    e, m = g["edges"], g["many"]
    assert P.EDGE_SIZES == (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385,
                            32767, 32768, 32769, 3 * 16384 + 5, 2**20 + 3)
    live = e.res["status"] == 0
    # every size in a live slot at every residue; the slot is exactly the size
    seen = {(int(s), int(a) % 16) for s, a in zip(e.res["comp_size"][live], e.desc["dst_offset"][live])}
    assert {(s, r) for s in P.EDGE_SIZES for r in range(16)} <= seen
    assert np.array_equal(e.res["comp_size"][live], e.desc["dst_capacity"][live])
    # every packed residue against several slot residues, and most of the 256 pairs
    pairs = P.residue_pairs(e)
    assert sorted(pairs) == list(range(16)) and min(len(v) for v in pairs.values()) >= 4
    assert sum(len(v) for v in pairs.values()) >= 128
    # every seventh entry failed, its garbage nonzero and inside its slot; nothing else failed
    n = len(e.res)
    assert np.array_equal(np.nonzero(~live)[0], np.arange(6, n, 7))
    assert (e.res["comp_size"][~live] > 0).all() and (e.res["comp_size"][~live] <= e.desc["dst_capacity"][~live]).all()
    # two empty live entries side by side at both ends
    assert live[[0, 1, n - 2, n - 1]].all() and not e.res["comp_size"][[0, 1, n - 2, n - 1]].any()
    # slots hold other bytes than the space between them, which holds GAP_BYTE; 64 bytes behind the last slot
    inside = np.zeros(len(e.slots), dtype=bool)
    for a, k in zip(e.desc["dst_offset"].tolist(), e.desc["dst_capacity"].tolist()):
        assert k == 0 or not inside[a - 1:a + k].any()                                   # at least one byte between two slots
        inside[a:a + k] = True
    assert (e.slots[~inside] == P.GAP_BYTE).all() and (e.slots[inside] != P.GAP_BYTE).mean() > 0.99 and not inside[-P.SLOT_PAD:].any()
    assert P.GAP_BYTE not in P.FILLS
    assert 18e6 < len(e.slots) < 30e6 and e.max_entry_size == 2**20 + 3
    ref = P.gather_reference("edges")
    total = len(ref.image)
    caps = P.short_caps(total)
    assert caps[:5] == [total - 1, total - 16, total - 16383, total - 16384, total - 16385] and abs(caps[5] - total / 2) < 8 and caps[6] == 0
    for cap in caps:          # every short cap leaves something that may be written and — but for 0 — something that must
        r = P.reference(e.desc, e.res, e.slots, cap)
        assert r.may.any() == (cap > 0) and r.must.any() == (cap > 0) and not (r.must & r.may).any()

    # many
    assert len(m.res) == 263171 and m.max_entry_size == 48 and int(m.res["comp_size"].max()) == 48 and int(m.desc["dst_capacity"].max()) == 48
    failed = m.res["status"] != 0
    assert 0.11 < failed.mean() < 0.14 and (m.res["comp_size"][failed] > 0).mean() > 0.8
    assert (m.res["comp_size"] <= m.desc["dst_capacity"]).all()
    gaps = m.desc["dst_offset"][1:] - (m.desc["dst_offset"][:-1] + m.desc["dst_capacity"][:-1])
    assert set(gaps.tolist()) == {0, 1, 2, 3}
    assert 5e6 < len(m.slots) < 8e6
    # runs of entries without a span: several lengths, in both trips of the scans
    spanless = failed | (m.res["comp_size"] == 0)
    edges = np.diff(np.concatenate([[0], spanless.astype(np.int8), [0]]))
    starts, lengths = np.nonzero(edges == 1)[0], np.nonzero(edges == -1)[0] - np.nonzero(edges == 1)[0]
    assert {1, 2, 3} <= set(lengths.tolist()) and (starts[lengths >= 2] > P.TRIP).any() and (starts[lengths >= 2] < P.TRIP).any()
    mref = P.gather_reference("many")
    assert set((mref.offsets[:-1][~spanless] % np.uint64(16)).tolist()) == set(range(16))
