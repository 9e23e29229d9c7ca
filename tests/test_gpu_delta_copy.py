"""k_delta_copy alone, through zpk_codec_delta_copy_device: ONE launch per element size that holds both directions, every size at which
the kernel takes another path, the misalignments of source, destination and base, two rows of 3 MiB + 5 bytes and a set of joins IN PLACE
(base == dst), byte-exact against numpy between canaries; the refusals of the call; its counters."""
import numpy as np
import pytest

import zpack_amd
from tests.device_mem import CANARY, GAP, torch      # noqa: F401  (the fixture)
from tests.test_gpu_plane_copy import sizes_of, grouped, MIS, BIG, _place

pytestmark = pytest.mark.gpu

# (source, destination, base) misalignments: source x destination is the full square, and the base runs through every value against every
# value of the source and against every value of the destination (a Latin square) — 16 triples, not 64
TRIPLES = [(MIS[a], MIS[b], MIS[(a + b) % 4]) for a in range(4) for b in range(4)]


def test_the_triples_pair_every_value_of_each_with_every_value_of_another():
    for x, y in ((0, 1), (0, 2), (1, 2)):
        assert {(t[x], t[y]) for t in TRIPLES} == {(p, q) for p in MIS for q in MIS}


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_split_and_join_with_a_base_are_the_numpy_layout_between_canaries(torch, k):
    rng = np.random.default_rng(29 + k)
    # (len, join, source mis, destination mis, base mis, in place)
    rows = [(n, join, s, d, b, False) for n in sizes_of(k) for join in (0, 1) for (s, d, b) in TRIPLES]
    rows += [(BIG, 0, 3, 1, 15, False), (BIG, 1, 15, 0, 1, False)]                                      # 193 items each
    rows += [(n, 1, s, d, d, True) for n in sizes_of(k) for s in MIS for d in MIS]                      # joins whose base IS the destination
    rows += [(BIG, 1, 1, 3, 3, True), (0, 0, 0, 0, 0, False)]                                           # ... a long one; and a last row of no bytes
    lens = [r[0] for r in rows]
    soffs, stotal = _place(lens, [r[2] for r in rows])
    doffs, dtotal = _place(lens, [r[3] for r in rows])
    boffs, btotal = _place(lens, [r[4] for r in rows])
    src_h = rng.integers(0, 256, stotal, dtype=np.uint8)
    base_h = rng.integers(0, 256, btotal, dtype=np.uint8)
    dst_h = np.full(dtotal, CANARY, dtype=np.uint8)
    want = dst_h.copy()
    for (n, join, _, _, _, inplace), so, do, bo in zip(rows, soffs, doffs, boffs):
        base = base_h[bo:bo + n]
        if inplace:
            dst_h[do:do + n] = base                                                                     # the destination holds the previous bytes
        if join:                                                                                        # the source holds split(plain ^ base): plain comes back
            plain = rng.integers(0, 256, n, dtype=np.uint8)
            src_h[so:so + n] = grouped(plain ^ base, k)
            want[do:do + n] = plain
        else:
            want[do:do + n] = grouped(src_h[so:so + n] ^ base, k)
    src = torch.from_numpy(src_h).to("cuda:0")
    base_d = torch.from_numpy(base_h).to("cuda:0")
    dst = torch.from_numpy(dst_h).to("cuda:0")
    assert src.data_ptr() % 256 == 0 and dst.data_ptr() % 256 == 0 and base_d.data_ptr() % 256 == 0
    table = np.zeros(len(rows), dtype=zpack_amd.DELTA_COPY)
    table["src"] = src.data_ptr() + np.array(soffs, dtype=np.uint64)
    table["dst"] = dst.data_ptr() + np.array(doffs, dtype=np.uint64)
    table["base"] = [dst.data_ptr() + do if r[5] else base_d.data_ptr() + bo for r, do, bo in zip(rows, doffs, boffs)]
    table["len"] = lens
    table["elem"] = k
    table["join"] = [r[1] for r in rows]
    codec = zpack_amd.Codec(0)
    try:
        codec.delta_copy_device(table)                                                                  # ONE launch
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (int(bad[0]), bad.size)                                                   # every row, in place too, and every canary
        assert np.array_equal(src.cpu().numpy(), src_h)                                                 # sources and bases are only read
        assert np.array_equal(base_d.cpu().numpy(), base_h)
        nz = [r for r in rows if r[0]]
        assert codec.delta_stats() == dict(split=sum(1 for r in nz if not r[1]), joined=sum(1 for r in nz if r[1]), launches=1, staged=0)
        assert codec.planes_stats() == dict(split=0, joined=0, launches=0, staged=0)
    finally:
        codec.close()


def test_a_round_trip_is_the_identity_and_a_base_equal_to_the_source_stores_zeros(torch):
    rng = np.random.default_rng(6)
    n = 2 * 16384 + 777
    plain_h = rng.integers(0, 256, n + 1, dtype=np.uint8)
    base_h = rng.integers(0, 256, n + 3, dtype=np.uint8)
    plain = torch.from_numpy(plain_h).to("cuda:0")
    base = torch.from_numpy(base_h).to("cuda:0")
    mid = torch.full((8, n + 2 * GAP), CANARY, dtype=torch.uint8, device="cuda:0")
    back = torch.full((4, n + 2 * GAP), CANARY, dtype=torch.uint8, device="cuda:0")
    ks = (1, 2, 4, 8)
    split = np.zeros(8, dtype=zpack_amd.DELTA_COPY)
    join = np.zeros(4, dtype=zpack_amd.DELTA_COPY)
    for i, k in enumerate(ks):
        split[i] = (plain.data_ptr() + 1, mid[i].data_ptr() + GAP, base.data_ptr() + 3, n, k, 0)
        split[4 + i] = (plain.data_ptr() + 1, mid[4 + i].data_ptr() + GAP, plain.data_ptr() + 1, n, k, 0)     # the base overlaps the source freely: both are read
        join[i] = (mid[i].data_ptr() + GAP, back[i].data_ptr() + GAP + 1, base.data_ptr() + 3, n, k, 1)
    codec = zpack_amd.Codec(0)
    try:
        codec.delta_copy_device(split)
        codec.delta_copy_device(join)                                                                   # (behind the split, on the same stream)
        torch.cuda.synchronize()
        m, b = mid.cpu().numpy(), back.cpu().numpy()
        for i, k in enumerate(ks):
            assert np.array_equal(m[i, GAP:GAP + n], grouped(plain_h[1:] ^ base_h[3:], k)), k
            assert not m[4 + i, GAP:GAP + n].any(), k
            assert (m[i, :GAP] == CANARY).all() and (m[i, GAP + n:] == CANARY).all()
            assert np.array_equal(b[i, GAP + 1:GAP + 1 + n], plain_h[1:]), k
            assert (b[i, :GAP + 1] == CANARY).all() and (b[i, GAP + 1 + n:] == CANARY).all()
        assert codec.delta_stats() == dict(split=0, joined=4, launches=1, staged=0)                     # (the most recent call)
    finally:
        codec.close()


def test_bad_pointers_and_overlaps_are_invalid_and_nothing_runs(torch):
    L = zpack_amd.lib()
    src = torch.arange(8192, dtype=torch.int32, device="cuda:0").view(torch.uint8)
    base = torch.arange(8192, dtype=torch.int32, device="cuda:0").view(torch.uint8) + 1
    dst = torch.full((8192 * 4 + 2 * GAP,), CANARY, dtype=torch.uint8, device="cuda:0")
    small = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    # (a base that is too short: source and destination hold LONG bytes, the base's allocation — a block of the caching allocator's, at most
    # 20 MiB around a 4 KiB tensor — does not)
    LONG = 24 << 20
    long_s = torch.zeros(LONG, dtype=torch.uint8, device="cuda:0")
    long_d = torch.full((LONG,), CANARY, dtype=torch.uint8, device="cuda:0")
    host = np.zeros(64, dtype=np.uint8)
    S, B, D = src.data_ptr(), base.data_ptr(), dst.data_ptr() + GAP
    good = (S, D, B, 1000, 4, 0)
    codec = zpack_amd.Codec(0)
    try:
        torch.cuda.synchronize()
        for bad in ((small.data_ptr(), D, B, 1 << 40, 2, 0), (S, small.data_ptr() + 100, B, 1 << 40, 2, 1),           # source, destination leave their allocation
                    (long_s.data_ptr(), long_d.data_ptr(), small.data_ptr(), LONG, 2, 0), (long_s.data_ptr(), long_d.data_ptr(), small.data_ptr() + 1, LONG, 1, 1),     # the base is too short
                    (host.ctypes.data, D + 4096, B, 64, 4, 0), (S, host.ctypes.data, B, 64, 4, 1), (S, D + 4096, host.ctypes.data, 64, 4, 1),      # host memory
                    (0, D + 4096, B, 16, 8, 0), (S, 0, B, 16, 8, 0),
                    (S, D + 4096, 0, 16, 8, 0), (S, D + 4096, 0, 16, 1, 1),                                           # no base: a row of the other call
                    (S, D + 4096, D + 4096 + 1, 64, 2, 1), (S, D + 4096 + 8, D + 4096, 64, 2, 1),                     # join: base and destination overlap in part
                    (S, D + 4096, D + 4096 + 63, 64, 1, 1), (S, D + 4096 + 1, D + 4096, 4096, 8, 0),
                    (S, D + 4096, D + 4096, 64, 2, 0),                                                                # split: base == dst is no in-place join
                    (S, D + 4096, B, 64, 3, 0), (S, D + 4096, B, 64, 0, 1), (S, D + 4096, B, 0, 16, 0)):              # element sizes
            both = np.array([good, bad], dtype=zpack_amd.DELTA_COPY)
            assert L.zpk_codec_delta_copy_device(codec.h, both.ctypes.data, 2, None) == -2, bad
        torch.cuda.synchronize()
        assert bool((dst == CANARY).all()) and bool((long_d == CANARY).all()) and not host.any() and not bool(small.any())                 # the good row beside the bad one has not run either
        assert codec.delta_stats() == dict(split=0, joined=0, launches=0, staged=0)
        # a row of no bytes passes wherever it points, base or none: the good row beside it runs, and only that
        both = np.array([(0, 0, 0, 0, 4, 0), good], dtype=zpack_amd.DELTA_COPY)
        assert L.zpk_codec_delta_copy_device(codec.h, both.ctypes.data, 2, None) == 0
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert np.array_equal(got[GAP:GAP + 1000], grouped(src.cpu().numpy()[:1000] ^ base.cpu().numpy()[:1000], 4))
        assert (got[:GAP] == CANARY).all() and (got[GAP + 1000:] == CANARY).all()
        assert codec.delta_stats() == dict(split=1, joined=0, launches=1, staged=0)
    finally:
        codec.close()
