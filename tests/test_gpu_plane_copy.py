"""k_plane_copy alone, through zpk_codec_plane_copy_device: both directions for every element size, every size at which the kernel takes
another path, every pairing of source and destination misalignment, many rows in one launch, byte-exact against numpy between canaries;
and the pointer rule of the call."""
import numpy as np
import pytest

import zpack_amd
from tests.device_mem import CANARY, GAP, torch      # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

MIS = (0, 1, 3, 15)
BIG = 3 * (1 << 20) + 5


def sizes_of(k):
    return [0, 1, k - 1, k, k + 1, 16 * k - 1, 16 * k + 1, 1024 * k - 1, 1024 * k + 1, 16384 - 1, 16384 + 1, 3 * 16384 + 5]


def grouped(a, k):
    m = a.size // k
    return np.concatenate([a[:m * k].reshape(m, k).T.reshape(-1), a[m * k:]])


def _place(lens, mis):
    """rows back to back, at least GAP bytes between them, row i at an address = mis[i] mod 16 (the buffers are 256-aligned)"""
    pos, offs = GAP, []
    for n, a in zip(lens, mis):
        pos = ((pos + 15) & ~15) + a
        offs.append(pos)
        pos += n + GAP
    return offs, pos + GAP


@pytest.mark.parametrize("k", [2, 4, 8])
def test_split_and_join_are_the_numpy_layout_between_canaries(torch, k):
    rng = np.random.default_rng(28 + k)
    rows = [(n, join, s, d) for n in sizes_of(k) for join in (0, 1) for s in MIS for d in MIS]          # every size x direction x misalignment pair
    rows += [(BIG, 0, 3, 1), (BIG, 1, 15, 0), (0, 0, 0, 0)]                                             # 193 items each; and a last row of no bytes
    lens = [r[0] for r in rows]
    soffs, stotal = _place(lens, [r[2] for r in rows])
    doffs, dtotal = _place(lens, [r[3] for r in rows])
    src_h = rng.integers(0, 256, stotal, dtype=np.uint8)
    want = np.full(dtotal, CANARY, dtype=np.uint8)
    for (n, join, _, _), so, do in zip(rows, soffs, doffs):
        plain = src_h[so:so + n]
        if join:                                                                                        # the source holds grouped bytes: they come back plain
            plain = rng.integers(0, 256, n, dtype=np.uint8)
            src_h[so:so + n] = grouped(plain, k)
            want[do:do + n] = plain
        else:
            want[do:do + n] = grouped(plain, k)
    src = torch.from_numpy(src_h).to("cuda:0")
    dst = torch.full((dtotal,), CANARY, dtype=torch.uint8, device="cuda:0")
    assert src.data_ptr() % 256 == 0 and dst.data_ptr() % 256 == 0
    table = np.zeros(len(rows), dtype=zpack_amd.PLANE_COPY)
    table["src"] = src.data_ptr() + np.array(soffs, dtype=np.uint64)
    table["dst"] = dst.data_ptr() + np.array(doffs, dtype=np.uint64)
    table["len"] = lens
    table["elem"] = k
    table["join"] = [r[1] for r in rows]
    codec = zpack_amd.Codec(0)
    try:
        codec.plane_copy_device(table)                                                                  # ONE launch
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (int(bad[0]), bad.size)
        assert np.array_equal(src.cpu().numpy(), src_h)
        nz = [r for r in rows if r[0]]
        assert codec.planes_stats() == dict(split=sum(1 for r in nz if not r[1]), joined=sum(1 for r in nz if r[1]), launches=1, staged=0)
    finally:
        codec.close()


def test_element_size_one_copies_and_a_round_trip_is_the_identity(torch):
    rng = np.random.default_rng(5)
    n = 2 * 16384 + 777
    plain_h = rng.integers(0, 256, n + 1, dtype=np.uint8)
    plain = torch.from_numpy(plain_h).to("cuda:0")
    mid = torch.full((4, n + 2 * GAP), CANARY, dtype=torch.uint8, device="cuda:0")
    back = torch.full((4, n + 2 * GAP), CANARY, dtype=torch.uint8, device="cuda:0")
    ks = (1, 2, 4, 8)
    split = np.zeros(4, dtype=zpack_amd.PLANE_COPY)
    join = np.zeros(4, dtype=zpack_amd.PLANE_COPY)
    for i, k in enumerate(ks):
        split[i] = (plain.data_ptr() + 1, mid[i].data_ptr() + GAP, n, k, 0)
        join[i] = (mid[i].data_ptr() + GAP, back[i].data_ptr() + GAP + 1, n, k, 1)
    codec = zpack_amd.Codec(0)
    try:
        codec.plane_copy_device(split)
        codec.plane_copy_device(join)                                                                   # (behind the split, on the same stream)
        torch.cuda.synchronize()
        m, b = mid.cpu().numpy(), back.cpu().numpy()
        for i, k in enumerate(ks):
            assert np.array_equal(m[i, GAP:GAP + n], grouped(plain_h[1:], k)), k
            assert (m[i, :GAP] == CANARY).all() and (m[i, GAP + n:] == CANARY).all()
            assert np.array_equal(b[i, GAP + 1:GAP + 1 + n], plain_h[1:]), k
            assert (b[i, :GAP + 1] == CANARY).all() and (b[i, GAP + 1 + n:] == CANARY).all()
        assert np.array_equal(m[0, GAP:GAP + n], plain_h[1:])                                           # element size 1: a copy
        assert codec.planes_stats() == dict(split=0, joined=4, launches=1, staged=0)                    # (the most recent call)
    finally:
        codec.close()


def test_a_pointer_that_leaves_its_allocation_is_invalid_and_nothing_runs(torch):
    L = zpack_amd.lib()
    src = torch.arange(8192, dtype=torch.int32, device="cuda:0").view(torch.uint8)
    dst = torch.full((8192 * 4 + 2 * GAP,), CANARY, dtype=torch.uint8, device="cuda:0")
    small = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    host = np.zeros(64, dtype=np.uint8)
    good = (src.data_ptr(), dst.data_ptr() + GAP, 1000, 4, 0)
    codec = zpack_amd.Codec(0)
    try:
        torch.cuda.synchronize()
        for bad in ((small.data_ptr(), dst.data_ptr() + GAP, 1 << 40, 2, 0), (src.data_ptr(), small.data_ptr() + 100, 1 << 40, 2, 1),
                    (host.ctypes.data, dst.data_ptr() + GAP, 64, 4, 0), (src.data_ptr(), host.ctypes.data, 64, 4, 1), (0, dst.data_ptr() + GAP, 16, 8, 0),
                    (src.data_ptr(), 0, 16, 8, 0),
                    (src.data_ptr(), dst.data_ptr() + GAP, 64, 3, 0), (src.data_ptr(), dst.data_ptr() + GAP, 64, 0, 1), (src.data_ptr(), dst.data_ptr() + GAP, 0, 16, 0)):
            both = np.array([good, bad], dtype=zpack_amd.PLANE_COPY)
            assert L.zpk_codec_plane_copy_device(codec.h, both.ctypes.data, 2, None) == -2, bad
        torch.cuda.synchronize()
        assert bool((dst == CANARY).all()) and not host.any() and not bool(small.any())
        assert codec.planes_stats() == dict(split=0, joined=0, launches=0, staged=0)
        # a row of no bytes passes wherever it points: the good row beside it runs, and only that
        both = np.array([(0, 0, 0, 4, 0), good], dtype=zpack_amd.PLANE_COPY)
        assert L.zpk_codec_plane_copy_device(codec.h, both.ctypes.data, 2, None) == 0
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert np.array_equal(got[GAP:GAP + 1000], grouped(src.cpu().numpy()[:1000], 4))
        assert (got[:GAP] == CANARY).all() and (got[GAP + 1000:] == CANARY).all()
    finally:
        codec.close()
