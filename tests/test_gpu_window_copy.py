"""k_window_copy alone, through zpk_codec_window_copy_device: ONE launch per element size that holds every geometry at which the kernel
takes another path — a group, a wave step, an item edge, one row and many, the whole width and part of it —, the misalignments of source,
destination and base, rows without a base, with one and IN PLACE (base == dst), byte-exact against the map in numpy between canaries;
the window whole against k_plane_copy and k_delta_copy; rows of mixed element sizes in one table; the refusals of the call; its counters."""
import numpy as np
import pytest

import zpack_amd
from tests.device_mem import CANARY, GAP, torch      # noqa: F401  (the fixture)
from tests.test_gpu_plane_copy import grouped, MIS, _place
from tests.test_gpu_delta_copy import TRIPLES

pytestmark = pytest.mark.gpu

NONE, BASE, INPLACE = 0, 1, 2
MIS7 = (0, 1, 7, 15)


def window_of(stored, k, w):
    """the map of include/zpack_codec.h in numpy: destination byte d <- stored[index_k((row0 + d / cols) * row_bytes + col0 + d % cols)]"""
    row_bytes, row0, rows, col0, cols = w
    d = np.arange(rows * cols, dtype=np.int64)
    if d.size == 0:
        return np.zeros(0, dtype=np.uint8)
    i = (row0 + d // cols) * row_bytes + col0 + d % cols
    m = stored.size // k
    return stored[(i % k) * m + i // k]


def geometries(k):
    """(n, window) at the smallest shapes at which the kernel can go wrong, in elements of k bytes: cols around a group (16), a wave step
    (64 groups) and an item (16384 / k); 1, 2, 3 and 70 window rows; the window at and off the row's start; the whole width and part of
    it; the first row, the second and the last"""
    pe = 16384 // k
    out = []
    for ci, colse in enumerate((1, 15, 16, 17, 63 * 16, 64 * 16, 65 * 16, pe - 1, pe, pe + 1)):
        for ri, rows in enumerate((1, 2, 3, 70)):
            if rows == 70 and colse > 65 * 16:
                rows = 5                                                                # (70 rows of an item each: 1 MiB and more per row of the table, no new path)
            col0e = (0, 1, 15, 16)[(ci + ri) % 4]
            whole = (ci + ri) % 3 == 0                                                  # row_bytes = cols: the whole width
            if whole:
                col0e = 0
            row_elems = colse if whole else col0e + colse + (3, 0, 17)[(ci + ri) % 3]   # (0: the window ends where the row ends)
            before, after = ((0, 0), (1, 2), (2, 0))[(ci + 2 * ri) % 3]                 # row0 = 0, 1, last
            nrows = before + rows + after
            out.append((nrows * row_elems * k, (row_elems * k, before, rows, col0e * k, colse * k)))
    out.append((4 * 32 * k, (32 * k, 4, 0, 0, 32 * k)))                                 # windows of no bytes: no rows, no columns
    out.append((4 * 32 * k, (32 * k, 1, 2, 32 * k, 0)))
    return out


def test_the_geometries_reach_every_value_the_issue_names():
    for k in (1, 2, 4, 8):
        g = [w for _, w in geometries(k)]
        pe = 16384 // k
        assert {w[4] // k for w in g} >= {1, 15, 16, 17, 63 * 16, 64 * 16, 65 * 16, pe - 1, pe, pe + 1}
        assert {w[2] for w in g} >= {0, 1, 2, 3, 70} and {w[3] // k for w in g} >= {0, 1, 15, 16} and {w[1] for w in g} >= {0, 1, 2}
        assert any(w[0] == w[4] for w in g) and any(w[0] > w[3] + w[4] for w in g) and any(w[0] == w[3] + w[4] and w[3] for w in g)
        assert any(n // w[0] == w[1] + w[2] and w[1] for n, w in geometries(k))        # the last rows of the entry


def _run_table(torch, rows, rng):
    """rows: (k, n, window, source mis, destination mis, base mis, mode) -> the table, run in ONE launch and compared"""
    lens = [w[2] * w[4] for _, _, w, *_ in rows]
    soffs, stotal = _place([r[1] for r in rows], [r[3] for r in rows])
    doffs, dtotal = _place(lens, [r[4] for r in rows])
    boffs, btotal = _place(lens, [r[5] for r in rows])
    src_h = rng.integers(0, 256, stotal, dtype=np.uint8)
    base_h = rng.integers(0, 256, btotal, dtype=np.uint8)
    dst_h = np.full(dtotal, CANARY, dtype=np.uint8)
    want = dst_h.copy()
    for (k, n, w, _, _, _, mode), ln, so, do, bo in zip(rows, lens, soffs, doffs, boffs):
        cut = window_of(src_h[so:so + n], k, w)
        if mode == INPLACE:
            dst_h[do:do + ln] = base_h[bo:bo + ln]                                      # the destination holds the shard of the previous checkpoint
        want[do:do + ln] = cut if mode == NONE else cut ^ base_h[bo:bo + ln]
    src = torch.from_numpy(src_h).to("cuda:0")
    base_d = torch.from_numpy(base_h).to("cuda:0")
    dst = torch.from_numpy(dst_h).to("cuda:0")
    assert src.data_ptr() % 256 == 0 and dst.data_ptr() % 256 == 0 and base_d.data_ptr() % 256 == 0
    table = np.zeros(len(rows), dtype=zpack_amd.WINDOW_COPY)
    table["src"] = src.data_ptr() + np.array(soffs, dtype=np.uint64)
    table["dst"] = dst.data_ptr() + np.array(doffs, dtype=np.uint64)
    table["base"] = [0 if r[6] == NONE else dst.data_ptr() + do if r[6] == INPLACE else base_d.data_ptr() + bo for r, do, bo in zip(rows, doffs, boffs)]
    table["n"] = [r[1] for r in rows]
    table["win"] = np.array([r[2] for r in rows], dtype=zpack_amd.WINDOW)
    table["elem"] = [r[0] for r in rows]
    codec = zpack_amd.Codec(0)
    try:
        codec.window_copy_device(table)                                                 # ONE launch
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (int(bad[0]), bad.size, [i for i, (do, ln) in enumerate(zip(doffs, lens)) if do - GAP <= bad[0] < do + ln + GAP][:1])
        assert np.array_equal(src.cpu().numpy(), src_h)                                 # sources and bases are only read
        assert np.array_equal(base_d.cpu().numpy(), base_h)
        assert codec.window_stats() == dict(rows=sum(1 for ln in lens if ln), launches=1, staged=0)
        assert codec.delta_stats() == dict(split=0, joined=0, launches=0, staged=0)
        assert codec.planes_stats() == dict(split=0, joined=0, launches=0, staged=0)
    finally:
        codec.close()


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_every_geometry_is_the_map_between_canaries(torch, k):
    rng = np.random.default_rng(34 + k)
    rows = []
    for gi, (n, w) in enumerate(geometries(k)):
        for mode in (NONE, BASE, INPLACE):
            s, d, b = TRIPLES[(gi * 3 + mode) % len(TRIPLES)]
            rows.append((k, n, w, s, d, d if mode == INPLACE else b, mode))
    # every (source, destination, base) misalignment of TRIPLES on one geometry that has groups, loose bytes and several window rows
    n, w = 5 * 90 * k, (90 * k, 1, 3, 7 * k, 67 * k)
    # (... and the same square over 0, 1, 7, 15)
    for mis, triples in ((MIS, TRIPLES), (MIS7, [(MIS7[a], MIS7[b], MIS7[(a + b) % 4]) for a in range(4) for b in range(4)])):
        rows += [(k, n, w, s, d, b, mode) for (s, d, b) in triples for mode in (NONE, BASE)]
        rows += [(k, n, w, s, d, d, INPLACE) for s in mis for d in mis]
    _run_table(torch, rows, rng)


def test_rows_of_mixed_element_sizes_in_one_table(torch):
    rng = np.random.default_rng(340)
    rows = []
    for rep in range(3):
        for k in (8, 1, 4, 2):
            g = geometries(k)
            for gi in range(rep, len(g), 7):
                mode = (gi + rep) % 3
                s, d, b = TRIPLES[(gi + 5 * rep + k) % len(TRIPLES)]
                rows.append((k, g[gi][0], g[gi][1], s, d, d if mode == INPLACE else b, mode))
    assert len({r[0] for r in rows}) == 4 and len(rows) > 60
    _run_table(torch, rows, rng)


def test_the_window_whole_is_the_join_of_the_other_two_kernels(torch):
    """rows = n / row_bytes, col0 = 0, cols = row_bytes: byte for byte what k_plane_copy (no base) and k_delta_copy (a base) join"""
    rng = np.random.default_rng(341)
    codec = zpack_amd.Codec(0)
    try:
        for k in (1, 2, 4, 8):
            for row_bytes, nrows in ((16 * k, 1), (1024 * k + 16 * k, 3), (16384 + 8 * k, 2), (3 * 16384 + 8, 1), (8, 4099)):
                n = row_bytes * nrows
                stored = torch.from_numpy(rng.integers(0, 256, n + 3, dtype=np.uint8)).to("cuda:0")
                base = torch.from_numpy(rng.integers(0, 256, n + 1, dtype=np.uint8)).to("cuda:0")
                out = torch.full((4, n + 2 * GAP), CANARY, dtype=torch.uint8, device="cuda:0")
                S, B = stored.data_ptr() + 3, base.data_ptr() + 1
                codec.plane_copy_device(np.array([(S, out[0].data_ptr() + GAP, n, k, 1)], dtype=zpack_amd.PLANE_COPY))
                codec.delta_copy_device(np.array([(S, out[1].data_ptr() + GAP, B, n, k, 1)], dtype=zpack_amd.DELTA_COPY))
                win = (row_bytes, 0, nrows, 0, row_bytes)
                codec.window_copy_device(np.array([(S, out[2].data_ptr() + GAP, 0, n, win, k, 0), (S, out[3].data_ptr() + GAP, B, n, win, k, 0)], dtype=zpack_amd.WINDOW_COPY))
                torch.cuda.synchronize()
                o = out.cpu().numpy()
                assert np.array_equal(o[2], o[0]) and np.array_equal(o[3], o[1]), (k, row_bytes, nrows)
                assert (o[2, :GAP] == CANARY).all() and (o[2, GAP + n:] == CANARY).all() and (o[0, GAP:GAP + n] != CANARY).any()
                back = np.empty(n, dtype=np.uint8)
                m = n // k
                back.reshape(m, k)[:] = stored.cpu().numpy()[3:].reshape(k, m).T        # join_k in numpy
                assert np.array_equal(o[2, GAP:GAP + n], back)
    finally:
        codec.close()


def test_invalid_windows_bad_pointers_and_overlaps_are_refused_and_nothing_runs(torch):
    L = zpack_amd.lib()
    src = torch.arange(8192, dtype=torch.int32, device="cuda:0").view(torch.uint8)      # 32 KiB
    base = torch.arange(8192, dtype=torch.int32, device="cuda:0").view(torch.uint8) + 1
    dst = torch.full((8192 * 4 + 2 * GAP,), CANARY, dtype=torch.uint8, device="cuda:0")
    small = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    # (ranges that leave their allocation: a block of the caching allocator's is at most 20 MiB around a 4 KiB tensor)
    LONG = 24 << 20
    long_s = torch.zeros(LONG, dtype=torch.uint8, device="cuda:0")
    long_d = torch.full((LONG,), CANARY, dtype=torch.uint8, device="cuda:0")
    host = np.zeros(4096, dtype=np.uint8)
    S, B, D = src.data_ptr(), base.data_ptr(), dst.data_ptr() + GAP
    N = 4096                                                                            # the entry: 16 rows of 256 bytes
    W = (256, 2, 4, 32, 64)                                                             # 256 bytes
    good = (S, D, B, N, W, 4, 0)
    whole_long = (LONG, 0, 1, 0, LONG)
    codec = zpack_amd.Codec(0)
    try:
        torch.cuda.synchronize()
        for bad in ((S, D + 4096, B, N, (0, 0, 0, 0, 0), 4, 0),                         # every clause of window_valid: row_bytes > 0
                    (S, D + 4096, B, N + 4, W, 4, 0),                                   # n % row_bytes
                    (S, D + 4096, B, 4092, (62, 0, 1, 0, 4), 4, 0),                     # row_bytes % k
                    (S, D + 4096, B, N, (256, 2, 4, 30, 64), 4, 0),                     # col0 % k
                    (S, D + 4096, B, N, (256, 2, 4, 32, 62), 4, 0),                     # cols % k
                    (S, D + 4096, B, N, (256, 2, 4, 196, 64), 4, 0),                    # col0 + cols <= row_bytes
                    (S, D + 4096, B, N, (256, 13, 4, 32, 64), 4, 0),                    # row0 + rows <= n / row_bytes
                    (S, D + 4096, B, N, (256, 17, 0, 32, 64), 4, 0),
                    (S, D + 4096, B, N, (256, 2, 4, 2 ** 64 - 32, 64), 4, 0),           # sums that wrap
                    (S, D + 4096, B, N, (256, 2 ** 64 - 2, 4, 32, 64), 4, 0),
                    (S, D + 4096, B, N, (256, 2, 2 ** 64 - 1, 32, 64), 4, 0),
                    (S, D + 4096, B, N, W, 3, 0), (S, D + 4096, B, N, W, 0, 0), (S, D + 4096, B, N, W, 16, 0),     # element sizes
                    (host.ctypes.data, D + 4096, B, N, W, 4, 0), (S, host.ctypes.data, B, N, W, 4, 0), (S, D + 4096, host.ctypes.data, N, W, 4, 0),       # host memory
                    (0, D + 4096, B, N, W, 4, 0), (S, 0, B, N, W, 4, 0),
                    (small.data_ptr(), long_d.data_ptr(), 0, LONG, whole_long, 2, 0),   # the source, the destination, the base leave their allocation
                    (long_s.data_ptr(), small.data_ptr() + 100, 0, LONG, whole_long, 2, 0),
                    (long_s.data_ptr(), long_d.data_ptr(), small.data_ptr() + 1, LONG, whole_long, 1, 0),
                    (S, D + 4096, D + 4096 + 1, N, W, 2, 0), (S, D + 4096 + 8, D + 4096, N, W, 2, 0),              # base and destination overlap in part
                    (S, D + 4096, D + 4096 + 255, N, W, 1, 0), (S, D + 4096 + 255, D + 4096, N, W, 8, 0)):
            both = np.array([good, bad], dtype=zpack_amd.WINDOW_COPY)
            assert L.zpk_codec_window_copy_device(codec.h, both.ctypes.data, 2, None) == -2, bad
        torch.cuda.synchronize()
        assert bool((dst == CANARY).all()) and bool((long_d == CANARY).all()) and not host.any() and not bool(small.any())      # the good row beside the bad one has not run either
        assert codec.window_stats() == dict(rows=0, launches=0, staged=0)
        # a window of no bytes passes wherever it points; a base exactly one window behind its destination passes: both good rows run, and only they
        three = np.array([(0, 0, 0, N, (256, 16, 0, 0, 256), 4, 0), good, (S, D + 8192, D + 8192 + 256, N, W, 2, 0)], dtype=zpack_amd.WINDOW_COPY)
        torch.cuda.synchronize()
        behind = dst[GAP + 8192 + 256:GAP + 8192 + 512].cpu().numpy().copy()            # (canaries: the base of the third row)
        assert L.zpk_codec_window_copy_device(codec.h, three.ctypes.data, 3, None) == 0
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        s_h, b_h = src.cpu().numpy(), base.cpu().numpy()
        assert np.array_equal(got[GAP:GAP + 256], window_of(s_h[:N], 4, W) ^ b_h[:256])
        assert np.array_equal(got[GAP + 8192:GAP + 8192 + 256], window_of(s_h[:N], 2, W) ^ behind)
        rest = np.ones(got.size, dtype=bool)
        rest[GAP:GAP + 256] = rest[GAP + 8192:GAP + 8192 + 256] = False
        assert (got[rest] == CANARY).all()
        assert codec.window_stats() == dict(rows=2, launches=1, staged=0)
    finally:
        codec.close()
