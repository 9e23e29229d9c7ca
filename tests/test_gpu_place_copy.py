"""k_place_copy alone, through zpk_codec_place_copy_device: ONE launch per element size that holds every geometry of the window test crossed
with the pitches at which the placed offsets can go wrong — none beyond the columns, one byte, an element, a group, the columns again,
4099 —, the misalignments of source, destination and base, rows without a base, with one and IN PLACE (base == dst), byte-exact against
the map in numpy with the destination filled with canaries: the gaps inside every extent are checked as both of its ends are.  Three
shards merged into one matrix in one table; an item that ends mid-row; pitch == cols against k_window_copy; mixed element sizes; the
refusals of the call; its counters."""
import numpy as np
import pytest

import zpack_amd
from tests.device_mem import CANARY, GAP, torch      # noqa: F401  (the fixture)
from tests.test_gpu_plane_copy import MIS, _place
from tests.test_gpu_delta_copy import TRIPLES
from tests.test_gpu_window_copy import geometries, window_of

pytestmark = pytest.mark.gpu

NONE, BASE, INPLACE = 0, 1, 2


def pitches_of(k, cols):
    return (cols, cols + 1, cols + k, cols + 16 * k, 2 * cols, cols + 4099)


def extent_of(w, pitch):
    return (w[2] - 1) * pitch + w[4] if w[2] * w[4] else 0


def placed_index(w, pitch):
    """the map of include/zpack_codec.h in numpy: window byte d lands at buffer byte (d / cols) * pitch + d % cols"""
    d = np.arange(w[2] * w[4], dtype=np.int64)
    return (d // w[4]) * pitch + d % w[4] if d.size else d


def _run_table(torch, rows, rng, codec=None):
    """rows: (k, n, window, pitch, source mis, destination mis, base mis, mode) -> the table, run in ONE launch and compared.  Rows with
    the same (k, n, window, source mis) read ONE source: sources are only read."""
    exts = [extent_of(r[2], r[3]) for r in rows]
    keys = sorted({(r[0], r[1], r[2], r[4]) for r in rows})
    soffs_of = dict(zip(keys, _place([key[1] for key in keys], [key[3] for key in keys])[0]))
    stotal = _place([key[1] for key in keys], [key[3] for key in keys])[1]
    doffs, dtotal = _place(exts, [r[5] for r in rows])
    boffs, btotal = _place(exts, [r[6] for r in rows])
    src_h = rng.integers(0, 256, stotal, dtype=np.uint8)
    base_h = rng.integers(0, 256, btotal, dtype=np.uint8)
    dst_h = np.full(dtotal, CANARY, dtype=np.uint8)
    for r, e, do, bo in zip(rows, exts, doffs, boffs):
        if r[7] == INPLACE:
            dst_h[do:do + e] = base_h[bo:bo + e]                                        # the destination holds the previous checkpoint, gaps included
    want = dst_h.copy()
    cuts = {key: window_of(src_h[so:so + key[1]], key[0], key[2]) for key, so in soffs_of.items()}
    for r, do, bo in zip(rows, doffs, boffs):
        k, n, w, pitch, s, _, _, mode = r
        o = placed_index(w, pitch)
        cut = cuts[(k, n, w, s)]
        want[do + o] = cut if mode == NONE else cut ^ base_h[bo + o]
    src = torch.from_numpy(src_h).to("cuda:0")
    base_d = torch.from_numpy(base_h).to("cuda:0")
    dst = torch.from_numpy(dst_h).to("cuda:0")
    assert src.data_ptr() % 256 == 0 and dst.data_ptr() % 256 == 0 and base_d.data_ptr() % 256 == 0
    table = np.zeros(len(rows), dtype=zpack_amd.PLACE_COPY)
    table["src"] = [src.data_ptr() + soffs_of[(r[0], r[1], r[2], r[4])] for r in rows]
    table["dst"] = dst.data_ptr() + np.array(doffs, dtype=np.uint64)
    table["base"] = [0 if r[7] == NONE else dst.data_ptr() + do if r[7] == INPLACE else base_d.data_ptr() + bo for r, do, bo in zip(rows, doffs, boffs)]
    table["n"] = [r[1] for r in rows]
    table["win"] = np.array([r[2] for r in rows], dtype=zpack_amd.WINDOW)
    table["pitch"] = [r[3] for r in rows]
    table["elem"] = [r[0] for r in rows]
    own = codec is None
    codec = codec or zpack_amd.Codec(0)
    try:
        codec.place_copy_device(table)                                                  # ONE launch
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        bad = np.flatnonzero(got != want)                                               # every byte of the buffer: placed bytes, gaps, both ends of every extent
        assert bad.size == 0, (int(bad[0]), bad.size, [(i, rows[i]) for i, (do, e) in enumerate(zip(doffs, exts)) if do - GAP <= bad[0] < do + e + GAP][:1])
        assert np.array_equal(src.cpu().numpy(), src_h)                                 # sources and bases are only read
        assert np.array_equal(base_d.cpu().numpy(), base_h)
        assert codec.place_stats() == dict(rows=sum(1 for e in exts if e), launches=1)
        assert codec.window_stats() == dict(rows=0, launches=0, staged=0)
        assert codec.delta_stats() == dict(split=0, joined=0, launches=0, staged=0)
        assert codec.planes_stats() == dict(split=0, joined=0, launches=0, staged=0)
    finally:
        if own:
            codec.close()
    return got, doffs


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_every_geometry_at_every_pitch_is_the_map_between_canaries(torch, k):
    rng = np.random.default_rng(38 + k)
    rows = []
    for gi, (n, w) in enumerate(geometries(k)):
        for pi, pitch in enumerate(pitches_of(k, w[4])):
            if pitch == 0:
                continue                                                                # (a window without columns at pitch == cols: no pitch)
            for mode in (NONE, BASE, INPLACE):
                s, d, b = TRIPLES[(gi * 3 + pi * 5 + mode) % len(TRIPLES)]
                rows.append((k, n, w, pitch, s, d, d if mode == INPLACE else b, mode))
    # every (source, destination, base) misalignment of TRIPLES on one geometry that has groups, loose bytes and several window rows,
    # at a pitch that gives every row another alignment
    n, w = 5 * 90 * k, (90 * k, 1, 3, 7 * k, 67 * k)
    rows += [(k, n, w, 67 * k + 1, s, d, b, mode) for (s, d, b) in TRIPLES for mode in (NONE, BASE)]
    rows += [(k, n, w, 67 * k + 1, s, d, d, INPLACE) for s in MIS for d in MIS]
    assert len(rows) > 700
    _run_table(torch, rows, rng)


def test_three_shards_side_by_side_are_the_concatenate(torch):
    """17, 16 and 1 elements wide at pitch 34 k, over 1, 3 and 70 rows, assembled in ONE table per height: the whole destination is
    numpy's concatenate, and again in place against a base"""
    rng = np.random.default_rng(380)
    codec = zpack_amd.Codec(0)
    try:
        for k in (1, 2, 4, 8):
            for nrows in (1, 3, 70):
                widths, pitch = (17, 16, 1), 34 * k
                shards = [rng.integers(0, 256, (nrows, wd * k), dtype=np.uint8) for wd in widths]
                merged = np.concatenate(shards, axis=1)
                assert merged.shape == (nrows, pitch)
                stored = [torch.from_numpy(np.ascontiguousarray(s.reshape(-1, k).T).reshape(-1)).to("cuda:0") for s in shards]       # each shard's byte planes
                prev = rng.integers(0, 256, (nrows, pitch), dtype=np.uint8)
                for inplace in (False, True):
                    dst = torch.from_numpy(prev.copy() if inplace else np.full((nrows, pitch), CANARY, dtype=np.uint8)).to("cuda:0")
                    table = np.zeros(3, dtype=zpack_amd.PLACE_COPY)
                    at = 0
                    for j, (wd, st) in enumerate(zip(widths, stored)):
                        table[j] = (st.data_ptr(), dst.data_ptr() + at, dst.data_ptr() + at if inplace else 0, nrows * wd * k, (wd * k, 0, nrows, 0, wd * k), pitch, k, 0)
                        at += wd * k
                    codec.place_copy_device(table)
                    torch.cuda.synchronize()
                    assert np.array_equal(dst.cpu().numpy(), merged ^ prev if inplace else merged), (k, nrows, inplace)
                    assert codec.place_stats() == dict(rows=3, launches=1)
    finally:
        codec.close()


def test_a_row_whose_first_item_ends_mid_row(torch):
    """cols = 16384 / k + 1 elements: the first item ends one element short of the first row's end, every later item begins mid-row"""
    rng = np.random.default_rng(381)
    rows = []
    for k in (1, 2, 4, 8):
        cols = (16384 // k + 1) * k
        for pi, pitch in enumerate((cols + 1, cols + 4099)):
            for mode in (NONE, BASE, INPLACE):
                s, d, b = TRIPLES[(pi * 3 + mode + k) % len(TRIPLES)]
                rows.append((k, 4 * (cols + 3 * k), (cols + 3 * k, 1, 3, k, cols), pitch, s, d, d if mode == INPLACE else b, mode))
    _run_table(torch, rows, rng)


def test_pitch_equal_to_cols_is_k_window_copy_byte_for_byte(torch):
    rng = np.random.default_rng(382)
    codec = zpack_amd.Codec(0)
    try:
        for k in (1, 2, 4, 8):
            geo = [(n, w) for n, w in geometries(k) if w[2] * w[4]]
            lens = [w[2] * w[4] for _, w in geo]
            soffs, stotal = _place([n for n, _ in geo], [MIS[i % 4] for i in range(len(geo))])
            doffs, dtotal = _place(lens, [MIS[(i // 4) % 4] for i in range(len(geo))])
            src = torch.from_numpy(rng.integers(0, 256, stotal, dtype=np.uint8)).to("cuda:0")
            base = torch.from_numpy(rng.integers(0, 256, dtotal, dtype=np.uint8)).to("cuda:0")
            out = torch.full((2, dtotal), CANARY, dtype=torch.uint8, device="cuda:0")
            wt = np.zeros(len(geo), dtype=zpack_amd.WINDOW_COPY)
            pt = np.zeros(len(geo), dtype=zpack_amd.PLACE_COPY)
            for t, o in ((wt, out[0]), (pt, out[1])):
                t["src"] = src.data_ptr() + np.array(soffs, dtype=np.uint64)
                t["dst"] = o.data_ptr() + np.array(doffs, dtype=np.uint64)
                t["base"] = [base.data_ptr() + do if i % 2 else 0 for i, do in enumerate(doffs)]
                t["n"] = [n for n, _ in geo]
                t["win"] = np.array([w for _, w in geo], dtype=zpack_amd.WINDOW)
                t["elem"] = k
            pt["pitch"] = [w[4] for _, w in geo]
            codec.window_copy_device(wt)
            assert codec.window_stats()["rows"] == len(geo) and codec.place_stats() == dict(rows=0, launches=0)
            codec.place_copy_device(pt)
            assert codec.place_stats() == dict(rows=len(geo), launches=1) and codec.window_stats() == dict(rows=0, launches=0, staged=0)
            torch.cuda.synchronize()
            o = out.cpu().numpy()
            assert np.array_equal(o[0], o[1]) and (o[0] != CANARY).any(), k
    finally:
        codec.close()


def test_rows_of_mixed_element_sizes_in_one_table(torch):
    rng = np.random.default_rng(383)
    rows = []
    for rep in range(3):
        for k in (8, 1, 4, 2):
            g = geometries(k)
            for gi in range(rep, len(g), 7):
                mode = (gi + rep) % 3
                n, w = g[gi]
                pitch = pitches_of(k, w[4])[(gi + rep) % 6] or 5
                s, d, b = TRIPLES[(gi + 5 * rep + k) % len(TRIPLES)]
                rows.append((k, n, w, pitch, s, d, d if mode == INPLACE else b, mode))
    assert len({r[0] for r in rows}) == 4 and len(rows) > 60
    _run_table(torch, rows, rng)


def test_invalid_placements_bad_pointers_and_overlaps_are_refused_and_nothing_runs(torch):
    L = zpack_amd.lib()
    src = torch.arange(8192, dtype=torch.int32, device="cuda:0").view(torch.uint8)      # 32 KiB
    base = torch.arange(8192, dtype=torch.int32, device="cuda:0").view(torch.uint8) + 1
    dst = torch.full((8192 * 4 + 2 * GAP,), CANARY, dtype=torch.uint8, device="cuda:0")
    small = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda:0")
    host = np.zeros(4096, dtype=np.uint8)
    S, B, D = src.data_ptr(), base.data_ptr(), dst.data_ptr() + GAP
    N = 4096                                                                            # the entry: 16 rows of 256 bytes
    W = (256, 2, 4, 32, 64)                                                             # 4 rows of 64 bytes; at pitch 100 the extent is 364 bytes
    P = 100
    good = (S, D, B, N, W, P, 4, 0)
    # (an extent that leaves its allocation: a block of the caching allocator's is at most 20 MiB around a 4 KiB tensor, the window's 256 bytes fit)
    FAR = 8 << 20
    codec = zpack_amd.Codec(0)
    try:
        torch.cuda.synchronize()
        for bad in ((S, D + 4096, B, N, W, 63, 4, 0), (S, D + 4096, B, N, W, 0, 4, 0), (S, D + 4096, B, N, W, 1, 4, 0),       # a pitch below cols
                    (S, D + 4096, B, N, (256, 13, 4, 32, 64), P, 4, 0),                 # the window's own rule
                    (S, D + 4096, B, N, (0, 0, 0, 0, 0), P, 4, 0),
                    (S, D + 4096, B, N, W, (2 ** 64 - 64) // 3 + 1, 4, 0),              # an extent that wraps
                    (S, D + 4096, B, N, W, 2 ** 64 - 1, 4, 0),
                    (S, D + 4096, B, N, W, P, 3, 0), (S, D + 4096, B, N, W, P, 0, 0),   # element sizes
                    (S, small.data_ptr(), 0, N, W, FAR, 4, 0),                          # the extent leaves the allocation; the window's bytes alone would fit
                    (S, D + 4096, small.data_ptr(), N, W, FAR, 4, 0),                   # ... of the base
                    (host.ctypes.data, D + 4096, B, N, W, P, 4, 0), (S, host.ctypes.data, B, N, W, P, 4, 0), (S, D + 4096, host.ctypes.data, N, W, P, 4, 0),   # host memory
                    (0, D + 4096, B, N, W, P, 4, 0), (S, 0, B, N, W, P, 4, 0),
                    (S, D + 4096, D + 4096 + 363, N, W, P, 2, 0), (S, D + 4096 + 363, D + 4096, N, W, P, 2, 0),               # base and destination overlap by one byte
                    (S, D + 4096, D + 4096 + 1, N, W, P, 1, 0), (S, D + 4096, D + 4096 + 64, N, W, P, 8, 0)):                 # ... by more (a base in the gaps included)
            both = np.array([good, bad], dtype=zpack_amd.PLACE_COPY)
            assert L.zpk_codec_place_copy_device(codec.h, both.ctypes.data, 2, None) == -2, bad
        torch.cuda.synchronize()
        assert bool((dst == CANARY).all()) and bool((small == CANARY).all()) and not host.any()       # the good row beside the bad one has not run either
        assert codec.place_stats() == dict(rows=0, launches=0)
        # a row of no bytes passes wherever it points; a base exactly one extent behind its destination passes: both good rows run, and only they
        three = np.array([(0, 0, 0, N, (256, 16, 0, 0, 256), 300, 4, 0), good, (S, D + 8192, D + 8192 + 364, N, W, P, 2, 0)], dtype=zpack_amd.PLACE_COPY)
        assert L.zpk_codec_place_copy_device(codec.h, three.ctypes.data, 3, None) == 0
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        s_h, b_h = src.cpu().numpy(), base.cpu().numpy()
        o = placed_index(W, P)
        want = np.full(got.size, CANARY, dtype=np.uint8)
        want[GAP + o] = window_of(s_h[:N], 4, W) ^ b_h[o]
        want[GAP + 8192 + o] = window_of(s_h[:N], 2, W) ^ CANARY                        # (canaries: the base of the third row)
        assert np.array_equal(got, want)
        assert codec.place_stats() == dict(rows=2, launches=1)
    finally:
        codec.close()
