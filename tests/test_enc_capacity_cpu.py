"""zpk_codec_compress_bound against what k_encode DEMANDS of a slot.  tests/test_abi_cpu.py pins the bound to values of the reference;
nothing said that a slot of the bound is one the kernel accepts, for every length.

Form chosen: the exported C function is called for EVERY n of the dense range (600 000 ctypes calls, well under a second); numpy only
compares.  No restatement of the bound in Python stands between the test and the library."""
import numpy as np

import zpack_amd
from zpack_amd import METHOD_NONE, METHOD_ZSTD, METHOD_LZ4

METHODS = (METHOD_NONE, METHOD_ZSTD, METHOD_LZ4)
DENSE = 200000


def min_capacity(method, n):
    """The smallest dst_capacity with which k_encode takes an entry of n bytes: the all-stored frame.  zpack_amd/csrc/zpk_encode.inc,
    k_encode: stored `cap < len` (:1251); LZ4 `cap < hdr + nblocks * 4 + len + 4`, hdr = 7, nblocks = ceil(len / 65536) (:1257-1259);
    Zstandard `cap < zhdr + nblocks * 3 + len`, zhdr = 5 + fcs_bytes, nblocks = max(1, ceil(len / 65536)), fcs_bytes 1 below 256,
    2 below 65536 + 256, 4 up to 2^32 - 1, else 8 (:1286-1289)."""
    n = int(n)
    if method == METHOD_NONE:
        return n
    if method == METHOD_LZ4:
        return 7 + 4 * ((n + 65535) >> 16) + n + 4
    assert method == METHOD_ZSTD
    fcs = 1 if n < 256 else (2 if n < 65536 + 256 else (4 if n <= 0xFFFFFFFF else 8))
    return 5 + fcs + 3 * max(1, (n + 65535) >> 16) + n


def _points():
    pts = [k * 65536 + d for k in list(range(1, 65)) + [4096, 65535, 65536] for d in (-2, -1, 0, 1, 2)]
    pts += [255, 256, 257, 65536 + 255, 65536 + 256, 65536 + 257, 2**32 - 1, 2**32, 2**32 + 1]
    return pts


def test_min_capacity_is_the_all_stored_frame():
    """... spelled out at the lengths where its terms switch (a slip in the function above would weaken every test that uses it)."""
    assert [min_capacity(METHOD_LZ4, n) for n in (0, 1, 65536, 65537, 131072, 131073)] == [11, 16, 65551, 65556, 131091, 131096]
    assert [min_capacity(METHOD_ZSTD, n) for n in (0, 1, 255, 256, 65536, 65537, 65791, 65792, 131072, 131073)] == \
        [9, 10, 264, 266, 65546, 65550, 65804, 65807, 131087, 131091]
    assert min_capacity(METHOD_ZSTD, 2**32 - 1) == 9 + 3 * 65536 + 2**32 - 1 and min_capacity(METHOD_ZSTD, 2**32) == 13 + 3 * 65536 + 2**32
    assert min_capacity(METHOD_NONE, 12345) == 12345


def test_the_bound_covers_what_the_kernel_demands():
    bound = zpack_amd.lib().zpk_codec_compress_bound
    for m in METHODS:
        got = np.array([bound(m, n) for n in range(DENSE + 1)], dtype=np.uint64)
        ns = np.arange(DENSE + 1, dtype=np.uint64)
        if m == METHOD_NONE:
            need = ns
        elif m == METHOD_LZ4:
            need = 11 + 4 * ((ns + 65535) >> 16) + ns
        else:
            need = 5 + np.where(ns < 256, 1, np.where(ns < 65536 + 256, 2, 4)).astype(np.uint64) + 3 * np.maximum(1, (ns + 65535) >> 16) + ns
        spot = list(range(0, DENSE + 1, 97)) + [255, 256, 65535, 65536, 65537, 65791, 65792, 131072, 131073, DENSE]
        assert [int(need[n]) for n in spot] == [min_capacity(m, n) for n in spot]           # the vectorised form IS min_capacity
        short = np.nonzero(got < need)[0]
        assert short.size == 0, (m, short[:8], got[short[:8]], need[short[:8]])
        falls = np.nonzero(got[1:] < got[:-1])[0]
        assert falls.size == 0, (m, falls[:8])                                               # non-decreasing
        for n in _points():
            assert bound(m, n) >= min_capacity(m, n), (m, n, bound(m, n), min_capacity(m, n))
        assert bound(m, 2**32 + 1) >= bound(m, 2**32) >= bound(m, 2**32 - 1)
