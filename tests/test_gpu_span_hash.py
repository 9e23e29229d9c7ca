"""k_span_hash and the chip-wide pair behind it, through zpk_codec_hash_spans_device: the XXH3-64 of arbitrary device spans against the CPU
XXH3 of the oracle — every length at which the hash or the kernels take another path, at pointer offsets 0, 1, 3 and 15 from a 256-byte
boundary, mixed in one call in three orders, with the chip-wide threshold lowered to 4 KiB, at its default, at its least and off; 3000
short rows in one launch; one unaligned row of three groups; the call's refusals and counters.  The sources are only read."""
import numpy as np
import pytest

import zpack_amd
from tests._libs import oracle
from tests.device_mem import torch      # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

T = 4096                                                                             # the lowered threshold: chip-wide rows stay small
LENGTHS = [0, 1, 16, 17, 128, 129, 240, 241, 1023, 1024, 1025, 2049, 65535, 65536, 65537, 65536 + 1025, T - 1, T, T + 1025]
OFFSETS = [0, 1, 3, 15]
BIG = 130 * 1024 + 77                                                                # 130 full blocks in front of the last byte's: three groups of 64


@pytest.fixture(scope="module")
def rows(torch):
    """[(offset in the buffer, len)], the device buffer, its host copy and the oracle's hash of every row, computed once.  Rows: every
    length at every pointer offset, random bytes; one all-zero and one all-0xFF row; the long unaligned one."""
    rng = np.random.default_rng(30)
    spec = [(n, o, "random") for n in LENGTHS for o in OFFSETS] + [(T + 1025, 3, "zero"), (65536 + 1025, 1, "ff"), (300, 15, "zero"), (BIG, 3, "random")]
    pos, where = 256, []
    for n, o, _ in spec:
        where.append((pos + o, n))
        pos = (pos + o + n + 64 + 255) & ~255                                         # at least 64 bytes between rows, each from a 256-byte boundary
    host = rng.integers(0, 256, pos + 256, dtype=np.uint8)
    for (at, n), (_, _, kind) in zip(where, spec):
        if kind != "random":
            host[at:at + n] = 0 if kind == "zero" else 0xFF
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    assert dev.data_ptr() % 256 == 0
    o = oracle()
    want = np.array([o.xxh3(host[at:at + n].tobytes()) for at, n in where], dtype=np.uint64)
    assert want[0] == o.xxh3(b"") and len(set(want.tolist())) > len(want) - 8           # (the four empty rows share one value)
    return dict(where=where, host=host, dev=dev, want=want)


def _table(dev, where, order):
    t = np.zeros(len(order), dtype=zpack_amd.HASH_SPAN)
    t["addr"] = [dev.data_ptr() + where[i][0] for i in order]
    t["len"] = [where[i][1] for i in order]
    return t


def _wide(n, threshold):
    return threshold is not None and n >= max(threshold, 1025)


@pytest.mark.parametrize("threshold", [pytest.param(T, id="4KiB"), pytest.param(256 << 10, id="default"), pytest.param(1, id="least"), pytest.param(None, id="never")])
def test_every_length_at_every_offset_mixed_in_one_call_in_three_orders(torch, rows, threshold):
    r = rows
    n = len(r["where"])
    by_len = sorted(range(n), key=lambda i: (r["where"][i][1], i))
    orders = dict(ascending=by_len, descending=by_len[::-1], shuffled=list(np.random.default_rng(7).permutation(n)))
    codec = zpack_amd.Codec(0)
    try:
        if threshold != 256 << 10:                                                    # (the default is not set: it is what a fresh codec has)
            codec.set_option(zpack_amd.OPT_SPAN_HASH_MIN, 0 if threshold is None else threshold)
        wide = sum(1 for _, ln in r["where"] if _wide(ln, threshold))
        for name, order in orders.items():
            got = codec.hash_spans_device(_table(r["dev"], r["where"], order))
            bad = [(r["where"][i], hex(int(g)), hex(int(r["want"][i]))) for g, i in zip(got, order) if g != r["want"][i]]
            assert not bad, (name, len(bad), bad[:4])
            assert codec.base_check_stats() == dict(wave=n - wide, wide=wide, refused=0, launches=(1 if n - wide else 0) + (2 if wide else 0)), name
        assert wide == {T: 27, 1: 39}.get(threshold, 0)                      # (the default takes nothing here: no row has 256 KiB)
    finally:
        codec.close()
    assert np.array_equal(r["dev"].cpu().numpy(), r["host"])                            # the spans are only read


def test_three_thousand_short_rows_in_one_launch(torch):
    rng = np.random.default_rng(31)
    host = rng.integers(0, 256, 3000 * 301 + 15, dtype=np.uint8)
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    where = [(i * 301 + 15, 300) for i in range(3000)]                                # back to back at every alignment, one byte between them
    o = oracle()
    want = np.array([o.xxh3(host[at:at + n].tobytes()) for at, n in where], dtype=np.uint64)
    codec = zpack_amd.Codec(0)
    try:
        codec.set_option(zpack_amd.OPT_SPAN_HASH_MIN, T)
        got = codec.hash_spans_device(_table(dev, where, range(3000)))
        assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0])
        assert codec.base_check_stats() == dict(wave=3000, wide=0, refused=0, launches=1)
    finally:
        codec.close()


def test_one_unaligned_row_of_three_groups_alone_and_the_same_row_by_one_wave(torch, rows):
    r = rows
    i = len(r["where"]) - 1
    assert r["where"][i][1] == BIG and r["where"][i][0] % 256 == 3
    codec = zpack_amd.Codec(0)
    try:
        for threshold, counts in ((T, dict(wave=0, wide=1, refused=0, launches=2)), (0, dict(wave=1, wide=0, refused=0, launches=1))):
            codec.set_option(zpack_amd.OPT_SPAN_HASH_MIN, threshold)
            got = codec.hash_spans_device(_table(r["dev"], r["where"], [i]))
            assert int(got[0]) == int(r["want"][i]) and codec.base_check_stats() == counts, threshold
    finally:
        codec.close()


def test_a_row_that_leaves_its_allocation_is_refused_and_nothing_runs(torch, rows):
    r = rows
    codec = zpack_amd.Codec(0)
    try:
        total = r["dev"].numel()
        t = _table(r["dev"], r["where"], [0, 5, 9])
        t["addr"][1] = r["dev"].data_ptr() + total - 8                                 # 16 bytes from 8 in front of the end
        t["len"][1] = 1 << 30
        with pytest.raises(RuntimeError, match="span 1 is not"):
            codec.hash_spans_device(t)
        assert codec.base_check_stats() == dict(wave=0, wide=0, refused=0, launches=0)
        host = np.zeros(64, dtype=np.uint8)
        t = np.zeros(1, dtype=zpack_amd.HASH_SPAN)
        t["addr"], t["len"] = host.ctypes.data, 64                                     # host memory is no device span
        with pytest.raises(RuntimeError):
            codec.hash_spans_device(t)
        t["addr"], t["len"] = 0, 0                                                     # no bytes: the address is not looked at
        assert int(codec.hash_spans_device(t)[0]) == oracle().xxh3(b"")
        assert len(codec.hash_spans_device(np.zeros(0, dtype=zpack_amd.HASH_SPAN))) == 0
    finally:
        codec.close()
