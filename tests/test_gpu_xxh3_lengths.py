"""XXH3 on the GPU against the oracle over the lengths that decide how xxh3_64_wave walks its input: the serial short path
(0..240), one to four 1 KiB blocks in the last four-block group (rows of the wave that have no block), every count of whole tail
stripes and every offset of the last stripe, the lengths around each multiple of 1 KiB up to 70 KiB, the benchmark's entry size,
a few lengths in the MiB range — each at every source alignment 0..15 mod 16.  k_hash runs the loop with its keys in registers; the
LZ4 decode kernels run the same loop with the keys read from LDS, so entries of as many lengths are decoded and verified as well."""
import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests._libs import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    return zpack_amd.Codec(0)


def _lengths():
    lens = list(range(0, 1301))
    for k in range(1, 71):
        lens += [1024 * k + d for d in (-1, 0, 1, 63, 64, 65)]
    lens += [65535, 65536, 65537]
    return lens


BIG = [(1 << 20) - 1, 1 << 20, (1 << 20) + 1025, (1 << 20) + 2048 + 63, (1 << 20) + 3072 + 64, 3 * (1 << 20) + 4097, (5 << 20) + 777]


def _hash_on_gpu(codec, blob, offs, sizes):
    import torch
    dev = torch.device("cuda:0")
    n = len(offs)
    src = torch.from_numpy(blob).to(dev)
    out = torch.zeros(n, dtype=torch.int64, device=dev)
    codec.hash_batch_device(src, torch.from_numpy(np.asarray(offs, dtype=np.uint64).view(np.int64)).to(dev),
                            torch.from_numpy(np.asarray(sizes, dtype=np.uint64).view(np.int64)).to(dev), n, out)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


def test_hash_batch_every_length_and_alignment(codec):
    o = oracle()
    lens = _lengths()
    blob = dg.fill(dg.RANDOM, 11, 0, (1 << 20) + 71 * 1024 + 64)
    rng = np.random.default_rng(9)
    offs, sizes = [], []
    for n in lens:
        base = int(rng.integers(0, 1 << 20)) & ~15
        for a in range(16):
            offs.append(base + a)
            sizes.append(n)
    got = _hash_on_gpu(codec, blob, offs, sizes)
    want = {}
    bad = []
    for i, (of, n) in enumerate(zip(offs, sizes)):
        w = want.setdefault((of, n), o.xxh3(blob[of:of + n]))
        if int(got[i]) != w:
            bad.append((n, of & 15))
    assert not bad, "%d of %d differ, first (length, offset mod 16): %s" % (len(bad), len(offs), bad[:8])


def test_hash_batch_mib_lengths(codec):
    o = oracle()
    blob = dg.fill(dg.RANDOM, 12, 0, (6 << 20) + 64)
    offs, sizes = [], []
    for j, n in enumerate(BIG):
        for a in range(16):
            offs.append(16 * j + a)
            sizes.append(n)
    got = _hash_on_gpu(codec, blob, offs, sizes)
    for i, (of, n) in enumerate(zip(offs, sizes)):
        assert int(got[i]) == o.xxh3(blob[of:of + n]), (n, of & 15)


@pytest.mark.parametrize("lo,hi,n", [(241, 9000, 600), (60000, 70000, 96)])
def test_lz4_decode_verifies_every_remainder(codec, lo, hi, n):
    """the LZ4 kernels' build of the loop (keys in the dead LDS stage): status OK means the kernel's XXH3 equals the writer's"""
    import torch
    o = oracle()
    b = dg.Batch(n, lo, hi, method=dg.LZ4, level=0, seed=77)
    assert len({((int(s) - 1) >> 10) & 3 for s in b.uncomp_sizes}) == 4          # every count of blocks in the last group
    desc, total = zpack_amd.decode_descs_from_batch(b)
    dev = torch.device("cuda:0")
    src = torch.from_numpy(b.archive).to(dev)
    dst = torch.zeros(total, dtype=torch.uint8, device=dev)
    ddesc = torch.from_numpy(desc.view(np.uint8)).to(dev)
    dres = torch.zeros(n * zpack_amd.DECODE_RESULT.itemsize, dtype=torch.uint8, device=dev)
    codec.decode_batch_device(src, ddesc, n, dst, dres)
    torch.cuda.synchronize()
    res = dres.cpu().numpy().view(zpack_amd.DECODE_RESULT)
    out = dst.cpu().numpy()
    assert (res["status"] == 0).all(), res[res["status"] != 0][:4]
    assert np.array_equal(res["hash"], b.hashes)
    for i in range(0, n, 7):
        d = desc[i]
        assert int(res["hash"][i]) == o.xxh3(out[int(d["dst_offset"]):int(d["dst_offset"] + d["uncomp_size"])])
