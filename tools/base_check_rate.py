#!/usr/bin/env python3
"""What the base check of a delta read costs, and the span-hash kernels alone (a sibling of tools/delta_rate.py, same archive).

  python tools/base_check_rate.py read [--entries 2000] [--pairs 7]
  python tools/base_check_rate.py kernels [--pairs 7]

read: --entries bf16 tensors of 1 MiB against a synthetic base (delta_rate.py's model, lr 1e-3), LZ4 level 0, element size 2, written into
a sink in device memory once; then, behind one warm-up round, --pairs rounds alternate zpk_codec_decode_batch_dimage_delta (the read as
it was: the checked call with no hashes IS that call) and zpk_codec_decode_batch_dimage_delta_checked with the bases' hashes, into
fresh buffers and in place.  The hashes come from zpk_codec_hash_spans_device and are compared with the CPU XXH3 of the first rows.
Medians and ranges; every read is compared with its sources.

kernels: zpk_codec_hash_spans_device alone — 2000 rows of 1 MiB by one wave each (threshold off) and chip-wide (the default threshold),
one row of 2 GiB chip-wide (and 64 MiB of it by one wave, scaled, for what the chip-wide path is there to avoid), and rows of 128, 256 and
512 KiB in calls of 1, 64 and 2000 rows, both ways: where the threshold belongs."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.delta_rate import perturbed, stat      # noqa: E402


def clock(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def cpu_xxh3(data):
    from tests._libs import oracle
    return oracle().xxh3(data)


def read(a):
    import torch
    import zpack_amd as Z
    n, size = a.entries, 1 << 20
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(29)
    base = torch.empty(n * size, dtype=torch.uint8, device=dev)
    src = torch.empty(n * size, dtype=torch.uint8, device=dev)
    for i in range(0, n, 100):
        m = min(100, n - i)
        w = (torch.randn(m * size // 2, generator=g, device=dev) * 0.02).to(torch.bfloat16)
        base[i * size:(i + m) * size] = w.view(torch.uint8)
        src[i * size:(i + m) * size] = perturbed(torch, w, 1e-3, g).view(torch.uint8)
    out = torch.empty(n * size, dtype=torch.uint8, device=dev)
    codec = Z.Codec(0)
    L = Z.lib()
    vp, u64 = C.c_void_p, C.c_uint64
    L.zpk_codec_encode_batch_dsink_delta.argtypes = [vp, vp, C.c_int, vp, u64, vp, u64, vp, C.POINTER(u64), C.POINTER(u64), vp, vp]
    L.zpk_codec_decode_batch_dimage_delta.argtypes = [vp, vp, u64, vp, u64, vp, C.c_int, vp, vp, vp]
    L.zpk_codec_decode_batch_dimage_delta_checked.argtypes = [vp, vp, u64, vp, u64, vp, C.c_int, vp, vp, vp, vp]
    bound = codec.compress_bound(Z.METHOD_LZ4, size)
    sink = torch.empty(n * bound + 64, dtype=torch.uint8, device=dev)
    ed = np.zeros(n, dtype=Z.ENCODE_DESC)
    ed["size"], ed["method"], ed["level"], ed["dst_capacity"] = size, Z.METHOD_LZ4, 0, bound
    arr = lambda t: (vp * n)(*[t.data_ptr() + i * size for i in range(n)])
    sptr, bptr, optr = arr(src), arr(base), arr(out)
    elem = (C.c_uint8 * n)(*([2] * n))
    torch.cuda.synchronize()
    res = np.zeros(n, dtype=Z.ENCODE_RESULT)
    placed, nbytes = u64(0), u64(0)
    rc = L.zpk_codec_encode_batch_dsink_delta(codec.h, sptr, 1, ed.ctypes.data, n, sink.data_ptr(), sink.numel(), res.ctypes.data, C.byref(placed), C.byref(nbytes), elem, bptr)
    assert rc == 0 and placed.value == n and (res["status"] == 0).all()
    dd = np.zeros(n, dtype=Z.DECODE_DESC)
    dd["comp_size"] = res["comp_size"]
    dd["src_offset"] = np.concatenate([[0], np.cumsum(dd["comp_size"])[:-1]])
    dd["uncomp_size"] = dd["dst_capacity"] = size
    dd["expect_hash"] = res["hash"]
    dd["method"] = Z.METHOD_LZ4
    image = sink[:nbytes.value + 1]                                                    # (a pad byte behind the payloads keeps the last entry inside)
    rows = np.zeros(n, dtype=Z.HASH_SPAN)
    rows["addr"], rows["len"] = list(bptr), size
    hashes = codec.hash_spans_device(rows)
    for i in (0, 1, n - 1):
        assert int(hashes[i]) == cpu_xxh3(base[i * size:(i + 1) * size].cpu().numpy().tobytes()), i
    print("%d x 1 MiB bf16 (delta_rate.py's synthetic step at lr 1e-3), LZ4 level 0, element size 2, out of an image in device memory (%d bytes, compressed/plain %.3f);" %
          (n, nbytes.value, nbytes.value / (n * size)))
    print("%d alternating rounds behind one warm-up round.  The bases' hashes: %s" % (a.pairs, codec.base_check_stats()))

    def run(leg):
        r = np.zeros(n, dtype=Z.DECODE_RESULT)
        b = optr if "in place" in leg else bptr
        if leg.startswith("checked"):
            rc = L.zpk_codec_decode_batch_dimage_delta_checked(codec.h, image.data_ptr(), image.numel(), dd.ctypes.data, n, optr, 1, r.ctypes.data, elem, b, hashes.ctypes.data)
        else:
            rc = L.zpk_codec_decode_batch_dimage_delta(codec.h, image.data_ptr(), image.numel(), dd.ctypes.data, n, optr, 1, r.ctypes.data, elem, b)
        assert rc == 0 and (r["status"] == 0).all(), leg

    legs = ("delta", "checked", "delta in place", "checked in place")
    times = {p: [] for p in legs}
    for rep in range(a.pairs + 1):
        for p in legs:
            if "in place" in p:
                out.copy_(base)                                                        # (not timed: the buffer holds the previous checkpoint)
            else:
                out.zero_()
            ms, _ = clock(torch, lambda: run(p))
            if rep:
                times[p].append(ms)
            if rep == 0:
                assert torch.equal(out, src), "the %s read does not return its sources" % p
    for p in legs:
        print("read, %-17s: %s   %7.2f GiB/s of plaintext" % (p, stat(times[p]), n * size / (1 << 30) / (statistics.median(times[p]) / 1e3)))
    med = {p: statistics.median(times[p]) for p in legs}
    print("checked - delta: %.3f ms into fresh buffers, %.3f ms in place, for %.2f GiB of bases (one more read of the base at 5 TB/s: %.2f ms)" %
          (med["checked"] - med["delta"], med["checked in place"] - med["delta in place"], n * size / (1 << 30), n * size / 5e12 * 1e3))
    hs = []
    for rep in range(a.pairs + 1):
        ms, _ = clock(torch, lambda: codec.hash_spans_device(rows))
        if rep:
            hs.append(ms)
    print("the hash pass of the same bases alone (tables up, launches, hashes home): %s   %s" % (stat(hs), codec.base_check_stats()))
    # a wrong base: nothing is delivered
    out.copy_(base)
    wrong = hashes.copy()
    wrong[::2] ^= np.uint64(1)
    r = np.zeros(n, dtype=Z.DECODE_RESULT)
    torch.cuda.synchronize()                                                           # (the codec runs on a stream of its own: the copy above has to have finished)
    rc = L.zpk_codec_decode_batch_dimage_delta_checked(codec.h, image.data_ptr(), image.numel(), dd.ctypes.data, n, optr, 1, r.ctypes.data, elem, optr, wrong.ctypes.data)
    torch.cuda.synchronize()
    assert rc == 0 and (r["status"][::2] == Z.R_BASE_MISMATCH).all() and (r["status"][1::2] == 0).all()
    v, s, b = out.view(n, size), src.view(n, size), base.view(n, size)
    assert torch.equal(v[::2], b[::2]) and torch.equal(v[1::2], s[1::2])
    print("every read returned its sources bit-exact; with every other hash wrong, in place: %d entries BASE_MISMATCH and their bases untouched, %d delivered" % ((n + 1) // 2, n // 2))
    codec.close()


def kernels(a):
    import torch
    import zpack_amd as Z
    dev = torch.device("cuda", 0)
    total = 2 << 30
    buf = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev).manual_seed(30)
    for i in range(0, total, 256 << 20):
        buf[i:i + (256 << 20)] = torch.randint(0, 256, (256 << 20,), generator=g, device=dev, dtype=torch.uint8)
    torch.cuda.synchronize()
    codec = Z.Codec(0)
    at = buf.data_ptr() + 3                                                             # unaligned on purpose

    def table(nrows, size):
        t = np.zeros(nrows, dtype=Z.HASH_SPAN)
        t["addr"] = at + np.arange(nrows, dtype=np.uint64) * np.uint64(size)
        t["len"] = size
        return t

    def timed(t, threshold):
        codec.set_option(Z.OPT_SPAN_HASH_MIN, threshold)
        xs, h = [], None
        for rep in range(a.pairs + 1):
            ms, h = clock(torch, lambda: codec.hash_spans_device(t))
            if rep:
                xs.append(ms)
        return xs, h, codec.base_check_stats()

    def line(what, t, threshold):
        xs, h, st = timed(t, threshold)
        nbytes = int(t["len"].astype(np.uint64).sum())
        print("%-58s %s   %8.1f GB/s   %s" % (what, stat(xs), nbytes / 1e9 / (statistics.median(xs) / 1e3), st))
        return h

    print("zpk_codec_hash_spans_device alone (tables up, launches, hashes home), %d rounds behind one warm-up round" % a.pairs)
    t = table(2000, 1 << 20)
    h1 = line("2000 x 1 MiB, one wave per row (threshold off)", t, 0)
    h2 = line("2000 x 1 MiB, chip-wide (threshold 256 KiB)", t, 256 << 10)
    assert np.array_equal(h1, h2)
    assert int(h1[7]) == cpu_xxh3(buf[3 + 7 * (1 << 20):3 + 8 * (1 << 20)].cpu().numpy().tobytes())
    big = table(1, total)
    hb = line("1 x 2 GiB, chip-wide", big, 256 << 10)
    part = table(1, 64 << 20)
    hp = line("1 x 64 MiB by ONE wave (x 32 for 2 GiB)", part, 0)
    assert int(hp[0]) == int(line("1 x 64 MiB, chip-wide", part, 256 << 10)[0])
    assert int(hb[0]) == cpu_xxh3(buf[3:3 + total].cpu().numpy().tobytes())
    print("rows of 128, 256 and 512 KiB, one wave per row against chip-wide:")
    for size in (128 << 10, 256 << 10, 512 << 10):
        for nrows in (1, 64, 2000):
            t = table(nrows, size)
            ha = line("%4d x %3d KiB, one wave per row" % (nrows, size >> 10), t, 0)
            hw = line("%4d x %3d KiB, chip-wide" % (nrows, size >> 10), t, 1)
            assert np.array_equal(ha, hw)
    codec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("read", "kernels"))
    ap.add_argument("--entries", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=7)
    a = ap.parse_args()
    (read if a.what == "read" else kernels)(a)


if __name__ == "__main__":
    main()
