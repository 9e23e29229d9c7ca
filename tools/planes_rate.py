#!/usr/bin/env python3
"""What byte planes cost: the planes calls against the plain calls on the same tensors, and k_plane_copy against k_span_copy.

  python tools/planes_rate.py [--entries 2000] [--pairs 7]

--entries bf16 tensors of 1 MiB (randn * 0.02) are written into a sink in device memory (zpk_codec_encode_batch_dsink / _planes, device
sources) and read out of an image in device memory (zpk_codec_decode_batch_dimage / _planes, device destinations), LZ4 level 0.  After a
warm-up round, --pairs rounds alternate plain, planes, grouped, plain, planes, grouped ...; the median and the range of each are printed,
and the same for the two copy kernels alone on the same rows.  "grouped" is the PLAIN call on buffers that already hold the grouped bytes:
it compresses and decodes the very bytes the planes call does, so planes against grouped is what the transposition in the copy costs,
and plain against grouped is what the codec does differently on bytes that compress.  (the two copy kernels alone: (zpk_codec_copy_spans_device, zpk_codec_plane_copy_device: split and join.)  The plain calls
run the code objects of the commit before byte planes, unchanged (tools/code_objects.py)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stat(xs):
    return "median %8.3f ms  (%8.3f .. %8.3f)" % (statistics.median(xs), min(xs), max(xs))


def main():
    import torch
    import zpack_amd as Z
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=7)
    a = ap.parse_args()
    n, size = a.entries, 1 << 20
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(28)
    src = torch.empty(n * size, dtype=torch.uint8, device=dev)
    for i in range(0, n, 100):
        m = min(100, n - i)
        src[i * size:(i + m) * size] = (torch.randn(m * size // 2, generator=g, device=dev) * 0.02).to(torch.bfloat16).view(torch.uint8)
    out = torch.empty(n * size, dtype=torch.uint8, device=dev)
    codec = Z.Codec(0)
    bound = codec.compress_bound(Z.METHOD_LZ4, size)
    legs = ("plain", "planes", "grouped")
    sink = {p: torch.empty(n * bound + 64, dtype=torch.uint8, device=dev) for p in legs}
    pre = torch.empty_like(src)                                                        # the grouped bytes, made by the kernel itself
    ed = np.zeros(n, dtype=Z.ENCODE_DESC)
    ed["size"], ed["method"], ed["level"], ed["dst_capacity"] = size, Z.METHOD_LZ4, 0, bound
    sptr = [src.data_ptr() + i * size for i in range(n)]
    gptr = [pre.data_ptr() + i * size for i in range(n)]
    optr = [out.data_ptr() + i * size for i in range(n)]
    elem = {"plain": None, "planes": [2] * n, "grouped": None}
    from_ = {"plain": sptr, "planes": sptr, "grouped": gptr}
    rows = np.zeros(n, dtype=Z.PLANE_COPY)
    rows["src"], rows["dst"], rows["len"], rows["elem"] = sptr, gptr, size, 2
    codec.plane_copy_device(rows)
    total_mib = n * size / (1 << 20)
    torch.cuda.synchronize()

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    # ---- the write into a device sink ----
    times = {p: [] for p in legs}
    res = {}
    for rep in range(a.pairs + 1):
        for p in legs:
            ms, r = clock(lambda: codec.encode_batch_dsink(from_[p], ed, sink[p], src_on_device=True, elem=elem[p]))
            assert r[1] == n and (r[0]["status"] == 0).all()
            res[p] = r
            if rep:
                times[p].append(ms)
    assert res["planes"][2] == res["grouped"][2] and torch.equal(sink["planes"][:res["planes"][2]], sink["grouped"][:res["grouped"][2]])
    print("%d x 1 MiB bf16 (randn * 0.02), LZ4 level 0, %d alternating rounds behind one warm-up round" % (n, a.pairs))
    print("(plain: the tensors as they are; planes: the same tensors, element size 2; grouped: the plain call on buffers that already hold the grouped bytes —")
    print(" the planes call and the grouped call wrote the same %d bytes)" % res["planes"][2])
    for p in legs:
        print("write into a device sink, %-7s: %s   %7.2f GiB/s of plaintext   compressed/plain %.3f" %
              (p, stat(times[p]), total_mib / 1024 / (statistics.median(times[p]) / 1e3), res[p][2] / (n * size)))
    # ---- the read out of a device image: the sinks ARE images of payloads back to back; a pad byte behind them keeps the last entry inside ----
    dd = {}
    for p in legs:
        d = np.zeros(n, dtype=Z.DECODE_DESC)
        d["comp_size"] = res[p][0]["comp_size"]
        d["src_offset"] = np.concatenate([[0], np.cumsum(d["comp_size"])[:-1]])
        d["uncomp_size"] = d["dst_capacity"] = size
        d["expect_hash"] = res[p][0]["hash"]
        d["method"] = Z.METHOD_LZ4
        dd[p] = d
    times = {p: [] for p in legs}
    for rep in range(a.pairs + 1):
        for p in legs:
            image = sink[p][:res[p][2] + 1]
            ms, r = clock(lambda: codec.decode_batch_dimage(image, dd[p], optr, elem=elem[p]))
            assert (r["status"] == 0).all()
            if rep:
                times[p].append(ms)
            if rep == 0:
                assert torch.equal(out, pre if p == "grouped" else src), "the %s read does not return its sources" % p
            if p == "planes":
                joined = codec.planes_stats()
    for p in legs:
        print("read out of a device image, %-7s: %s   %7.2f GiB/s of plaintext" % (p, stat(times[p]), total_mib / 1024 / (statistics.median(times[p]) / 1e3)))
    print("every read returned its sources bit-exact; the planes read: %s" % joined)
    # ---- the two copy kernels alone, the same rows ----
    spans = np.array([[s, o, size] for s, o in zip(sptr, optr)], dtype=np.uint64)
    rows["dst"] = optr
    kt = {"k_span_copy": [], "k_plane_copy split": [], "k_plane_copy join": []}
    for rep in range(a.pairs + 1):
        for name in kt:
            if name == "k_span_copy":
                ms, _ = clock(lambda: codec.copy_spans_device(spans))
            else:
                rows["join"] = 1 if name.endswith("join") else 0
                ms, _ = clock(lambda: codec.plane_copy_device(rows))
            if rep:
                kt[name].append(ms)
    for name, xs in kt.items():
        print("%-18s alone (table upload + launch + kernel, %d rows of 1 MiB): %s   %7.1f GB/s read + written" %
              (name, n, stat(xs), 2 * n * size / 1e9 / (statistics.median(xs) / 1e3)))
    codec.close()


if __name__ == "__main__":
    main()
