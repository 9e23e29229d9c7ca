#!/usr/bin/env python3
"""What delta entries gain and what the XOR costs.

  python tools/delta_rate.py ratio [--mib 64]
  python tools/delta_rate.py rate [--entries 2000] [--pairs 7]

The base is SYNTHETIC, not a training run: w = randn * 0.02 is the base, w' = w + lr * 0.02 * U(0, 3) * sign (sign +-1, both uniform), rounded
to the dtype, is the tensor that is written.  At lr 1e-3 and 1e-4 most bf16 values do not move at all.

ratio: compressed size over plain size of bf16, fp16 and fp32 tensors, --mib MiB per dtype as entries of 1 MiB, through THIS project's
device encoders (zpack_amd/device_io.py) at LZ4 level 0 and Zstandard levels 1 and 3, in four variants — as is, grouped (planes=), XOR
alone (base=) and XOR grouped (both) —, each archive read back and compared before its figure is printed.  In brackets: liblz4 / libzstd
on the CPU over the first 4 MiB of the same stored bytes, when this machine has the libraries.  The sizes are the entries' compressed
bytes: the archive without header, CDR and EOCDR.

rate: --entries bf16 tensors of 1 MiB, LZ4 level 0, written into a sink in device memory and read out of an image in device memory.  After
a warm-up round --pairs rounds alternate the DELTA call (tensor, base, element size 2) and the PLANES call on buffers that already hold
tensor XOR base: both compress and decode the very same bytes, so the difference is what the XOR in the copy costs.  Then the kernels
alone on the same rows: k_plane_copy split and join against k_delta_copy split, join and join in place.  Medians and ranges."""
import argparse
import ctypes as C
import ctypes.util
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stat(xs):
    return "median %8.3f ms  (%8.3f .. %8.3f)" % (statistics.median(xs), min(xs), max(xs))


def perturbed(torch, w, lr, g):
    """the model of the module's docstring, computed in fp32 and rounded to w's dtype"""
    u = torch.rand(w.shape, generator=g, device=w.device) * 3.0
    s = (torch.randint(0, 2, w.shape, generator=g, device=w.device).float() * 2.0 - 1.0)
    return (w.float() + lr * 0.02 * u * s).to(w.dtype)


def grouped(a, k):
    m = a.size // k
    return np.concatenate([a[:m * k].reshape(m, k).T.reshape(-1), a[m * k:]])


class CpuLibs:
    """liblz4 and libzstd through ctypes, each None when this machine does not have it"""
    def __init__(self):
        self.lz4 = self.zstd = None
        for attr, name in (("lz4", "lz4"), ("zstd", "zstd")):
            path = ctypes.util.find_library(name)
            try:
                setattr(self, attr, C.CDLL(path) if path else None)
            except OSError:
                pass
        if self.lz4 is not None:
            self.lz4.LZ4_compress_default.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
            self.lz4.LZ4_compressBound.argtypes = [C.c_int]
        if self.zstd is not None:
            self.zstd.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
            self.zstd.ZSTD_compress.restype = C.c_size_t
            self.zstd.ZSTD_compressBound.argtypes = [C.c_size_t]
            self.zstd.ZSTD_compressBound.restype = C.c_size_t

    def ratio(self, codec, chunks):
        """compressed / plain over `chunks` (np.uint8 arrays of 1 MiB), or None"""
        got = 0
        for a in chunks:
            a = np.ascontiguousarray(a)
            if codec == "lz4":
                if self.lz4 is None:
                    return None
                cap = self.lz4.LZ4_compressBound(a.size)
                out = np.empty(cap, dtype=np.uint8)
                got += min(self.lz4.LZ4_compress_default(a.ctypes.data, out.ctypes.data, a.size, cap), a.size)      # (an incompressible block is stored)
            else:
                if self.zstd is None:
                    return None
                cap = self.zstd.ZSTD_compressBound(a.size)
                out = np.empty(cap, dtype=np.uint8)
                got += self.zstd.ZSTD_compress(out.ctypes.data, cap, a.ctypes.data, a.size, int(codec.split("-")[1]))
        return got / sum(a.size for a in chunks)


def ratio(a):
    import torch
    from zpack_amd import device_io as io
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(29)
    cpu = CpuLibs()
    codecs = (("lz4", io.METHOD_LZ4, 0), ("zstd-1", io.METHOD_ZSTD, 1), ("zstd-3", io.METHOD_ZSTD, 3))
    print("compressed size / plain size through this project's device encoders, %d MiB per dtype as entries of 1 MiB; the base is SYNTHETIC:" % a.mib)
    print("base = randn * 0.02, tensor = base + lr * 0.02 * U(0, 3) * sign, rounded to the dtype.  In brackets: the CPU library over 4 MiB of the same stored bytes.")
    print("| dtype | codec | as is | grouped | XOR alone, lr 1e-3 | XOR grouped, lr 1e-3 | XOR alone, lr 1e-4 | XOR grouped, lr 1e-4 |")
    print("|---|---|---|---|---|---|---|---|")

    def cell(r, c):
        return "%.3f (%s)" % (r, "n/a" if c is None else "%.3f" % c)

    for tag, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16), ("fp32", torch.float32)):
        k = torch.empty(0, dtype=dt).element_size()
        names = ["%s.%03d" % (tag, i) for i in range(a.mib)]
        base = {n: (torch.randn((1 << 20) // k, generator=g, device=dev) * 0.02).to(dt) for n in names}
        new = {lr: {n: perturbed(torch, w, lr, g) for n, w in base.items()} for lr in (1e-3, 1e-4)}
        unchanged = {lr: sum(int((new[lr][n] == base[n]).sum()) for n in names) / (a.mib * ((1 << 20) // k)) for lr in new}
        plain_bytes = a.mib << 20
        fixed = 10 + 20 + sum(35 + len(n) for n in names) + 12
        planes = {n: k for n in names}
        for name, method, level in codecs:
            cells = []
            for lr, use_planes, use_base in ((1e-3, False, False), (1e-3, True, False), (1e-3, False, True), (1e-3, True, True), (1e-4, False, True), (1e-4, True, True)):
                tensors = new[lr]
                kw = dict(planes=planes if use_planes else None, base=base if use_base else None)
                image = io.write_archive_device(tensors, method=method, level=level, **kw)
                outs, status = io.read_files_device(image, **kw)
                if not (status == [0] * len(names) and all(torch.equal(o.view(dt), t) for o, t in zip(outs, tensors.values()))):
                    raise SystemExit("%s %s planes=%s base=%s: the archive does not read back" % (tag, name, use_planes, use_base))
                assert io.test_files(image) == [0] * len(names)
                chunks = []
                for n in names[:4]:                                                       # what the CPU library is given: the bytes this variant stores
                    b = tensors[n].view(torch.uint8).cpu().numpy()
                    if use_base:
                        b = b ^ base[n].view(torch.uint8).cpu().numpy()
                    chunks.append(grouped(b, k) if use_planes else b)
                cells.append(cell((image.numel() - fixed) / plain_bytes, cpu.ratio(name, chunks)))
                del image, outs
            print("| %s | %s | %s |" % (tag, name, " | ".join(cells)))
        print("(%s: %.1f %% of the values are unchanged at lr 1e-3, %.1f %% at lr 1e-4)" % (tag, 100 * unchanged[1e-3], 100 * unchanged[1e-4]))
        del base, new
    print("every archive above was read back bit-exact and passes zpack_amd_test_files")


def rate(a):
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
    xor = src ^ base                                                                   # what the planes call is handed
    out = torch.empty(n * size, dtype=torch.uint8, device=dev)
    codec = Z.Codec(0)
    L = Z.lib()
    vp, u64 = C.c_void_p, C.c_uint64
    L.zpk_codec_encode_batch_dsink_delta.argtypes = [vp, vp, C.c_int, vp, u64, vp, u64, vp, C.POINTER(u64), C.POINTER(u64), vp, vp]
    L.zpk_codec_decode_batch_dimage_delta.argtypes = [vp, vp, u64, vp, u64, vp, C.c_int, vp, vp, vp]
    bound = codec.compress_bound(Z.METHOD_LZ4, size)
    legs = ("delta", "planes")
    sink = {p: torch.empty(n * bound + 64, dtype=torch.uint8, device=dev) for p in legs}
    ed = np.zeros(n, dtype=Z.ENCODE_DESC)
    ed["size"], ed["method"], ed["level"], ed["dst_capacity"] = size, Z.METHOD_LZ4, 0, bound
    arr = lambda t: (vp * n)(*[t.data_ptr() + i * size for i in range(n)])
    sptr, bptr, xptr, optr = arr(src), arr(base), arr(xor), arr(out)
    elem = (C.c_uint8 * n)(*([2] * n))
    total_mib = n * size / (1 << 20)
    torch.cuda.synchronize()

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def write(p):
        res = np.zeros(n, dtype=Z.ENCODE_RESULT)
        placed, nbytes = u64(0), u64(0)
        rc = L.zpk_codec_encode_batch_dsink_delta(codec.h, sptr if p == "delta" else xptr, 1, ed.ctypes.data, n, sink[p].data_ptr(), sink[p].numel(), res.ctypes.data,
                                                  C.byref(placed), C.byref(nbytes), elem, bptr if p == "delta" else None)
        assert rc == 0 and placed.value == n and (res["status"] == 0).all()
        return res, nbytes.value

    times = {p: [] for p in legs}
    res = {}
    for rep in range(a.pairs + 1):
        for p in legs:
            ms, res[p] = clock(lambda: write(p))
            if rep:
                times[p].append(ms)
    assert res["delta"][1] == res["planes"][1] and torch.equal(sink["delta"][:res["delta"][1]], sink["planes"][:res["planes"][1]])
    print("%d x 1 MiB bf16 (base randn * 0.02, tensor = base moved by the synthetic step at lr 1e-3), LZ4 level 0, element size 2, %d alternating rounds behind one warm-up round" % (n, a.pairs))
    print("(delta: tensor and base; planes: the planes call on buffers that already hold tensor XOR base — both wrote the same %d bytes, compressed/plain %.3f)" %
          (res["delta"][1], res["delta"][1] / (n * size)))
    for p in legs:
        print("write into a device sink, %-6s: %s   %7.2f GiB/s of plaintext" % (p, stat(times[p]), total_mib / 1024 / (statistics.median(times[p]) / 1e3)))
    dd = np.zeros(n, dtype=Z.DECODE_DESC)
    dd["comp_size"] = res["delta"][0]["comp_size"]
    dd["src_offset"] = np.concatenate([[0], np.cumsum(dd["comp_size"])[:-1]])
    dd["uncomp_size"] = dd["dst_capacity"] = size
    dd["expect_hash"] = res["delta"][0]["hash"]
    dd["method"] = Z.METHOD_LZ4
    image = sink["delta"][:res["delta"][1] + 1]                                        # (a pad byte behind the payloads keeps the last entry inside)

    def read(p):
        r = np.zeros(n, dtype=Z.DECODE_RESULT)
        rc = L.zpk_codec_decode_batch_dimage_delta(codec.h, image.data_ptr(), image.numel(), dd.ctypes.data, n, optr, 1, r.ctypes.data, elem,
                                                   None if p == "planes" else optr if p == "in place" else bptr)
        assert rc == 0 and (r["status"] == 0).all()

    rlegs = ("delta", "in place", "planes")
    times = {p: [] for p in rlegs}
    for rep in range(a.pairs + 1):
        for p in rlegs:
            if p == "in place":
                out.copy_(base)                                                        # (not timed: the buffer holds the previous checkpoint)
            ms, _ = clock(lambda: read(p))
            if rep:
                times[p].append(ms)
            if rep == 0:
                assert torch.equal(out, xor if p == "planes" else src), "the %s read does not return its sources" % p
    for p in rlegs:
        print("read out of a device image, %-8s: %s   %7.2f GiB/s of plaintext" % (p, stat(times[p]), total_mib / 1024 / (statistics.median(times[p]) / 1e3)))
    print("every read returned its sources bit-exact (in place: the buffer held the base and holds the tensor)")
    # ---- the kernels alone, the same rows ----
    prow = np.zeros(n, dtype=Z.PLANE_COPY)
    prow["src"], prow["dst"], prow["len"], prow["elem"] = list(sptr), list(optr), size, 2
    drow = np.zeros(n, dtype=Z.DELTA_COPY)
    drow["src"], drow["dst"], drow["base"], drow["len"], drow["elem"] = list(sptr), list(optr), list(bptr), size, 2
    inrow = drow.copy()
    inrow["base"], inrow["join"] = inrow["dst"], 1
    kt = {"k_plane_copy split": [], "k_delta_copy split": [], "k_plane_copy join": [], "k_delta_copy join": [], "k_delta_copy join in place": []}
    for rep in range(a.pairs + 1):
        for name in kt:
            if name.startswith("k_plane"):
                prow["join"] = 1 if name.endswith("join") else 0
                ms, _ = clock(lambda: codec.plane_copy_device(prow))
            elif name.endswith("in place"):
                ms, _ = clock(lambda: codec.delta_copy_device(inrow))
            else:
                drow["join"] = 1 if name.endswith("join") else 0
                ms, _ = clock(lambda: codec.delta_copy_device(drow))
            if rep:
                kt[name].append(ms)
    for name, xs in kt.items():
        streams = 2 if name.startswith("k_plane") else 3
        print("%-27s alone (table upload + launch + kernel, %d rows of 1 MiB): %s   %7.1f GB/s over its %d streams" %
              (name, n, stat(xs), streams * n * size / 1e9 / (statistics.median(xs) / 1e3), streams))
    med = {k: statistics.median(v) for k, v in kt.items()}
    print("k_delta_copy / k_plane_copy: split %.2f, join %.2f, join in place %.2f  (3 bytes moved per plaintext byte against 2: 1.50 expected)" %
          (med["k_delta_copy split"] / med["k_plane_copy split"], med["k_delta_copy join"] / med["k_plane_copy join"], med["k_delta_copy join in place"] / med["k_plane_copy join"]))
    codec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("ratio", "rate"))
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--entries", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=7)
    a = ap.parse_args()
    (ratio if a.what == "ratio" else rate)(a)


if __name__ == "__main__":
    main()
