#!/usr/bin/env python3
"""What a window read saves, and what k_window_copy costs beside the joins of whole entries.

  python tools/window_read_rate.py [--entries 2000] [--pairs 7]

--entries bf16 tensors of 1 MiB, each a (512, 1024) matrix, written as delta entries (element size 2, a base per entry: the synthetic
step of tools/delta_rate.py at lr 1e-3) at LZ4 level 0 into a sink in device memory and read out of that image.  Two windows of 1/8 of
every tensor: rows [64, 128) — a slice along dimension 0, ONE window row of 128 KiB — and columns [128, 256) — a slice along the last
dimension, 512 window rows of 256 bytes.  After a warm-up round --pairs rounds alternate the legs; medians and ranges.

(a) the call: zpk_codec_decode_batch_dimage_windows with the base's shard of window size, against what a caller does today — the _delta
    read into full-size tensors, then a torch slice made contiguous (the allocation of the slice is inside the clock: the caller pays it).
(b) the kernels alone on the same stored bytes: k_window_copy for both windows, without a base and with one, against k_plane_copy and
    k_delta_copy joining the same entries whole."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS, COLS, K = 512, 1024, 2                     # the tensor: 512 x 1024 bf16
SIZE = ROWS * COLS * K


def stat(xs):
    return "median %8.3f ms  (%8.3f .. %8.3f)" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=7)
    a = ap.parse_args()
    import torch
    import zpack_amd as Z
    from tools.delta_rate import perturbed
    n = a.entries
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(34)
    base = torch.empty(n * SIZE, dtype=torch.uint8, device=dev)
    src = torch.empty(n * SIZE, dtype=torch.uint8, device=dev)
    for i in range(0, n, 100):
        m = min(100, n - i)
        w = (torch.randn(m * SIZE // K, generator=g, device=dev) * 0.02).to(torch.bfloat16)
        base[i * SIZE:(i + m) * SIZE] = w.view(torch.uint8)
        src[i * SIZE:(i + m) * SIZE] = perturbed(torch, w, 1e-3, g).view(torch.uint8)
    out = torch.empty(n * SIZE, dtype=torch.uint8, device=dev)
    codec = Z.Codec(0)
    L = Z.lib()
    vp, u64 = C.c_void_p, C.c_uint64
    L.zpk_codec_encode_batch_dsink_delta.argtypes = [vp, vp, C.c_int, vp, u64, vp, u64, vp, C.POINTER(u64), C.POINTER(u64), vp, vp]
    L.zpk_codec_decode_batch_dimage_delta.argtypes = [vp, vp, u64, vp, u64, vp, C.c_int, vp, vp, vp]
    L.zpk_codec_decode_batch_dimage_windows.argtypes = [vp, vp, u64, vp, u64, vp, C.c_int, vp, vp, vp, vp, vp]
    bound = codec.compress_bound(Z.METHOD_LZ4, SIZE)
    sink = torch.empty(n * bound + 64, dtype=torch.uint8, device=dev)
    ed = np.zeros(n, dtype=Z.ENCODE_DESC)
    ed["size"], ed["method"], ed["level"], ed["dst_capacity"] = SIZE, Z.METHOD_LZ4, 0, bound
    arr = lambda t, stride, off=0: (vp * n)(*[t.data_ptr() + i * stride + off for i in range(n)])
    sptr, bptr, optr = arr(src, SIZE), arr(base, SIZE), arr(out, SIZE)
    elem = (C.c_uint8 * n)(*([K] * n))
    torch.cuda.synchronize()

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    res = np.zeros(n, dtype=Z.ENCODE_RESULT)
    placed, nbytes = u64(0), u64(0)
    rc = L.zpk_codec_encode_batch_dsink_delta(codec.h, sptr, 1, ed.ctypes.data, n, sink.data_ptr(), sink.numel(), res.ctypes.data, C.byref(placed), C.byref(nbytes), elem, bptr)
    assert rc == 0 and placed.value == n and (res["status"] == 0).all()
    dd = np.zeros(n, dtype=Z.DECODE_DESC)
    dd["comp_size"] = res["comp_size"]
    dd["src_offset"] = np.concatenate([[0], np.cumsum(dd["comp_size"])[:-1]])
    dd["uncomp_size"] = dd["dst_capacity"] = SIZE
    dd["expect_hash"] = res["hash"]
    dd["method"] = Z.METHOD_LZ4
    image = sink[:nbytes.value + 1]                                                    # (a pad byte behind the payloads keeps the last entry inside)
    print("%d x 1 MiB bf16 as (512, 1024), delta entries (element size 2, base: the synthetic step at lr 1e-3), LZ4 level 0, compressed/plain %.3f; "
          "%d alternating rounds behind one warm-up round" % (n, nbytes.value / (n * SIZE), a.pairs))

    # ---- the two windows: 1/8 of every tensor ----
    r0, r1, c0, c1 = 64, 128, 128, 256
    windows = {
        "dim 0":    (Z.slice_window((ROWS, COLS), 0, r0, r1, K), lambda t: t.view(n, ROWS, COLS * K)[:, r0:r1, :]),
        "last dim": (Z.slice_window((ROWS, COLS), 1, c0, c1, K), lambda t: t.view(n, ROWS, COLS * K)[:, :, c0 * K:c1 * K]),
    }
    wbytes = SIZE // 8
    assert all(w[2] * w[4] == wbytes for w, _ in windows.values()) and windows["last dim"][0][4] == 256
    wout = torch.empty(n * wbytes, dtype=torch.uint8, device=dev)
    wptr = arr(wout, wbytes)
    shards = {name: cut(base).contiguous().view(-1) for name, (_, cut) in windows.items()}      # the caller's shard of the previous checkpoint
    want = {name: cut(src).contiguous().view(-1) for name, (_, cut) in windows.items()}
    wdd = dd.copy()
    wdd["dst_capacity"] = wbytes

    def read_windows(name):
        wins = np.array([windows[name][0]] * n, dtype=Z.WINDOW)
        r = np.zeros(n, dtype=Z.DECODE_RESULT)
        rc = L.zpk_codec_decode_batch_dimage_windows(codec.h, image.data_ptr(), image.numel(), wdd.ctypes.data, n, wptr, 1, r.ctypes.data, elem, arr(shards[name], wbytes), None,
                                                     wins.ctypes.data)
        assert rc == 0 and (r["status"] == 0).all()
        return wout

    def read_whole_then_slice(name):
        r = np.zeros(n, dtype=Z.DECODE_RESULT)
        rc = L.zpk_codec_decode_batch_dimage_delta(codec.h, image.data_ptr(), image.numel(), dd.ctypes.data, n, optr, 1, r.ctypes.data, elem, bptr)
        assert rc == 0 and (r["status"] == 0).all()
        return windows[name][1](out).contiguous().view(-1)

    legs = [(kind, name) for name in windows for kind in ("windows call", "whole read + slice")]
    times = {leg: [] for leg in legs}
    for rep in range(a.pairs + 1):
        for leg in legs:
            ms, got = clock(lambda: (read_windows if leg[0] == "windows call" else read_whole_then_slice)(leg[1]))
            if rep:
                times[leg].append(ms)
            else:
                assert torch.equal(got, want[leg[1]]), "%s, %s: not the slice of the tensors" % leg
            del got
    print("(a) out of a device image, a window of 1/8 of every tensor (every leg returned the slice of the tensors bit-exact):")
    for leg in legs:
        print("    %-8s  %-18s: %s" % (leg[1], leg[0], stat(times[leg])))
    for name in windows:
        w, s = statistics.median(times[("windows call", name)]), statistics.median(times[("whole read + slice", name)])
        print("    %-8s  the windows call takes %.3f of the whole read + slice (%.3f ms less); HBM for the destinations: %d MiB against %d + %d MiB" %
              (name, w / s, s - w, n * wbytes >> 20, n * SIZE >> 20, n * wbytes >> 20))

    # ---- (b) the kernels alone, on the stored bytes of the same entries ----
    stored = torch.empty(n * SIZE, dtype=torch.uint8, device=dev)
    srow = np.zeros(n, dtype=Z.DELTA_COPY)
    srow["src"], srow["dst"], srow["base"], srow["len"], srow["elem"], srow["join"] = list(sptr), list(arr(stored, SIZE)), list(bptr), SIZE, K, 0
    codec.delta_copy_device(srow)                                                      # stored = split(tensor ^ base)
    torch.cuda.synchronize()
    stptr = arr(stored, SIZE)
    prow = np.zeros(n, dtype=Z.PLANE_COPY)
    prow["src"], prow["dst"], prow["len"], prow["elem"], prow["join"] = list(stptr), list(optr), SIZE, K, 1
    drow = np.zeros(n, dtype=Z.DELTA_COPY)
    drow["src"], drow["dst"], drow["base"], drow["len"], drow["elem"], drow["join"] = list(stptr), list(optr), list(bptr), SIZE, K, 1
    wrows = {}
    for name, (w, _) in windows.items():
        for with_base in (False, True):
            t = np.zeros(n, dtype=Z.WINDOW_COPY)
            t["src"], t["dst"], t["n"], t["elem"] = list(stptr), list(wptr), SIZE, K
            t["base"] = list(arr(shards[name], wbytes)) if with_base else 0
            t["win"] = np.array([w] * n, dtype=Z.WINDOW)
            wrows["k_window_copy %s%s" % (name, ", base" if with_base else "")] = t
    kt = {"k_plane_copy join whole": [], "k_delta_copy join whole": []}
    kt.update({k: [] for k in wrows})
    for rep in range(a.pairs + 1):
        for name in kt:
            if name.startswith("k_plane"):
                ms, _ = clock(lambda: codec.plane_copy_device(prow))
                if rep == 0:
                    assert torch.equal(out, src ^ base)
            elif name.startswith("k_delta"):
                ms, _ = clock(lambda: codec.delta_copy_device(drow))
                if rep == 0:
                    assert torch.equal(out, src)
            else:
                ms, _ = clock(lambda: codec.window_copy_device(wrows[name]))
                if rep == 0:
                    wname = "dim 0" if "dim 0" in name else "last dim"
                    assert torch.equal(wout, want[wname] if name.endswith("base") else want[wname] ^ shards[wname]), name
            if rep:
                kt[name].append(ms)
    print("(b) the kernels alone (table upload + launch + kernel, %d rows; every kernel's bytes were checked):" % n)
    for name, xs in kt.items():
        moved = (2 if name.startswith("k_plane") else 3) * n * SIZE if "whole" in name else (3 if name.endswith("base") else 2) * n * wbytes
        print("    %-30s: %s   %7.1f GB/s over the %.2f GB it moves" % (name, stat(xs), moved / 1e9 / (statistics.median(xs) / 1e3), moved / 1e9))
    med = {k: statistics.median(v) for k, v in kt.items()}
    for name in wrows:
        whole = "k_delta_copy join whole" if name.endswith("base") else "k_plane_copy join whole"
        print("    %-30s / %s: %.3f  (1/8 of the bytes: 0.125 if time followed bytes alone)" % (name, whole, med[name] / med[whole]))
    codec.close()


if __name__ == "__main__":
    main()
