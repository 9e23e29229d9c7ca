#!/usr/bin/env python3
"""Developer: ONE large text entry compressed from device memory into device memory — zpk_codec_encode_big_device (512 KiB pieces side
by side, the frame assembled on the device) against zpk_codec_encode_batch_device (one wave, the smaller entry only: it takes seconds).
LZ4-0 and Zstandard-1; median of five runs behind a warm-up, host time around enqueue + synchronise; the gather's own time from the
codec's event pair around k_big_gather (ZPK_K_PACK).  A library without the new call (ZPACK_AMD_CODEC_SO = a build of an older commit)
runs the one-wave leg alone.
usage: big_encode_device_rate.py [MiB ...=64 256] [--one-wave-mib 64] [--once]      (--once: one run of the new call per case, no
one-wave leg — for a kernel trace)"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zpack_amd
from benchdata import datagen as dg

args = sys.argv[1:]
once = "--once" in args
one_wave_mib = 64
if "--one-wave-mib" in args:
    one_wave_mib = int(args[args.index("--one-wave-mib") + 1])
    del args[args.index("--one-wave-mib"):args.index("--one-wave-mib") + 2]
sizes = [int(a) for a in args if not a.startswith("--")] or [64, 256]
codec = zpack_amd.Codec(0)
have_big = hasattr(codec.L, "zpk_codec_encode_big_device")
dev = torch.device("cuda:0")
GIB = float(1 << 30)


def median_ms(fn, runs=5):
    fn()                                                                         # warm-up: the codec's staging grows here
    ts = []
    for _ in range(1 if once else runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


for mib in sizes:
    size = mib << 20
    tile = np.concatenate([dg.fill(dg.TEXT, 5, k, 1 << 20) for k in range(8)])      # 8 MiB of text, repeated
    plain = np.ascontiguousarray(np.resize(tile, size))
    want = dg.xxh3(plain)
    src = torch.zeros(size + 64, dtype=torch.uint8, device=dev)
    src[:size] = torch.from_numpy(plain).to(dev)
    for method, level, name in [(zpack_amd.METHOD_LZ4, 0, "lz4-0"), (zpack_amd.METHOD_ZSTD, 1, "zstd-1")]:
        bound = codec.compress_bound(method, size)
        dst = torch.zeros(bound + 64, dtype=torch.uint8, device=dev)
        res = torch.zeros(zpack_amd.ENCODE_RESULT.itemsize, dtype=torch.uint8, device=dev)
        desc = np.zeros(1, dtype=zpack_amd.ENCODE_DESC)
        desc["size"] = size; desc["dst_capacity"] = bound; desc["method"] = method; desc["level"] = level
        line = "%-6s %4d MiB text, device to device:" % (name, mib)
        if have_big:
            codec.set_option(zpack_amd.OPT_ENC_SPLIT_MIN, 2 << 20)
            codec.set_profiling(True)
            ms = median_ms(lambda: codec.encode_big_device(src, desc, dst, res))
            r = res.cpu().numpy().view(zpack_amd.ENCODE_RESULT)[0]
            assert int(r["status"]) == 0 and int(r["hash"]) == want, r
            gms = codec.kernel_ms(zpack_amd.K_PACK)
            cs = int(r["comp_size"])
            codec.set_profiling(False)
            st = codec.encode_stats()
            line += " in %d pieces %.1f ms = %.2f GiB/s, ratio %.4f; k_big_gather %.3f ms = %.0f GiB/s read + written" % (
                st["pieces"], ms, size / GIB / (ms / 1e3), cs / size, gms, 2 * cs / GIB / (gms / 1e3))
        if mib <= one_wave_mib and not once:
            ddesc = torch.from_numpy(desc.view(np.uint8)).to(dev)
            ms1 = median_ms(lambda: codec.encode_batch_device(src, ddesc, 1, dst, res), runs=3)
            r = res.cpu().numpy().view(zpack_amd.ENCODE_RESULT)[0]
            assert int(r["status"]) == 0 and int(r["hash"]) == want, r
            line += " | one wave (zpk_codec_encode_batch_device): %.0f ms = %.3f GiB/s, ratio %.4f" % (ms1, size / GIB / (ms1 / 1e3), int(r["comp_size"]) / size)
        print(line, flush=True)
        del dst
    del src
