#!/usr/bin/env python3
"""Developer: device-resident batches of large text entries, device to device — (a) zpk_codec_decode_big_batch_device (block headers walked
on the device by k_big_walk, one call), (b) a loop of zpk_codec_decode_big_device calls (each entry's compressed bytes copied to the host
for the walk), (c) zpk_codec_decode_batch_device (one wave per entry; the smallest entries only).  LZ4-0 and Zstandard-3, three shapes of
256 MiB in all; (a) and (b) take turns, `pairs` times behind one warm-up each; host time around call + synchronise.
usage: big_batch_device_rate.py [--pairs 3] [--shapes 1x256,16x16,64x4] [--once]     (--once: the new call alone, once per case, no
warm-up — for a kernel trace: one k_big_walk dispatch per case, in the order printed)"""
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
pairs = int(args[args.index("--pairs") + 1]) if "--pairs" in args else 3
shapes = args[args.index("--shapes") + 1] if "--shapes" in args else "1x256,16x16,64x4"
shapes = [tuple(int(x) for x in s.split("x")) for s in shapes.split(",")]
codec = zpack_amd.Codec(0)
dev = torch.device("cuda:0")
GIB = float(1 << 30)
tile = np.concatenate([dg.fill(dg.TEXT, 5, k, 1 << 20) for k in range(8)])          # 8 MiB of text, repeated


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def span(ts):
    return "median %.2f ms (%.2f .. %.2f)" % (statistics.median(ts), min(ts), max(ts))


for count, mib in shapes:
    size = mib << 20
    plain = np.ascontiguousarray(np.resize(tile, size))
    want = dg.xxh3(plain)
    for method, level, name in [(zpack_amd.METHOD_LZ4, 0, "lz4-0"), (zpack_amd.METHOD_ZSTD, 3, "zstd-3")]:
        frame = np.frombuffer(dg.compress(method, level, plain), dtype=np.uint8)
        cs = len(frame)
        stride = cs + 7                                                                # (entries at every alignment)
        src = torch.zeros(10 + count * stride + 64, dtype=torch.uint8, device=dev)
        fd = torch.from_numpy(np.array(frame)).to(dev)
        slot = (size + 255) & ~255
        dst = torch.zeros(count * slot + 256, dtype=torch.uint8, device=dev)
        d = np.zeros(count, dtype=zpack_amd.DECODE_DESC)
        for i in range(count):
            src[10 + i * stride:10 + i * stride + cs] = fd
            d[i]["src_offset"] = 10 + i * stride; d[i]["dst_offset"] = i * slot
        d["comp_size"] = cs; d["uncomp_size"] = size; d["expect_hash"] = want; d["dst_capacity"] = size; d["method"] = method
        out = {}

        def new_call():
            out["a"] = codec.decode_big_batch_device(src, d, dst)

        def loop_call():
            out["b"] = [codec.decode_big_device(src, d[i:i + 1], dst) for i in range(count)]

        head = "%-6s %3d x %3d MiB text (ratio %.3f), device to device:" % (name, count, mib, cs / size)
        if once:
            ms = timed(new_call)
            st = codec.decode_stats()
            assert (out["a"]["status"] == 0).all() and (out["a"]["hash"] == want).all(), out["a"]
            print("%s new call once %.2f ms; walked %d, accepted %d, block-parallel %d" % (head, ms, st["device_walked"], st["device_walk_accepted"], st["frame_parallel_entries"]), flush=True)
            continue
        new_call(); loop_call()                                                        # warm-up: the codec's staging grows here
        ta, tb = [], []
        for _ in range(pairs):
            ta.append(timed(new_call))
            st = codec.decode_stats()
            tb.append(timed(loop_call))
        assert (out["a"]["status"] == 0).all() and (out["a"]["hash"] == want).all(), out["a"]
        assert all(int(r["status"]) == 0 and int(r["hash"]) == want for r in out["b"])
        total = count * size / GIB
        line = "%s (a) decode_big_batch_device %s = %.2f GiB/s, walked %d accepted %d block-parallel %d | (b) %d x decode_big_device %s = %.2f GiB/s" % (
            head, span(ta), total / (statistics.median(ta) / 1e3), st["device_walked"], st["device_walk_accepted"], st["frame_parallel_entries"],
            count, span(tb), total / (statistics.median(tb) / 1e3))
        if (count, mib) == min(shapes, key=lambda s: s[1]):
            ddesc = torch.from_numpy(d.view(np.uint8)).to(dev)
            dres = torch.zeros(count * zpack_amd.DECODE_RESULT.itemsize, dtype=torch.uint8, device=dev)
            tc = [timed(lambda: codec.decode_batch_device(src, ddesc, count, dst, dres)) for _ in range(1 + pairs)][1:]
            r = dres.cpu().numpy().view(zpack_amd.DECODE_RESULT)
            assert (r["status"] == 0).all() and (r["hash"] == want).all(), r
            line += " | (c) decode_batch_device, one wave each %s = %.2f GiB/s" % (span(tc), total / (statistics.median(tc) / 1e3))
        print(line, flush=True)
        del src, dst, fd
