#!/usr/bin/env python3
"""Developer: device-resident batches of large text entries, device to device — (a) zpk_codec_decode_big_batch_device (block headers walked
on the device by k_big_walk, one call), (b) a loop of zpk_codec_decode_big_device calls (each entry's compressed bytes copied to the host
for the walk), (c) zpk_codec_decode_batch_device (one wave per entry; the smallest entries only).  LZ4-0 and Zstandard-3, three shapes of
256 MiB in all; (a) and (b) take turns, `pairs` times behind one warm-up each; host time around call + synchronise.
usage: big_batch_device_rate.py [--pairs 3] [--shapes 1x256,16x16,64x4] [--once]     (--once: the new call alone, once per case, no
warm-up — for a kernel trace: one k_big_walk dispatch per case, in the order printed)
       big_batch_device_rate.py --stored [--pairs 3] [--shapes 1x256M,16x16M,64x4M,1024x256K] [--once]
STORED entries (bytes that do not compress) through zpk_codec_decode_big_batch_device: OPT_STORED_SPAN_MIN on (k_stored_span + the XXH3
chain across the chip) and off (one wave per entry) take turns, `pairs` times behind one warm-up each.  A library without the option
(ZPACK_AMD_CODEC_SO = an older build) is timed as it is, one series.
       big_batch_device_rate.py --stored-beside-lz4 [--pairs 3] [--mib 256]
one stored entry and one LZ4 text entry of that size in ONE call (what a second stream for the stored spans would overlap): one series;
run it with two builds of the library in turns."""
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
shapes = [tuple(int(x) for x in s.split("x")) for s in shapes.split(",")] if "--stored" not in args else []
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


def stored_batch(count, size, noise):
    """-> (src, dst, desc, hash): `count` stored entries of `size` bytes at every alignment, slots 256-aligned"""
    plain = np.ascontiguousarray(np.resize(noise, size))
    want = dg.xxh3(plain)
    stride = size + 7
    src = torch.zeros(10 + count * stride + 64, dtype=torch.uint8, device=dev)
    pd = torch.from_numpy(plain).to(dev)
    slot = (size + 255) & ~255
    dst = torch.zeros(count * slot + 256, dtype=torch.uint8, device=dev)
    d = np.zeros(count, dtype=zpack_amd.DECODE_DESC)
    for i in range(count):
        src[10 + i * stride:10 + i * stride + size] = pd
        d[i]["src_offset"] = 10 + i * stride; d[i]["dst_offset"] = i * slot
    d["comp_size"] = size; d["uncomp_size"] = size; d["expect_hash"] = want; d["dst_capacity"] = size; d["method"] = zpack_amd.METHOD_NONE
    return src, dst, d, want


def has_span_option():
    try:
        codec.set_option(zpack_amd.OPT_STORED_SPAN_MIN, 256 << 10)
        return True
    except RuntimeError:
        return False


if "--stored" in args:
    noise = np.concatenate([dg.fill(dg.RANDOM, 6, k, 1 << 20) for k in range(8)])
    unit = {"K": 1 << 10, "M": 1 << 20}
    sh = args[args.index("--shapes") + 1] if "--shapes" in args else "1x256M,16x16M,64x4M,1024x256K"
    sh = [(int(x.split("x")[0]), int(x.split("x")[1][:-1]) * unit[x[-1]], x) for x in sh.split(",")]
    opt = has_span_option()
    for count, size, label in sh:
        src, dst, d, want = stored_batch(count, size, noise)
        out = {}

        def call(on):
            if opt:
                codec.set_option(zpack_amd.OPT_STORED_SPAN_MIN, (1025 if on else 0))
            out["r"] = codec.decode_big_batch_device(src, d, dst)

        def check():
            assert (out["r"]["status"] == 0).all() and (out["r"]["hash"] == want).all(), out["r"]

        total = count * size / GIB
        head = "stored %-9s (%d x %d bytes), device to device:" % (label, count, size)
        if once:
            ms = timed(lambda: call(True)); check()
            st = codec.decode_stats()
            print("%s once %.2f ms; chip-wide %s, groups %s" % (head, ms, st.get("stored_span_entries"), st.get("stored_span_groups")), flush=True)
            continue
        call(True); call(False); check()
        ton, toff = [], []
        for _ in range(pairs):
            ton.append(timed(lambda: call(True))); check()
            st = codec.decode_stats()
            if opt:
                toff.append(timed(lambda: call(False))); check()
        if opt:
            print("%s on %s = %.2f GiB/s, chip-wide %d groups %d | off (one wave per entry) %s = %.2f GiB/s" % (
                head, span(ton), total / (statistics.median(ton) / 1e3), st["stored_span_entries"], st["stored_span_groups"],
                span(toff), total / (statistics.median(toff) / 1e3)), flush=True)
        else:
            print("%s library without the option %s = %.2f GiB/s" % (head, span(ton), total / (statistics.median(ton) / 1e3)), flush=True)
        del src, dst
    sys.exit(0)

if "--stored-beside-lz4" in args:
    mib = int(args[args.index("--mib") + 1]) if "--mib" in args else 256
    size = mib << 20
    noise = np.concatenate([dg.fill(dg.RANDOM, 6, k, 1 << 20) for k in range(8)])
    stored = np.ascontiguousarray(np.resize(noise, size))
    text = np.ascontiguousarray(np.resize(tile, size))
    frame = np.frombuffer(dg.compress(zpack_amd.METHOD_LZ4, 0, text), dtype=np.uint8)
    src = torch.zeros(10 + size + 7 + len(frame) + 64, dtype=torch.uint8, device=dev)
    src[10:10 + size] = torch.from_numpy(stored).to(dev)
    src[10 + size + 7:10 + size + 7 + len(frame)] = torch.from_numpy(np.array(frame)).to(dev)
    dst = torch.zeros(2 * size + 512, dtype=torch.uint8, device=dev)
    d = np.zeros(2, dtype=zpack_amd.DECODE_DESC)
    d[0]["src_offset"] = 10; d[0]["comp_size"] = size; d[0]["expect_hash"] = dg.xxh3(stored); d[0]["method"] = zpack_amd.METHOD_NONE
    d[1]["src_offset"] = 10 + size + 7; d[1]["comp_size"] = len(frame); d[1]["expect_hash"] = dg.xxh3(text); d[1]["method"] = zpack_amd.METHOD_LZ4; d[1]["dst_offset"] = size + 256
    d["uncomp_size"] = size; d["dst_capacity"] = size
    out = {}

    def both():
        out["r"] = codec.decode_big_batch_device(src, d, dst)

    both()
    ts = [timed(both) for _ in range(pairs)]
    st = codec.decode_stats()
    assert (out["r"]["status"] == 0).all() and (out["r"]["hash"] == d["expect_hash"]).all(), out["r"]
    print("stored %d MiB beside lz4-0 text %d MiB in one call (%s): %s; chip-wide %s, block-parallel %d" % (
        mib, mib, os.path.basename(os.path.dirname(zpack_amd.CODEC_SO)) + "/" + os.path.basename(zpack_amd.CODEC_SO), span(ts),
        st.get("stored_span_entries"), st["frame_parallel_entries"]), flush=True)
    sys.exit(0)


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
