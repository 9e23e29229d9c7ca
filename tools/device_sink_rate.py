#!/usr/bin/env python3
"""Developer: what a writer whose sink is an archive image in DEVICE memory (include/zpack_amd.h: zpack_amd_init_writer_device) saves a
caller whose plaintext lies in device memory and who wants the archive there too.

  today's way   zpack_amd_write_files_device into a HEAP writer (the compressed bytes come home and are copied into the heap image),
                then the upload of the heap image: the compressed bytes cross the bus twice
  device sink   the same calls on a writer over a device tensor of archive_capacity bytes: results and the cut come home, no compressed byte

Both sides write header, data signature, files, CDR and EOCDR from the same tensors with one shared context (a caller that writes more
than once keeps one).  Behind one warm-up of each side: seven alternating pairs per shape, median and range per side, and whether the
device sink is behind today's way by more than the pairs' own spread.  Then one more device-sink call with the codec's kernel timing on:
k_sink_place's own time and rate.

  tools/device_sink_rate.py [shape ...]      shapes: lz4_64k (20000 x 64 KiB LZ4), zstd_256k (8000 x 256 KiB Zstandard-1),
                                             lz4_256m, zstd_256m (one entry of 256 MiB); default: all four
  tools/device_sink_rate.py --pairs N ...    N pairs instead of seven"""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import zpack_amd
from benchdata import datagen as dg
from zpack_amd import device_io
from tests._libs import ZPackAPI, Writer, File, CompressOptions, u8p

SHAPES = {"lz4_64k": (20000, 64 << 10, dg.LZ4, 0), "zstd_256k": (8000, 256 << 10, dg.ZSTD, 1),
          "lz4_256m": (1, 256 << 20, dg.LZ4, 0), "zstd_256m": (1, 256 << 20, dg.ZSTD, 1)}
args = sys.argv[1:]
npairs = 7
if args and args[0] == "--pairs":
    npairs = int(args[1]); args = args[2:]
shapes = args or list(SHAPES)

Z = ZPackAPI(zpack_amd.ZPACK_SO)
W = C.POINTER(Writer)
Z.lib.zpack_amd_init_writer_device.argtypes = [W, C.c_void_p, C.c_size_t]
Z.lib.zpack_amd_write_files_device.argtypes = [W, C.POINTER(File), C.c_uint64]
Z.lib.zpack_create_cctx.restype = C.c_void_p
Z.lib.zpack_create_cctx.argtypes = [C.c_int]
Z.lib.zpack_free_cctx.restype = None
Z.lib.zpack_free_cctx.argtypes = [C.c_int, C.c_void_p]
L = zpack_amd.lib()
dev = torch.device("cuda:0")


def run(shape):
    n, size, method, level = SHAPES[shape]
    label = "write %d x %d bytes, method %d level %d" % (n, size, method, level)
    rng = np.random.default_rng(5)
    k = min(n, 64)
    classes = rng.choice(4, size=k, p=[0.70, 0.20, 0.05, 0.05]) if n > 1 else [dg.TEXT]
    pool = [np.ascontiguousarray(dg.fill(int(classes[i]), 5, i, size)) for i in range(k)]
    src = torch.from_numpy(np.concatenate([pool[i % k] for i in range(n)])).to(dev)    # the caller's tensors: n entries in device memory
    del pool
    torch.cuda.synchronize()
    total = n * size
    cctx = Z.lib.zpack_create_cctx(method)
    assert cctx
    opts = CompressOptions(method, level)
    names = [("f%06d" % i).encode() for i in range(n)]
    arr = (File * n)()
    for i in range(n):
        arr[i].filename = names[i]; arr[i].buffer = C.cast(src.data_ptr() + i * size, u8p); arr[i].size = size; arr[i].options = C.pointer(opts); arr[i].cctx = cctx
    capacity = device_io.archive_capacity([size] * n, [nm.decode() for nm in names], method)
    out = {}

    def archive(w):
        assert Z.lib.zpack_write_header(w) == 0 and Z.lib.zpack_write_data_header(w) == 0
        rc = Z.lib.zpack_amd_write_files_device(w, arr, n)
        assert rc == 0, rc
        assert Z.lib.zpack_write_cdr(w) == 0 and Z.lib.zpack_write_eocdr(w) == 0

    def old():
        w = Writer()
        assert Z.lib.zpack_init_writer_heap(C.byref(w), 0) == 0
        archive(C.byref(w))
        heap = np.ctypeslib.as_array(C.cast(w.buffer, C.POINTER(C.c_uint8)), shape=(int(w.file_size),))
        image = torch.from_numpy(heap).to(dev)                                         # the upload a caller makes today
        torch.cuda.synchronize()
        Z.lib.zpack_close_writer(C.byref(w))
        out["old"] = image

    def new():
        image = torch.empty(capacity, dtype=torch.uint8, device=dev)
        w = Writer()
        assert Z.lib.zpack_amd_init_writer_device(C.byref(w), image.data_ptr(), capacity) == 0
        archive(C.byref(w))
        out["new"] = image[:int(w.file_size)]
        Z.lib.zpack_close_writer(C.byref(w))

    old(); new()                                                                       # warm-up: the context, its staging, pinned buffers, the allocator
    t_old, t_new = [], []
    for it in range(npairs):
        t0 = time.time(); old(); t_old.append(time.time() - t0)
        t0 = time.time(); new(); t_new.append(time.time() - t0)
        print("%s pair %d: today's way %.1f ms, device sink %.1f ms" % (label, it, t_old[-1] * 1e3, t_new[-1] * 1e3), flush=True)
    for name, t in (("today's way", t_old), ("device sink", t_new)):
        print("%s %s: median %.1f ms (%.1f .. %.1f) -> %.2f GiB/s of plaintext" % (label, name, statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3,
                                                                                     total / statistics.median(t) / 2**30), flush=True)
    spread = max(max(t_old) - min(t_old), max(t_new) - min(t_new))
    gain = statistics.median(t_old) - statistics.median(t_new)
    verdict = "ahead by more than the spread" if gain > spread else ("within the spread" if abs(gain) <= spread else "BEHIND by more than the spread")
    print("%s: the device sink is %s by %.1f ms; the pairs' spread is %.1f ms -> %s" % (label, "ahead" if gain > 0 else "behind", abs(gain) * 1e3, spread * 1e3, verdict), flush=True)
    same = bool(torch.equal(out["old"], out["new"]))
    print("%s: same archive both ways: %s (%.3f GB)" % (label, same, out["new"].numel() / 1e6 / 1e3), flush=True)
    assert same
    # k_sink_place alone: the context's first codec (zi_ctx: a count, then the codecs) with kernel timing on, one more device-sink call
    codec = C.cast(cctx, C.POINTER(C.c_void_p))[1]
    L.zpk_codec_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.zpk_codec_kernel_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
    assert L.zpk_codec_set_profiling(codec, 1) == 0
    new()
    ms = C.c_float(0)
    assert L.zpk_codec_kernel_ms(codec, zpack_amd.K_PACK, C.byref(ms)) == 0
    L.zpk_codec_set_profiling(codec, 0)
    payload = out["new"].numel() - 10 - 20 - sum(35 + len(nm) for nm in names) - 12
    print("%s: k_sink_place %.3f ms for %.1f MB of payloads -> %.2f TB/s copied" % (label, ms.value, payload / 1e6, payload / (ms.value * 1e-3) / 1e12 if ms.value > 0 else 0.0), flush=True)
    out.clear()
    Z.lib.zpack_free_cctx(method, cctx)
    del src
    torch.cuda.empty_cache()


for s in shapes:
    run(s)
