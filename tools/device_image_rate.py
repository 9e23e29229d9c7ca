#!/usr/bin/env python3
"""Developer: what a reader over an archive image in DEVICE memory (include/zpack_amd.h: zpack_amd_init_reader_device) saves a caller whose
archive already lies there, reading into device memory.

  today's way   a memory reader over a host copy of the image, zpack_amd_read_files_device: the compressed bytes cross the bus again
  device image  a reader over the image where it lies, the same call: nothing crosses the bus but tables

The shapes of tools/device_io_rate.py (entries of 64 KiB LZ4 / 256 KiB Zstandard-3).  Behind one warm-up of each side: three alternating
pairs, median and range per side.  The copy of the image to the host and the opening of the memory reader, which today's caller pays once
per archive, are timed on their own and are not part of the pairs.

  tools/device_image_rate.py [entries] [method: 2 lz4 | 1 zstd]
  tools/device_image_rate.py device-only [entries] [method]       the new reader's call alone, three times (for a kernel trace)"""
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
from tests._libs import ZPackAPI, FileEntry, Reader, u8p

args = sys.argv[1:]
only_device = bool(args) and args[0] == "device-only"
if only_device:
    args = args[1:]
n = int(args[0]) if len(args) > 0 else 20000
method = int(args[1]) if len(args) > 1 else dg.LZ4
size = 65536 if method == dg.LZ4 else 262144

Z = ZPackAPI(zpack_amd.ZPACK_SO)
PFE = C.POINTER(FileEntry)
Z.lib.zpack_amd_read_files_device.argtypes = [C.POINTER(Reader), C.POINTER(PFE), C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.c_void_p]
Z.lib.zpack_amd_init_reader_device.argtypes = [C.POINTER(Reader), C.c_void_p, C.c_size_t]
dev = torch.device("cuda:0")

b = dg.Batch(n, size, size, method=method, level=0 if method == dg.LZ4 else 3, seed=1)
image = torch.from_numpy(b.archive).to(dev)                                            # where the caller's archive lies
torch.cuda.synchronize()
label = "read %d x %d bytes, method %d" % (n, size, method)
total = n * size

t0 = time.time()
home = image.cpu().numpy()                                                             # today: the image comes home ...
keep = (C.c_uint8 * home.size).from_buffer(home)
rm = Reader()
assert Z.lib.zpack_init_reader_memory_shared(C.byref(rm), C.cast(keep, u8p), home.size) == 0      # ... and a memory reader is opened over it
t_home = time.time() - t0
t0 = time.time()
rd = Reader()
assert Z.lib.zpack_amd_init_reader_device(C.byref(rd), image.data_ptr(), image.numel()) == 0
t_open = time.time() - t0
assert rm.file_count == n and rd.file_count == n
print("%s, once per archive: the image (%.1f MB) home and a memory reader opened %.1f ms; the device reader opened %.1f ms"
      % (label, image.numel() / 1e6, t_home * 1e3, t_open * 1e3), flush=True)

caps = (C.c_size_t * n)(*([size] * n))
res = (C.c_int * n)()
out = {}
for tag, r in (("old", rm), ("new", rd)):
    t = torch.empty(total, dtype=torch.uint8, device=dev)
    out[tag] = (r, (PFE * n)(*[C.pointer(r.file_entries[i]) for i in range(n)]), t, (C.c_void_p * n)(*[t.data_ptr() + i * size for i in range(n)]))
torch.cuda.synchronize()


def read(tag):
    r, ents, t, ptrs = out[tag]
    assert Z.lib.zpack_amd_read_files_device(C.byref(r), ents, n, ptrs, caps, res, None) == 0 and not any(res)


if only_device:
    for it in range(3):
        t0 = time.time(); read("new"); dt = time.time() - t0
        print("%s, the device reader alone, pass %d: %.1f ms -> %.1f GiB/s" % (label, it, dt * 1e3, total / dt / 2**30), flush=True)
else:
    read("old"); read("new")                                                           # warm-up: contexts, staging, pinned buffers
    t_old, t_new = [], []
    for it in range(3):
        t0 = time.time(); read("old"); t_old.append(time.time() - t0)
        t0 = time.time(); read("new"); t_new.append(time.time() - t0)
        print("%s pair %d: today's way %.1f ms, device image %.1f ms" % (label, it, t_old[-1] * 1e3, t_new[-1] * 1e3), flush=True)
    for name, t in (("today's way", t_old), ("device image", t_new)):
        print("%s %s: median %.1f ms (%.1f .. %.1f) -> %.1f GiB/s" % (label, name, statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3,
                                                                        total / statistics.median(t) / 2**30), flush=True)
    spread = max(max(t_old) - min(t_old), max(t_new) - min(t_new))
    gain = statistics.median(t_old) - statistics.median(t_new)
    print("%s: the device image is %s by %.1f ms; the pairs' spread is %.1f ms -> %s" % (label, "ahead" if gain > 0 else "BEHIND", abs(gain) * 1e3, spread * 1e3,
                                                                                           "ahead by more than the spread" if gain > spread else "NOT ahead by more than the spread"), flush=True)
    print("same bytes both ways:", bool(torch.equal(out["old"][2], out["new"][2])))
Z.close_reader(rd)
Z.close_reader(rm)
