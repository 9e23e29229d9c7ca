#!/usr/bin/env python3
"""Developer: what testing an archive without bringing its plaintext home (include/zpack_amd.h: zpack_amd_test_files) saves against the
read a tester used before, which copied every decoded byte into a buffer nobody looked at.

  host side     a memory reader: zpack_read_files_packed into a host buffer (what `zpk-batch t` did)   against   zpack_amd_test_files
  device side   a reader over the image in device memory: zpack_amd_read_files_device_packed into a device buffer as large as the
                whole plaintext (what a caller of such an image had to allocate)                        against   zpack_amd_test_files

Behind one warm-up of each side: alternating pairs — the read first in the even pairs, the test first in the odd ones, so that what one
call leaves behind (a host cache full of plaintext, say) is not always the other's burden —, median and range per side, and whether the
new call is behind the read by more than the read's own run-to-run spread.  For the host side the expected gain is the download that
is left out: the plaintext bytes over the bus.

  tools/verify_rate.py [shape: lz4 | zstd | big] [pairs]
      lz4   20 000 x 64 KiB LZ4        zstd   8 000 x 256 KiB Zstandard-3        big   one entry of 256 MiB, LZ4"""
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

shape = sys.argv[1] if len(sys.argv) > 1 else "lz4"
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
n, size, method, level = {"lz4": (20000, 65536, dg.LZ4, 0), "zstd": (8000, 262144, dg.ZSTD, 3), "big": (1, 256 << 20, dg.LZ4, 0)}[shape]

Z = ZPackAPI(zpack_amd.ZPACK_SO)
PFE = C.POINTER(FileEntry)
R = C.POINTER(Reader)
Z.lib.zpack_read_files_packed.argtypes = [R, C.POINTER(PFE), C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.c_void_p]
Z.lib.zpack_amd_read_files_device_packed.argtypes = Z.lib.zpack_read_files_packed.argtypes
Z.lib.zpack_amd_test_files.argtypes = [R, C.POINTER(PFE), C.c_uint64, C.POINTER(C.c_int), C.c_void_p]
Z.lib.zpack_amd_init_reader_device.argtypes = [R, C.c_void_p, C.c_size_t]
dev = torch.device("cuda:0")

b = dg.Batch(n, size, size, method=method, level=level, seed=1)
total, comp = n * size, int(b.total_comp)
label = "%s: %d x %d bytes, method %d (ratio %.3f)" % (shape, n, size, method, comp / total)
image = torch.from_numpy(b.archive).to(dev)
torch.cuda.synchronize()
keep = (C.c_uint8 * b.archive.size).from_buffer(b.archive)
rm, rd = Reader(), Reader()
assert Z.lib.zpack_init_reader_memory_shared(C.byref(rm), C.cast(keep, u8p), b.archive.size) == 0
assert Z.lib.zpack_amd_init_reader_device(C.byref(rd), image.data_ptr(), image.numel()) == 0
assert rm.file_count == n and rd.file_count == n
res = (C.c_int * n)()
offs = (C.c_uint64 * n)()
ents = {id(r): (PFE * n)(*[C.pointer(r.file_entries[i]) for i in range(n)]) for r in (rm, rd)}
host_buf = np.empty(total, dtype=np.uint8)
stride = (size + 255) & ~255
dev_buf = torch.empty(n * stride, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()


def host_read():
    assert Z.lib.zpack_read_files_packed(C.byref(rm), ents[id(rm)], n, host_buf.ctypes.data, total, offs, res, None) == 0 and not any(res)


def device_read():
    assert Z.lib.zpack_amd_read_files_device_packed(C.byref(rd), ents[id(rd)], n, dev_buf.data_ptr(), dev_buf.numel(), offs, res, None) == 0 and not any(res)


def test(r):
    assert Z.lib.zpack_amd_test_files(C.byref(r), ents[id(r)], n, res, None) == 0 and not any(res)


for side, old, new, note in (("host", host_read, lambda: test(rm), "expected gain: %.1f MB of plaintext no longer downloaded (%.1f MB still go up)" % (total / 1e6, comp / 1e6)),
                             ("device", device_read, lambda: test(rd), "nothing crosses the bus either way; the new call needs no %.1f MB buffer" % (n * stride / 1e6))):
    old(); new()                                                                       # warm-up: contexts, staging, pinned buffers
    t_old, t_new = [], []
    for it in range(pairs):
        for which in ((0, 1) if it % 2 == 0 else (1, 0)):
            t0 = time.time(); (old, new)[which](); (t_old, t_new)[which].append(time.time() - t0)
        print("%s, %s side, pair %d: the read %.1f ms, the test %.1f ms" % (label, side, it, t_old[-1] * 1e3, t_new[-1] * 1e3), flush=True)
    for name, t in (("the read", t_old), ("the test", t_new)):
        print("%s, %s side, %s: median %.1f ms (%.1f .. %.1f) -> %.1f GiB/s of plaintext" % (label, side, name, statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3,
                                                                                          total / statistics.median(t) / 2**30), flush=True)
    spread = max(t_old) - min(t_old)
    gain = statistics.median(t_old) - statistics.median(t_new)
    print("%s, %s side: the test is %s by %.1f ms (%.2fx); the read's own spread is %.1f ms -> %s.  %s" % (
        label, side, "ahead" if gain > 0 else "BEHIND", abs(gain) * 1e3, statistics.median(t_old) / statistics.median(t_new), spread * 1e3,
        "SLOWER than the read by more than its spread" if -gain > spread else "not slower than the read", note), flush=True)
Z.close_reader(rd)
Z.close_reader(rm)
