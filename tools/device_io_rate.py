#!/usr/bin/env python3
"""Developer: what the device-memory calls of libzpack_amd.so (include/zpack_amd.h) save a caller whose plaintext lives in device memory.

  reads   zpack_amd_read_files_device                 against   zpack_read_files, then the H2D copy of the outputs
  writes  zpack_amd_write_files_device                against   the D2H copy of the sources, then zpack_write_files

The shapes of tools/host_rate.py (entries of 64 KiB LZ4 / 256 KiB Zstandard-3) and tools/host_write_rate.py (1 MiB sources).  Behind one
warm-up of each side: three alternating pairs, median and range per side.

  tools/device_io_rate.py read  [entries] [method: 2 lz4 | 1 zstd]
  tools/device_io_rate.py write [entries] [entry_bytes] [method: 1 zstd | 2 lz4] [level]
  tools/device_io_rate.py read-device-only / write-device-only ...     the new call alone, three times (for a kernel trace)"""
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
from tests._libs import ZPackAPI, FileEntry, Reader, Writer, File, CompressOptions, u8p

mode = sys.argv[1] if len(sys.argv) > 1 else "read"
args = sys.argv[2:]
only_device = mode.endswith("-device-only")
Z = ZPackAPI(zpack_amd.ZPACK_SO)
PFE = C.POINTER(FileEntry)
Z.lib.zpack_read_files.argtypes = [C.POINTER(Reader), C.POINTER(PFE), C.c_uint64, C.POINTER(u8p), C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.c_void_p]
Z.lib.zpack_amd_read_files_device.argtypes = [C.POINTER(Reader), C.POINTER(PFE), C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.c_void_p]
Z.lib.zpack_amd_write_files_device.argtypes = [C.POINTER(Writer), C.POINTER(File), C.c_uint64]
dev = torch.device("cuda:0")


def pairs(label, total_bytes, old, new):
    """old / new: callables that do the whole job and return when the bytes are where they belong"""
    if only_device:
        for it in range(3):
            t0 = time.time(); new(); dt = time.time() - t0
            print("%s, the device call alone, pass %d: %.1f ms -> %.1f GiB/s" % (label, it, dt * 1e3, total_bytes / dt / 2**30), flush=True)
        return
    old(); new()                                                                      # warm-up: contexts, staging, pinned buffers
    t_old, t_new = [], []
    for it in range(3):
        t0 = time.time(); old(); t_old.append(time.time() - t0)
        t0 = time.time(); new(); t_new.append(time.time() - t0)
        print("%s pair %d: today's way %.1f ms, device call %.1f ms" % (label, it, t_old[-1] * 1e3, t_new[-1] * 1e3), flush=True)
    for name, t in (("today's way", t_old), ("device call", t_new)):
        print("%s %s: median %.1f ms (%.1f .. %.1f) -> %.1f GiB/s" % (label, name, statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3,
                                                                        total_bytes / statistics.median(t) / 2**30), flush=True)
    spread = max(max(t_old) - min(t_old), max(t_new) - min(t_new))
    gain = statistics.median(t_old) - statistics.median(t_new)
    print("%s: the device call is %s by %.1f ms; the pairs' spread is %.1f ms -> %s" % (label, "ahead" if gain > 0 else "BEHIND", abs(gain) * 1e3, spread * 1e3,
                                                                                          "ahead by more than the spread" if gain > spread else "NOT ahead by more than the spread"), flush=True)


if mode.startswith("read"):
    n = int(args[0]) if len(args) > 0 else 20000
    method = int(args[1]) if len(args) > 1 else dg.LZ4
    size = 65536 if method == dg.LZ4 else 262144
    b = dg.Batch(n, size, size, method=method, level=0 if method == dg.LZ4 else 3, seed=1)
    rc, r, keep = Z.open_memory(b.archive.tobytes())
    assert rc == 0 and r.file_count == n
    ents = (PFE * n)(*[C.pointer(r.file_entries[i]) for i in range(n)])
    caps = (C.c_size_t * n)(*([size] * n))
    res = (C.c_int * n)()
    total = n * size
    host = np.empty(total, dtype=np.uint8)
    hptrs = (u8p * n)(*[C.cast(host.ctypes.data + i * size, u8p) for i in range(n)])
    up = torch.empty(total, dtype=torch.uint8, device=dev)                             # where today's caller uploads to
    direct = torch.empty(total, dtype=torch.uint8, device=dev)                         # where the device call decodes to
    dptrs = (C.c_void_p * n)(*[direct.data_ptr() + i * size for i in range(n)])
    torch.cuda.synchronize()

    def old():
        assert Z.lib.zpack_read_files(C.byref(r), ents, n, hptrs, caps, res, None) == 0 and not any(res)
        up.copy_(torch.from_numpy(host)); torch.cuda.synchronize()

    def new():
        assert Z.lib.zpack_amd_read_files_device(C.byref(r), ents, n, dptrs, caps, res, None) == 0 and not any(res)

    pairs("read %d x %d bytes, method %d" % (n, size, method), total, old, new)
    if not only_device:
        print("same bytes both ways:", bool(torch.equal(up, direct)))
    Z.close_reader(r)
else:
    n = int(args[0]) if len(args) > 0 else 4000
    size = int(args[1]) if len(args) > 1 else 1 << 20
    method = int(args[2]) if len(args) > 2 else 1
    level = int(args[3]) if len(args) > 3 else 1
    rng = np.random.default_rng(5)
    classes = rng.choice(4, size=64, p=[0.70, 0.20, 0.05, 0.05])
    pool = [np.ascontiguousarray(dg.fill(int(classes[i]), 5, i, size)) for i in range(64)]
    src = torch.from_numpy(np.concatenate([pool[i % 64] for i in range(n)])).to(dev)   # the caller's tensors: n entries in device memory
    torch.cuda.synchronize()
    opts = CompressOptions(method, level)
    names = [("f%06d" % i).encode() for i in range(n)]
    out = {}

    def write(base_addr, call, tag):
        w = Writer()
        assert Z.lib.zpack_init_writer_heap(C.byref(w), 0) == 0
        arr = (File * n)()
        for i in range(n):
            arr[i].filename = names[i]; arr[i].buffer = C.cast(base_addr + i * size, u8p); arr[i].size = size; arr[i].options = C.pointer(opts)
        assert Z.lib.zpack_write_header(C.byref(w)) == 0 and Z.lib.zpack_write_data_header(C.byref(w)) == 0
        rc = call(C.byref(w), arr, n)
        assert rc == 0, rc
        out[tag] = (int(w.write_offset), C.string_at(w.buffer, min(int(w.file_size), 1 << 20)))
        Z.lib.zpack_close_writer(C.byref(w))

    def old():
        home = src.cpu().numpy()                                                       # the D2H copy a caller makes today
        write(home.ctypes.data, Z.lib.zpack_write_files, "old")

    def new():
        write(src.data_ptr(), Z.lib.zpack_amd_write_files_device, "new")

    pairs("write %d x %d bytes, method %d level %d" % (n, size, method, level), n * size, old, new)
    if not only_device:
        print("same archive both ways (size, first MiB):", out["old"] == out["new"], "compressed to %.2f GB" % (out["new"][0] / 1e9))
