"""What the GPU tests of the device-memory paths share (test_gpu_device_io.py, test_gpu_device_image.py, test_gpu_device_sink.py): the
`torch` and `Z` fixtures, the plaintexts and archives they read and write, and the layout of device destinations between canaries.
A plain module: the test files import what they use."""
import ctypes as C

import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests import zpk
from tests._libs import ZPackAPI, Reader, Writer, File, FileEntry

CANARY = 0xA5
GAP = 64
PFE = C.POINTER(FileEntry)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def Z():
    """libzpack_amd.so with the prototypes of the three files together.  Arrays of buffers go as c_void_p: one file hands arrays of
    POINTER(c_uint8), another arrays of c_void_p, to the same calls."""
    z = ZPackAPI(zpack_amd.ZPACK_SO)
    L = z.lib
    R, W, vp, u64 = C.POINTER(Reader), C.POINTER(Writer), C.c_void_p, C.c_uint64
    L.zpack_amd_init_reader_device.argtypes = [R, vp, C.c_size_t]
    L.zpack_amd_reader_device_image.argtypes = [R, C.POINTER(vp), C.POINTER(C.c_int)]
    L.zpack_read_file.argtypes = [R, PFE, vp, C.c_size_t, vp]
    L.zpack_read_files.argtypes = [R, C.POINTER(PFE), u64, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_int), vp]
    L.zpack_amd_read_files_device.argtypes = L.zpack_read_files.argtypes
    L.zpack_read_files_packed.argtypes = [R, C.POINTER(PFE), u64, vp, C.c_size_t, C.POINTER(u64), C.POINTER(C.c_int), vp]
    L.zpack_amd_read_files_device_packed.argtypes = L.zpack_read_files_packed.argtypes
    L.zpack_read_raw_file.argtypes = [R, PFE, vp, C.c_size_t]
    L.zpack_read_archive_memory.argtypes = [R]
    L.zpack_read_archive.argtypes = [R]
    L.zpack_amd_read_ahead_stats.argtypes = [R, vp, C.POINTER(u64)]
    L.zpack_create_dctx.restype = vp
    L.zpack_create_dctx.argtypes = [C.c_int]
    L.zpack_free_dctx.restype = None
    L.zpack_free_dctx.argtypes = [C.c_int, vp]
    L.zpack_amd_init_writer_device.argtypes = [W, vp, C.c_size_t]
    L.zpack_amd_writer_device_image.argtypes = [W, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    L.zpack_amd_write_files_device.argtypes = [W, C.POINTER(File), u64]
    L.zpack_write_files_from_archive.argtypes = [W, R, PFE, u64]
    return z


def _layout(caps, mis):
    """device destinations back to back in one buffer, at least GAP canary bytes around each; destination i at an address = mis[i % len] mod 16"""
    pos, offs = GAP, []
    for i, c in enumerate(caps):
        pos = ((pos + 15) & ~15) + mis[i % len(mis)]
        offs.append(pos)
        pos += c + GAP
    return offs, pos + GAP


def _plain(i, n):
    """n bytes, three kinds: text with edits (matches at many distances), random bytes, long runs"""
    rng = np.random.default_rng(1000 + i)
    if n == 0:
        return b""
    if i % 3 == 0:
        words = [b"alpha ", b"beta ", b"gamma delta ", b"epsilon\n", b"0123456789", b"the quick brown fox "]
        out = bytearray()
        while len(out) < n:
            out += words[int(rng.integers(len(words)))]
            if rng.integers(8) == 0:
                out += bytes(rng.integers(0, 256, 3, dtype=np.uint8))
        return bytes(out[:n])
    if i % 3 == 1:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    unit = bytes([i & 255]) * 700 + b"ab" * 150 + rng.integers(0, 256, 40, dtype=np.uint8).tobytes()
    return (unit * (n // len(unit) + 1))[:n]


def _build(specs):
    """specs: [(method, level, plaintext)] -> archive bytes, plaintexts"""
    payloads, entries, pos = [], [], 10
    for i, (m, lv, data) in enumerate(specs):
        p = dg.compress(m, lv, data)
        payloads.append(p)
        entries.append(("e%04d" % i, pos, len(p), len(data), dg.xxh3(data), m))
        pos += len(p)
    return zpk.assemble(payloads, entries)
