"""Window reads without a GPU: the window, its rule, the row table of k_window_copy and what an item covers
(zpack_amd/csrc/window_copy_plan.h) under ASan + UBSan — the items tile the window once, every source index lies inside the entry, no
stored byte is read twice, the window whole is the join, a read in place reads no base byte another item writes —, the slice-to-window
formula against numpy slicing, the new symbols of both libraries, and what the library call answers before it needs a device."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import zpack_amd
from tests._libs import ZPackAPI, Reader, FileEntry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tools", "hostfuzz", "run_window_copy_plan.sh")
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
STREAM_INVALID, NOT_AVAILABLE = 21, 24


class Window(C.Structure):
    _fields_ = [("row_bytes", C.c_uint64), ("row0", C.c_uint64), ("rows", C.c_uint64), ("col0", C.c_uint64), ("cols", C.c_uint64)]


@pytest.fixture(scope="module")
def L():
    lib = ZPackAPI(zpack_amd.ZPACK_SO).lib
    lib.zpack_amd_read_files_device_windows.argtypes = [C.POINTER(Reader), C.POINTER(C.POINTER(FileEntry)), C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                        C.POINTER(C.c_uint8), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(Window), C.POINTER(C.c_int), C.c_void_p]
    return lib


def _no_device():
    lib = zpack_amd.lib()
    lib.zpk_codec_device_count.restype = C.c_int
    return lib.zpk_codec_device_count() <= 0


def _reader(L):
    r = Reader()
    path = os.path.join(ROOT, "tests", "golden", "ref_workdir", "archive_lz4.zpk")
    assert L.zpack_init_reader(C.byref(r), path.encode()) == 0
    assert r.file_count == 2
    return r


@needs_gxx
def test_window_copy_plan_under_asan_ubsan():
    p = subprocess.run(["bash", SCRIPT], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    for line in ("rule: every clause of window_valid, wrap-around included; rows as given, none for the empty window; overlap over window_bytes",
                 "items: 1608 edge and 600 random geometries (k in 1, 2, 4, 8), each without a base, with one, and in place with the items in either order: "
                 "the items tile the window once, every source index lies inside the entry, no stored byte is read twice, every byte is the map, "
                 "the window whole is the join",
                 "wide path: more than half of the window bytes walked"):
        assert line in p.stdout, p.stdout
    assert "FAILED" not in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def _window_bytes_by_the_map(stored, k, w):
    """the map of window_copy_plan.h, byte by byte, in numpy: destination byte d <- stored[plane_stored_index(i(d))]"""
    row_bytes, row0, rows, col0, cols = w
    d = np.arange(rows * cols, dtype=np.int64)
    if d.size == 0:
        return np.zeros(0, dtype=np.uint8)
    i = (row0 + d // cols) * row_bytes + col0 + d % cols
    m = stored.size // k
    return stored[(i % k) * m + i // k]


def test_every_slice_along_one_dimension_is_the_window_of_the_formula():
    """arange tensors of every dtype width, 1-D to 4-D, every dim, a few [start, stop): the window of slice_window, read through the map
    from the entry's bytes, is the numpy slice made contiguous; and the codec's rule accepts it with that many bytes"""
    codec = zpack_amd.lib()
    shapes = [(7,), (1,), (5, 6), (1, 9), (9, 1), (3, 4, 5), (2, 1, 7), (2, 3, 4, 5), (1, 2, 1, 3)]
    checked = 0
    for shape, dtype in itertools.product(shapes, (np.uint8, np.uint16, np.uint32, np.uint64)):
        k = np.dtype(dtype).itemsize
        t = (np.arange(int(np.prod(shape)), dtype=np.uint64) * 0x9E3779B97F4A7C15 >> 7).astype(dtype).reshape(shape)
        plain = t.reshape(-1).view(np.uint8)
        for dim in range(-len(shape), len(shape)):
            size = shape[dim]
            for start, stop in {(0, size), (0, 0), (size, size), (0, 1), (size - 1, size), (size // 3, size - size // 4)}:
                w = zpack_amd.slice_window(shape, dim, start, stop, k)
                want = np.ascontiguousarray(t[(slice(None),) * (dim % len(shape)) + (slice(start, stop),)]).reshape(-1).view(np.uint8)
                assert w[2] * w[4] == want.size
                # as plain bytes (element size 1) and as byte planes of the dtype's width: the same bytes come out
                assert np.array_equal(_window_bytes_by_the_map(plain, 1, w), want), (shape, dtype, dim, start, stop)
                m = plain.size // k
                stored = plain.reshape(m, k).T.reshape(-1)
                assert np.array_equal(_window_bytes_by_the_map(stored, k, w), want), (shape, dtype, dim, start, stop)
                rec = np.array([w], dtype=zpack_amd.WINDOW)
                out = C.c_uint64(77)
                assert codec.zpk_codec_window_valid(plain.size, k, rec.ctypes.data, C.byref(out)) == 1 and out.value == want.size
                checked += 1
    assert checked > 500
    for bad in (((4, 5), 2, 0, 1), ((4, 5), -3, 0, 1), ((4, 5), 1, 3, 2), ((4, 5), 1, 0, 6), ((4, 5), 0, -1, 2), ((), 0, 0, 0)):
        with pytest.raises(ValueError):
            zpack_amd.slice_window(*bad)


def test_the_rule_as_the_codec_exports_it():
    codec = zpack_amd.lib()

    def valid(n, k, *w):
        rec = np.array([w], dtype=zpack_amd.WINDOW)
        return codec.zpk_codec_window_valid(n, k, rec.ctypes.data, None)

    assert valid(256, 4, 64, 1, 2, 8, 16) == 1
    assert valid(256, 4, 0, 0, 0, 0, 0) == 0                                            # no window
    assert valid(250, 1, 64, 0, 1, 0, 8) == 0                                           # a tail
    assert valid(256, 4, 64, 1, 2, 6, 16) == 0 and valid(256, 4, 64, 1, 2, 8, 18) == 0 and valid(252, 4, 42, 0, 1, 0, 8) == 0     # whole elements
    assert valid(256, 4, 64, 1, 2, 52, 16) == 0 and valid(256, 4, 64, 3, 2, 8, 16) == 0                                      # inside the matrix
    assert valid(256, 4, 64, 1, 2, 2 ** 64 - 4, 8) == 0 and valid(256, 4, 64, 2 ** 64 - 1, 2, 8, 16) == 0                    # wrap-around
    assert valid(256, 3, 64, 1, 2, 9, 15) == 0 and valid(256, 0, 64, 1, 2, 8, 16) == 0                                       # element sizes
    assert valid(256, 4, 64, 4, 0, 64, 0) == 1                                          # the empty window
    assert codec.zpk_codec_window_valid(256, 4, None, None) == 0
    rec = np.array([(64, 1, 2, 8, 16)], dtype=zpack_amd.WINDOW)                         # 32 bytes
    ok = codec.zpk_codec_window_overlap_ok
    assert ok(1000, 1000, rec.ctypes.data) == 1 and ok(1000, 1032, rec.ctypes.data) == 1 and ok(1032, 1000, rec.ctypes.data) == 1
    assert ok(1000, 1031, rec.ctypes.data) == 0 and ok(1031, 1000, rec.ctypes.data) == 0 and ok(1000, 1001, rec.ctypes.data) == 0


def test_both_libraries_export_the_new_calls_and_the_headers_declare_them():
    codec = C.CDLL(zpack_amd.CODEC_SO)
    codec_names = ("zpk_codec_window_copy_device", "zpk_codec_window_stats", "zpk_codec_window_valid", "zpk_codec_window_overlap_ok",
                   "zpk_codec_decode_batch_host_dptr_windows", "zpk_codec_decode_batch_dimage_windows")
    for name in codec_names:
        assert hasattr(codec, name), name
    lib = C.CDLL(zpack_amd.ZPACK_SO)
    assert hasattr(lib, "zpack_amd_read_files_device_windows")
    codec_h = open(os.path.join(ROOT, "include", "zpack_codec.h")).read()
    for name in codec_names:
        assert re.search(r"\bint\s+%s\s*\(" % name, codec_h), name
    assert "typedef struct zpk_window { uint64_t row_bytes, row0, rows, col0, cols; } zpk_window;" in codec_h
    assert "typedef struct zpk_window_copy { uint64_t src, dst, base, n; zpk_window win; uint32_t elem, pad; } zpk_window_copy;" in codec_h
    assert re.search(r"#define\s+ZPK_CODEC_ABI_VERSION\s+3\b", codec_h)                 # additive: the ABI version stays
    amd_h = open(os.path.join(ROOT, "include", "zpack_amd.h")).read()
    assert re.search(r"ZPACK_EXPORT\s+int\s+zpack_amd_read_files_device_windows\s*\(", amd_h)
    assert "typedef struct zpack_amd_window { zpack_u64 row_bytes, row0, rows, col0, cols; } zpack_amd_window;" in amd_h
    zpack_h = open(os.path.join(ROOT, "include", "zpack.h")).read()
    assert "zpack_amd_" not in zpack_h and len(re.findall(r"^ZPACK_EXPORT\b", zpack_h, flags=re.M)) == 54       # zpack.h keeps its 54 prototypes
    assert zpack_amd.WINDOW.itemsize == 40 and zpack_amd.WINDOW.names == ("row_bytes", "row0", "rows", "col0", "cols")
    assert zpack_amd.WINDOW_COPY.itemsize == 80 and zpack_amd.WINDOW_COPY.names == ("src", "dst", "base", "n", "win", "elem", "pad")
    assert callable(zpack_amd.Codec.window_copy_device) and callable(zpack_amd.Codec.window_stats)


def test_null_arrays_bad_element_sizes_and_bad_windows_are_stream_invalid_before_any_context(L):
    """with or without a device: these are judged first, no context is created, no result is set"""
    r = _reader(L)
    try:
        ents = (C.POINTER(FileEntry) * 2)(C.pointer(r.file_entries[0]), C.pointer(r.file_entries[1]))
        n0, n1 = int(r.file_entries[0].uncomp_size), int(r.file_entries[1].uncomp_size)
        assert n0 > 2 and n1 > 2
        bufs = (C.c_void_p * 2)(0x10000, 0x20000)
        caps = (C.c_size_t * 2)(1 << 20, 1 << 20)
        res = (C.c_int * 2)(-7, -7)
        whole = (Window * 2)(Window(0, 0, 0, 0, 0), Window(n1, 0, 1, 0, n1))
        rd = L.zpack_amd_read_files_device_windows
        assert rd(None, ents, 2, bufs, caps, None, None, None, whole, res, None) == STREAM_INVALID
        assert rd(C.byref(r), None, 2, bufs, caps, None, None, None, whole, res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, None, caps, None, None, None, whole, res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, bufs, None, None, None, None, whole, res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, bufs, caps, None, None, None, whole, None, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, bufs, caps, (C.c_uint8 * 2)(3, 1), None, None, whole, res, None) == STREAM_INVALID
        for bad in (Window(n1 + 1, 0, 1, 0, 1),             # n is no multiple of row_bytes
                    Window(n1, 0, 2, 0, 1),                 # a row too many
                    Window(n1, 1, 1, 0, 1),                 # ... or one too far down
                    Window(n1, 0, 1, 1, n1),                # past the row's end
                    Window(n1, 0, 1, n1, 1),
                    Window(n1, 0, 1, 2 ** 64 - 1, 2),       # a sum that wraps
                    Window(n1, 2 ** 64 - 1, 2, 0, 1)):
            assert rd(C.byref(r), ents, 2, bufs, caps, None, None, None, (Window * 2)(Window(0, 0, 0, 0, 0), bad), res, None) == STREAM_INVALID
        # element sizes decide too: a window of bytes that is no window of 2-byte elements
        odd = (Window * 2)(Window(0, 0, 0, 0, 0), Window(n1, 0, 1, 1, 1))
        if n1 % 2 == 0:
            assert rd(C.byref(r), ents, 2, bufs, caps, (C.c_uint8 * 2)(1, 2), None, None, odd, res, None) == STREAM_INVALID
        # a base that overlaps its window's buffer other than by being it (the window has n1 - 1 bytes)
        part = (Window * 2)(Window(0, 0, 0, 0, 0), Window(n1, 0, 1, 0, n1 - 1))
        for off in (1, n1 - 2, -1):
            bases = (C.c_void_p * 2)(None, 0x20000 + off)
            assert rd(C.byref(r), ents, 2, bufs, caps, None, bases, None, part, res, None) == STREAM_INVALID
        assert list(res) == [-7, -7] and not r.zstd_dctx
    finally:
        L.zpack_close_reader(C.byref(r))


def test_without_a_device_the_call_is_not_available(L):
    if not _no_device():
        pytest.skip("a HIP device is present: tests/test_gpu_window_io.py covers the call")
    r = _reader(L)
    try:
        ents = (C.POINTER(FileEntry) * 2)(C.pointer(r.file_entries[0]), C.pointer(r.file_entries[1]))
        n1 = int(r.file_entries[1].uncomp_size)
        bufs = (C.c_void_p * 2)(None, None)
        caps = (C.c_size_t * 2)(1 << 20, 1 << 20)
        res = (C.c_int * 2)(-7, -7)
        for wins in (None, (Window * 2)(Window(0, 0, 0, 0, 0), Window(n1, 0, 1, 0, n1))):
            for bases in (None, (C.c_void_p * 2)(None, None)):
                assert L.zpack_amd_read_files_device_windows(C.byref(r), ents, 2, bufs, caps, None, bases, None, wins, res, None) == NOT_AVAILABLE
        assert list(res) == [-7, -7]
    finally:
        L.zpack_close_reader(C.byref(r))
