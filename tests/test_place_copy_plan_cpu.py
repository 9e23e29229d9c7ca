"""Placed reads without a GPU: the pitch, its rule, the extent, the row table of k_place_copy and the placed offsets
(zpack_amd/csrc/place_copy_plan.h) under ASan + UBSan — every placed byte written once, no gap byte, nothing outside the extent, the rule
against a 128-bit model at the wrap —, the rule and the overlap rule as the codec exports them, over every clause, the text of
zpk_place_copy and its size, the destination-to-placement formula against numpy slicing, the new symbols of both libraries, and what the
library call answers before it needs a device."""
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
SCRIPT = os.path.join(ROOT, "tools", "hostfuzz", "run_place_copy_plan.sh")
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
STREAM_INVALID, NOT_AVAILABLE = 21, 24


class Window(C.Structure):
    _fields_ = [("row_bytes", C.c_uint64), ("row0", C.c_uint64), ("rows", C.c_uint64), ("col0", C.c_uint64), ("cols", C.c_uint64)]


@pytest.fixture(scope="module")
def L():
    lib = ZPackAPI(zpack_amd.ZPACK_SO).lib
    lib.zpack_amd_read_files_device_placed.argtypes = [C.POINTER(Reader), C.POINTER(C.POINTER(FileEntry)), C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                       C.POINTER(C.c_uint8), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(Window), C.POINTER(C.c_uint64),
                                                       C.POINTER(C.c_int), C.c_void_p]
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
def test_place_copy_plan_under_asan_ubsan():
    p = subprocess.run(["bash", SCRIPT], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    for line in ("rule: every clause of place_valid against a 128-bit model, products past 32 bits and pitches at the wrap; rows as given, none for no bytes; "
                 "overlap over the extent",
                 "items: 1736 edge and ",
                 "each without a base, with one, and in place with the items in either order: every placed byte written once, no gap byte, nothing outside the extent, "
                 "every byte the map"):
        assert line in p.stdout, p.stdout
    assert "FAILED" not in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_the_text_of_zpk_place_copy_and_its_size():
    codec_h = open(os.path.join(ROOT, "include", "zpack_codec.h")).read()
    assert "typedef struct zpk_place_copy { uint64_t src, dst, base, n; zpk_window win; uint64_t pitch; uint32_t elem, pad; } zpk_place_copy;" in codec_h
    assert zpack_amd.PLACE_COPY.names == ("src", "dst", "base", "n", "win", "pitch", "elem", "pad")
    if shutil.which("gcc"):                                                             # sizeof, as the compiler lays the header's struct out
        src = '#include <stdio.h>\n#include <stddef.h>\n#include "zpack_codec.h"\nint main(void) { printf("%zu %zu %zu", sizeof(zpk_place_copy), offsetof(zpk_place_copy, pitch), offsetof(zpk_place_copy, elem)); return 0; }\n'
        import tempfile
        with tempfile.TemporaryDirectory() as work:
            open(os.path.join(work, "s.c"), "w").write(src)
            subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(work, "s"), os.path.join(work, "s.c")])
            size, at_pitch, at_elem = (int(x) for x in subprocess.check_output([os.path.join(work, "s")], text=True).split())
        assert zpack_amd.PLACE_COPY.itemsize == size and zpack_amd.PLACE_COPY.fields["pitch"][1] == at_pitch and zpack_amd.PLACE_COPY.fields["elem"][1] == at_elem
    assert zpack_amd.PLACE_COPY.itemsize == 88                                          # 4 x 8 + 40 + 8 + 2 x 4
    # the structs that exist keep their layouts
    assert zpack_amd.WINDOW_COPY.itemsize == 80 and zpack_amd.WINDOW.itemsize == 40


def test_the_rule_and_the_overlap_rule_as_the_codec_exports_them():
    codec = zpack_amd.lib()

    def valid(n, k, w, pitch):
        rec = np.array([w], dtype=zpack_amd.WINDOW)
        out = C.c_uint64(77)
        ok = codec.zpk_codec_place_valid(n, k, rec.ctypes.data, pitch, C.byref(out))
        assert ok in (0, 1) and (ok == 1 or out.value == 77)                            # a refusal writes no extent
        return (ok, out.value) if ok else (0, None)

    W = (64, 1, 2, 8, 16)                                                               # 2 rows of 16 bytes of an entry of 256
    assert valid(256, 4, W, 15) == (0, None)                                            # pitch cols - 1
    assert valid(256, 4, W, 16) == (1, 32)                                              # cols: dense
    assert valid(256, 4, W, 17) == (1, 33)                                              # cols + 1: no alignment to the element size
    assert valid(256, 4, W, 0) == (0, None)                                             # no pitch is no placement
    assert valid(256, 4, (64, 3, 2, 8, 16), 64) == (0, None) and valid(256, 4, (0, 0, 0, 0, 0), 64) == (0, None) and valid(256, 3, W, 64) == (0, None)   # window_valid
    # an extent that wraps: (rows - 1) * pitch + cols, tested with a division
    assert valid(256, 4, W, 2 ** 64 - 17) == (1, 2 ** 64 - 1) and valid(256, 4, W, 2 ** 64 - 16) == (0, None) and valid(256, 4, W, 2 ** 64 - 1) == (0, None)
    tall = (8, 0, 2 ** 33, 0, 8)                                                        # products past 32 bits: 2^33 rows
    assert valid(2 ** 36, 8, tall, 2 ** 20) == (1, (2 ** 33 - 1) * 2 ** 20 + 8)
    assert valid(2 ** 36, 8, tall, 2 ** 31) == (1, (2 ** 33 - 1) * 2 ** 31 + 8) and valid(2 ** 36, 8, tall, 2 ** 31 + 1) == (0, None)
    # rows == 0, cols == 0: valid at any pitch but 0, an extent of 0
    assert valid(256, 4, (64, 1, 0, 8, 16), 16) == (1, 0) and valid(256, 4, (64, 4, 0, 8, 16), 2 ** 64 - 1) == (1, 0) and valid(256, 4, (64, 1, 0, 8, 16), 15) == (0, None)
    assert valid(256, 4, (64, 1, 2, 8, 0), 1) == (1, 0) and valid(256, 4, (64, 1, 2, 8, 0), 2 ** 64 - 1) == (1, 0) and valid(256, 4, (64, 1, 2, 8, 0), 0) == (0, None)
    assert valid(256, 4, (64, 1, 1, 8, 16), 2 ** 64 - 1) == (1, 16)                     # one row: the pitch multiplies nothing
    assert codec.zpk_codec_place_valid(256, 4, None, 16, None) == 0
    rec = np.array([W], dtype=zpack_amd.WINDOW)
    assert codec.zpk_codec_place_valid(256, 4, rec.ctypes.data, 16, None) == 1          # (no extent wanted)
    # the overlap rule, over the EXTENT: W at pitch 24 spans 40 bytes though the window has 32
    ok = codec.zpk_codec_place_overlap_ok
    p = rec.ctypes.data
    assert ok(1000, 1000, p, 24) == 1 and ok(1000, 1040, p, 24) == 1 and ok(1040, 1000, p, 24) == 1
    assert ok(1000, 1039, p, 24) == 0 and ok(1039, 1000, p, 24) == 0 and ok(1000, 1032, p, 24) == 0 and ok(1000, 1001, p, 24) == 0 and ok(1000, 1016, p, 24) == 0
    assert ok(1000, 1032, p, 16) == 1 and ok(1000, 1031, p, 16) == 0                    # pitch == cols: the window's rule
    empty = np.array([(64, 1, 0, 8, 16)], dtype=zpack_amd.WINDOW)
    assert ok(1000, 1001, empty.ctypes.data, 24) == 1 and ok(1000, 1001, None, 24) == 0


def test_place_of_against_numpy_slicing():
    """arange destinations of every dtype width, 1-D to 4-D, every dim, a few [start, start + length): the bytes at byte_offset + r * pitch
    + [0, cols), r in [0, rows), are the numpy slice of the destination made contiguous; and the codec's rule accepts the placement of a
    whole entry of that many bytes with that extent"""
    codec = zpack_amd.lib()
    shapes = [(7,), (1,), (5, 6), (1, 9), (9, 1), (3, 4, 5), (2, 1, 7), (2, 3, 4, 5), (1, 2, 1, 3)]
    checked = 0
    for shape, dtype in itertools.product(shapes, (np.uint8, np.uint16, np.uint32, np.uint64)):
        k = np.dtype(dtype).itemsize
        t = (np.arange(int(np.prod(shape)), dtype=np.uint64) * 0x9E3779B97F4A7C15 >> 7).astype(dtype).reshape(shape)
        flat = t.reshape(-1).view(np.uint8)
        for dim in range(-len(shape), len(shape)):
            size = shape[dim]
            for start, length in {(0, size), (0, 0), (size, 0), (0, 1), (size - 1, 1), (size // 3, size - size // 4 - size // 3)}:
                rows, cols, pitch, offset = zpack_amd.place_of(shape, dim, start, length, k)
                want = np.ascontiguousarray(t[(slice(None),) * (dim % len(shape)) + (slice(start, start + length),)]).reshape(-1).view(np.uint8)
                assert rows * cols == want.size, (shape, dtype, dim, start, length)
                d = np.arange(rows * cols, dtype=np.int64)
                got = flat[offset + (d // cols) * pitch + d % cols] if d.size else flat[:0]
                assert np.array_equal(got, want), (shape, dtype, dim, start, length)
                if cols:
                    rec = np.array([(cols, 0, rows, 0, cols)], dtype=zpack_amd.WINDOW)   # the entry whole
                    ext = C.c_uint64(77)
                    assert codec.zpk_codec_place_valid(rows * cols, k, rec.ctypes.data, pitch, C.byref(ext)) == 1
                    assert ext.value == (rows - 1) * pitch + cols and offset + ext.value <= flat.size
                checked += 1
    assert checked > 500
    for bad in (((4, 5), 2, 0, 1), ((4, 5), -3, 0, 1), ((4, 5), 1, 3, 3), ((4, 5), 1, 0, 6), ((4, 5), 0, -1, 2), ((4, 5), 0, 1, -1), ((), 0, 0, 0)):
        with pytest.raises(ValueError):
            zpack_amd.place_of(*bad)


def test_both_libraries_export_the_new_calls_and_the_headers_declare_them():
    codec = C.CDLL(zpack_amd.CODEC_SO)
    codec_names = ("zpk_codec_place_copy_device", "zpk_codec_place_stats", "zpk_codec_place_valid", "zpk_codec_place_overlap_ok",
                   "zpk_codec_decode_batch_host_dptr_placed", "zpk_codec_decode_batch_dimage_placed")
    for name in codec_names:
        assert hasattr(codec, name), name
    lib = C.CDLL(zpack_amd.ZPACK_SO)
    assert hasattr(lib, "zpack_amd_read_files_device_placed")
    codec_h = open(os.path.join(ROOT, "include", "zpack_codec.h")).read()
    for name in codec_names:
        assert re.search(r"\bint\s+%s\s*\(" % name, codec_h), name
    assert re.search(r"#define\s+ZPK_CODEC_ABI_VERSION\s+3\b", codec_h)                 # additive: the ABI version stays
    amd_h = open(os.path.join(ROOT, "include", "zpack_amd.h")).read()
    assert re.search(r"ZPACK_EXPORT\s+int\s+zpack_amd_read_files_device_placed\s*\(", amd_h)
    assert callable(zpack_amd.Codec.place_copy_device) and callable(zpack_amd.Codec.place_stats) and callable(zpack_amd.place_of)


def test_bad_placements_are_stream_invalid_before_any_context(L):
    """with or without a device: these are judged first, no context is created, no result is set"""
    r = _reader(L)
    try:
        ents = (C.POINTER(FileEntry) * 2)(C.pointer(r.file_entries[0]), C.pointer(r.file_entries[1]))
        assert int(r.file_entries[0].uncomp_size) == 169                               # 13 rows of 13 bytes
        bufs = (C.c_void_p * 2)(0x10000, 0x20000)
        caps = (C.c_size_t * 2)(1 << 20, 1 << 20)
        res = (C.c_int * 2)(-7, -7)
        two = (Window * 2)(Window(13, 0, 13, 0, 13), Window(0, 0, 0, 0, 0))             # the first entry as 13 rows, the second whole
        rd = L.zpack_amd_read_files_device_placed

        def pitches(a, b=0):
            return (C.c_uint64 * 2)(a, b)

        assert rd(None, ents, 2, bufs, caps, None, None, None, two, pitches(13), res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, None, caps, None, None, None, two, pitches(13), res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, bufs, caps, None, None, None, two, pitches(12), res, None) == STREAM_INVALID              # rows that run into each other
        assert rd(C.byref(r), ents, 2, bufs, caps, None, None, None, two, pitches((2 ** 64 - 14) // 12 + 1), res, None) == STREAM_INVALID   # an extent that wraps
        assert rd(C.byref(r), ents, 2, bufs, caps, None, None, None, two, pitches(13, 13), res, None) == STREAM_INVALID          # a pitch without a window
        assert rd(C.byref(r), ents, 2, bufs, caps, None, None, None, None, pitches(13), res, None) == STREAM_INVALID             # ... without any
        bad_win = (Window * 2)(Window(13, 0, 14, 0, 13), Window(0, 0, 0, 0, 0))
        assert rd(C.byref(r), ents, 2, bufs, caps, None, None, None, bad_win, pitches(21), res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, bufs, caps, (C.c_uint8 * 2)(2, 1), None, None, two, pitches(21), res, None) == STREAM_INVALID    # 13 bytes are no 2-byte elements
        # a base that overlaps its placed entry's buffer other than by being it: over the EXTENT (12 * 113 + 13 = 1369 bytes), gaps included
        for off in (1, 13, 60, 1368, -1, -1368):
            bases = (C.c_void_p * 2)(0x10000 + off, None)
            assert rd(C.byref(r), ents, 2, bufs, caps, None, bases, None, two, pitches(113), res, None) == STREAM_INVALID, off
        # a placed base in a call that checks hashes — unless its extent is its window's bytes
        bases = (C.c_void_p * 2)(0x10000, None)
        hashes = (C.c_uint64 * 2)(0, 0)
        assert rd(C.byref(r), ents, 2, bufs, caps, None, bases, hashes, two, pitches(113), res, None) == STREAM_INVALID
        assert list(res) == [-7, -7] and not r.zstd_dctx
        if _no_device():                                                                # what passes the rule reaches the device question
            apart = (C.c_void_p * 2)(0x10000 + 1369, None)
            for args in ((None, None, pitches(113)), (bases, None, pitches(113)), (apart, None, pitches(113)), (bases, hashes, pitches(13)), (None, None, None)):
                assert rd(C.byref(r), ents, 2, bufs, caps, None, args[0], args[1], two, args[2], res, None) == NOT_AVAILABLE
            assert list(res) == [-7, -7]
    finally:
        L.zpack_close_reader(C.byref(r))
