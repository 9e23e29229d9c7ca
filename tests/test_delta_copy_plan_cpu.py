"""Delta entries without a GPU: the layout and the row table of k_delta_copy (zpack_amd/csrc/delta_copy_plan.h) under ASan + UBSan —
split then join is the identity, the items tile the bytes once, a join in place reads no base byte another item writes —, the new symbols
of both libraries, and what the two library calls answer before they need a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import zpack_amd
from tests._libs import ZPackAPI, Reader, Writer, File, FileEntry, CompressOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tools", "hostfuzz", "run_delta_copy_plan.sh")
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
STREAM_INVALID, NOT_AVAILABLE = 21, 24


@pytest.fixture(scope="module")
def L():
    lib = ZPackAPI(zpack_amd.ZPACK_SO).lib
    lib.zpack_amd_write_files_device_delta.argtypes = [C.POINTER(Writer), C.POINTER(File), C.c_uint64, C.POINTER(C.c_uint8), C.POINTER(C.c_void_p)]
    lib.zpack_amd_read_files_device_delta.argtypes = [C.POINTER(Reader), C.POINTER(C.POINTER(FileEntry)), C.c_uint64, C.POINTER(C.c_void_p),
                                                      C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p]
    return lib


def _no_device():
    lib = zpack_amd.lib()
    lib.zpk_codec_device_count.restype = C.c_int
    return lib.zpk_codec_device_count() <= 0


def _files(n=2, size=64):
    opts = CompressOptions(2, 0)
    arr = (File * n)()
    for i in range(n):
        arr[i].filename = b"x%d" % i
        arr[i].buffer = None
        arr[i].size = size
        arr[i].options = C.pointer(opts)
    return arr, opts


def _reader(L):
    r = Reader()
    path = os.path.join(ROOT, "tests", "golden", "ref_workdir", "archive_lz4.zpk")
    assert L.zpack_init_reader(C.byref(r), path.encode()) == 0
    assert r.file_count == 2
    return r


@needs_gxx
def test_delta_copy_plan_under_asan_ubsan():
    p = subprocess.run(["bash", SCRIPT], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    for line in ("rows: as given with base, element size and direction; none for the empty row, none without a base; item_base ascending",
                 "overlap: the same address passes, disjoint ranges pass, every partial overlap is refused",
                 "layout: 48 rows (k in 1, 2, 4, 8; n around k, 16 k, 1024 k, one piece and three): stored = split(plain ^ base), join inverts it, "
                 "in place too and with the items in either order; the items tile source, base and destination once; 358160 of 358949 bytes take the wide path"):
        assert line in p.stdout, p.stdout
    assert "FAILED" not in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_both_libraries_export_the_new_calls_and_the_headers_declare_them():
    codec = C.CDLL(zpack_amd.CODEC_SO)
    codec_names = ("zpk_codec_delta_copy_device", "zpk_codec_delta_stats", "zpk_codec_encode_batch_dsrc_delta", "zpk_codec_encode_batch_dsink_delta",
                   "zpk_codec_decode_batch_host_dptr_delta", "zpk_codec_decode_batch_dimage_delta")
    for name in codec_names:
        assert hasattr(codec, name), name
    lib = C.CDLL(zpack_amd.ZPACK_SO)
    lib_names = ("zpack_amd_write_files_device_delta", "zpack_amd_read_files_device_delta")
    for name in lib_names:
        assert hasattr(lib, name), name
    codec_h = open(os.path.join(ROOT, "include", "zpack_codec.h")).read()
    for name in codec_names:
        assert re.search(r"\bint\s+%s\s*\(" % name, codec_h), name
    assert "typedef struct zpk_delta_copy { uint64_t src, dst, base, len; uint32_t elem, join; } zpk_delta_copy;" in codec_h
    assert re.search(r"#define\s+ZPK_CODEC_ABI_VERSION\s+3\b", codec_h)                 # additive: the ABI version stays
    amd_h = open(os.path.join(ROOT, "include", "zpack_amd.h")).read()
    for name in lib_names:
        assert re.search(r"ZPACK_EXPORT\s+int\s+%s\s*\(" % name, amd_h), name
    zpack_h = open(os.path.join(ROOT, "include", "zpack.h")).read()
    assert "zpack_amd_" not in zpack_h and len(re.findall(r"^ZPACK_EXPORT\b", zpack_h, flags=re.M)) == 54       # zpack.h keeps its 54 prototypes
    assert zpack_amd.DELTA_COPY.itemsize == 40 and zpack_amd.DELTA_COPY.names == ("src", "dst", "base", "len", "elem", "join")
    assert callable(zpack_amd.Codec.delta_copy_device) and callable(zpack_amd.Codec.delta_stats)


def test_null_arrays_and_an_element_size_of_three_are_stream_invalid_before_any_context(L):
    """with or without a device: these are judged first, nothing is written, no context is created, no result is set"""
    w = Writer()
    assert L.zpack_init_writer_heap(C.byref(w), 0) == 0
    try:
        arr, _opts = _files()
        bases = (C.c_void_p * 2)(None, None)
        wr = L.zpack_amd_write_files_device_delta
        assert wr(None, arr, 2, None, bases) == STREAM_INVALID
        assert wr(C.byref(w), None, 2, None, bases) == STREAM_INVALID
        assert wr(C.byref(w), arr, 2, (C.c_uint8 * 2)(2, 3), bases) == STREAM_INVALID
        assert wr(C.byref(w), arr, 2, (C.c_uint8 * 2)(3, 1), None) == STREAM_INVALID
        assert w.write_offset == 0 and w.file_count == 0 and not w.zstd_cctx
    finally:
        L.zpack_close_writer(C.byref(w))
    r = _reader(L)
    try:
        ents = (C.POINTER(FileEntry) * 2)(C.pointer(r.file_entries[0]), C.pointer(r.file_entries[1]))
        bufs = (C.c_void_p * 2)(None, None)
        caps = (C.c_size_t * 2)(1 << 20, 1 << 20)
        bases = (C.c_void_p * 2)(None, None)
        res = (C.c_int * 2)(-7, -7)
        rd = L.zpack_amd_read_files_device_delta
        assert rd(None, ents, 2, bufs, caps, None, bases, res, None) == STREAM_INVALID
        assert rd(C.byref(r), None, 2, bufs, caps, None, bases, res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, None, caps, None, bases, res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, bufs, None, None, bases, res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, bufs, caps, None, bases, None, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, bufs, caps, (C.c_uint8 * 2)(3, 4), bases, res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, bufs, caps, (C.c_uint8 * 2)(4, 3), None, res, None) == STREAM_INVALID
        assert list(res) == [-7, -7] and not r.zstd_dctx
    finally:
        L.zpack_close_reader(C.byref(r))


def test_without_a_device_both_calls_are_not_available(L):
    if not _no_device():
        pytest.skip("a HIP device is present: tests/test_gpu_delta_io.py covers the calls")
    w = Writer()
    assert L.zpack_init_writer_heap(C.byref(w), 0) == 0
    try:
        arr, _opts = _files()
        for elem in (None, (C.c_uint8 * 2)(2, 4)):
            for bases in (None, (C.c_void_p * 2)(None, None)):
                assert L.zpack_amd_write_files_device_delta(C.byref(w), arr, 2, elem, bases) == NOT_AVAILABLE
        assert w.write_offset == 0 and w.file_count == 0
    finally:
        L.zpack_close_writer(C.byref(w))
    r = _reader(L)
    try:
        ents = (C.POINTER(FileEntry) * 2)(C.pointer(r.file_entries[0]), C.pointer(r.file_entries[1]))
        bufs = (C.c_void_p * 2)(None, None)
        caps = (C.c_size_t * 2)(1 << 20, 1 << 20)
        res = (C.c_int * 2)(-7, -7)
        for elem in (None, (C.c_uint8 * 2)(2, 4)):
            for bases in (None, (C.c_void_p * 2)(None, None)):
                assert L.zpack_amd_read_files_device_delta(C.byref(r), ents, 2, bufs, caps, elem, bases, res, None) == NOT_AVAILABLE
        assert list(res) == [-7, -7]
    finally:
        L.zpack_close_reader(C.byref(r))
