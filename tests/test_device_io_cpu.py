"""CPU: the device-memory reads and writes of the library API (include/zpack_amd.h) as far as a machine without a GPU can see them.
libzpack_amd.so exports the three calls; NULL arrays are ZPACK_ERROR_STREAM_INVALID (21) before any context is created, and without a
HIP device every call is ZPACK_ERROR_NOT_AVAILABLE (24): there is no CPU fallback.  libzpk_codec.so exports the codec calls behind them
at ABI version 3.  zpack_amd/csrc/span_copy_plan.h — the row table, work items and launches of k_span_copy, the staging slots, the
packed offsets, the pointer test: the very header the codec compiles — runs under AddressSanitizer + UBSan
(tools/hostfuzz/span_copy_plan_main.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import zpack_amd
from tests._libs import ZPackAPI, Reader, Writer, File, FileEntry, CompressOptions, u8p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_INVALID, NOT_AVAILABLE = 21, 24
NEW_CODEC_CALLS = ["zpk_codec_decode_batch_host_dptr", "zpk_codec_encode_batch_dsrc", "zpk_codec_copy_spans_device",
                   "zpk_codec_pointer_device", "zpk_codec_packed_stride"]


@pytest.fixture(scope="module")
def Z():
    z = ZPackAPI(zpack_amd.ZPACK_SO)
    L = z.lib
    L.zpack_amd_read_files_device.argtypes = [C.POINTER(Reader), C.POINTER(C.POINTER(FileEntry)), C.c_uint64, C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.c_void_p]
    L.zpack_amd_read_files_device_packed.argtypes = [C.POINTER(Reader), C.POINTER(C.POINTER(FileEntry)), C.c_uint64, C.c_void_p, C.c_size_t,
                                                     C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.c_void_p]
    L.zpack_amd_write_files_device.argtypes = [C.POINTER(Writer), C.POINTER(File), C.c_uint64]
    return z


def _no_device():
    L = zpack_amd.lib()
    L.zpk_codec_device_count.restype = C.c_int
    return L.zpk_codec_device_count() <= 0


def _reader(Z, golden_dir):
    r = Reader()
    assert Z.lib.zpack_init_reader(C.byref(r), os.path.join(golden_dir, "ref_workdir", "archive_lz4.zpk").encode()) == 0
    assert r.file_count == 2
    return r


def test_the_library_exports_the_three_calls_and_the_header_declares_them(Z):
    hdr = open(os.path.join(ROOT, "include", "zpack_amd.h")).read()
    for name in ("zpack_amd_read_files_device", "zpack_amd_read_files_device_packed", "zpack_amd_write_files_device"):
        assert getattr(Z.lib, name) is not None
        assert re.search(r"ZPACK_EXPORT\s+int\s+%s\s*\(" % name, hdr), name
    zpack_h = open(os.path.join(ROOT, "include", "zpack.h")).read()
    assert "zpack_amd_" not in zpack_h                                               # zpack.h stays the reference's header


def test_null_arrays_are_stream_invalid_before_any_context(Z, golden_dir):
    r = _reader(Z, golden_dir)
    try:
        ents = (C.POINTER(FileEntry) * 2)(C.pointer(r.file_entries[0]), C.pointer(r.file_entries[1]))
        bufs = (C.c_void_p * 2)()
        caps = (C.c_size_t * 2)(350, 350)
        res = (C.c_int * 2)(-1, -1)
        offs = (C.c_uint64 * 2)()
        rd = Z.lib.zpack_amd_read_files_device
        assert rd(None, ents, 2, bufs, caps, res, None) == STREAM_INVALID
        assert rd(C.byref(r), None, 2, bufs, caps, res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, None, caps, res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, bufs, None, res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, bufs, caps, None, None) == STREAM_INVALID
        pk = Z.lib.zpack_amd_read_files_device_packed
        assert pk(None, ents, 2, 4096, 1024, offs, res, None) == STREAM_INVALID
        assert pk(C.byref(r), None, 2, 4096, 1024, offs, res, None) == STREAM_INVALID
        assert pk(C.byref(r), ents, 2, None, 1024, offs, res, None) == STREAM_INVALID
        assert pk(C.byref(r), ents, 2, 4096, 1024, None, res, None) == STREAM_INVALID
        assert pk(C.byref(r), ents, 2, 4096, 1024, offs, None, None) == STREAM_INVALID
        assert not r.zstd_dctx and list(res) == [-1, -1]                             # no context was created, no result written
        w = Writer()
        assert Z.lib.zpack_init_writer_heap(C.byref(w), 0) == 0
        wr = Z.lib.zpack_amd_write_files_device
        assert wr(None, (File * 1)(), 1) == STREAM_INVALID
        assert wr(C.byref(w), None, 1) == STREAM_INVALID
        assert not w.zstd_cctx and w.file_count == 0 and w.write_offset == 0
        Z.lib.zpack_close_writer(C.byref(w))
    finally:
        Z.lib.zpack_close_reader(C.byref(r))


def test_without_a_device_every_call_is_not_available(Z, golden_dir):
    if not _no_device():
        pytest.skip("a HIP device is present: tests/test_gpu_device_io.py covers the calls")
    r = _reader(Z, golden_dir)
    try:
        ents = (C.POINTER(FileEntry) * 2)(C.pointer(r.file_entries[0]), C.pointer(r.file_entries[1]))
        bufs = (C.c_void_p * 2)(0x1000, 0x2000)                                      # never dereferenced: there is no device to run on
        caps = (C.c_size_t * 2)(350, 350)
        res = (C.c_int * 2)(-1, -1)
        offs = (C.c_uint64 * 2)()
        assert Z.lib.zpack_amd_read_files_device(C.byref(r), ents, 2, bufs, caps, res, None) == NOT_AVAILABLE
        assert Z.lib.zpack_amd_read_files_device(C.byref(r), ents, 0, bufs, caps, res, None) == NOT_AVAILABLE
        assert Z.lib.zpack_amd_read_files_device_packed(C.byref(r), ents, 2, 0x1000, 1024, offs, res, None) == NOT_AVAILABLE
        assert list(res) == [-1, -1]
        w = Writer()
        assert Z.lib.zpack_init_writer_heap(C.byref(w), 0) == 0
        opts = CompressOptions(2, 0)
        arr = (File * 1)()
        arr[0].filename = b"a"; arr[0].buffer = C.cast(0x1000, u8p); arr[0].size = 16; arr[0].options = C.pointer(opts)
        assert Z.lib.zpack_amd_write_files_device(C.byref(w), arr, 1) == NOT_AVAILABLE
        assert w.file_count == 0 and w.write_offset == 0
        Z.lib.zpack_close_writer(C.byref(w))
    finally:
        Z.lib.zpack_close_reader(C.byref(r))


def test_the_codec_exports_the_new_calls_at_abi_version_3():
    L = zpack_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "zpack_codec.h")).read()
    for name in NEW_CODEC_CALLS:
        assert getattr(L, name) is not None
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert L.zpk_codec_abi_version() == 3
    assert re.search(r"#define\s+ZPK_CODEC_ABI_VERSION\s+3\b", hdr)
    L.zpk_codec_packed_stride.restype = C.c_uint64
    L.zpk_codec_packed_stride.argtypes = [C.c_uint64]
    assert [L.zpk_codec_packed_stride(n) for n in (0, 1, 255, 256, 257)] == [0, 256, 256, 256, 512]
    L.zpk_codec_pointer_device.argtypes = [C.c_void_p]
    keep = (C.c_uint8 * 64)()
    assert L.zpk_codec_pointer_device(None) == -1 and L.zpk_codec_pointer_device(C.addressof(keep)) == -1      # host memory is no device's


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
def test_span_copy_plan_under_asan_ubsan():
    p = subprocess.run(["bash", os.path.join(ROOT, "tools", "hostfuzz", "run_span_copy_plan.sh")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    for line in ("rows: 6 spans of the lengths 0, 1, 16383, 16384, 16385, 2^32 + 5 are 5 rows and 262150 items: rows as given, none for the empty span",
                 "item_base: ascending and disjoint without a gap, 15 items searched for land in their own rows",
                 "launches: one grid holds 8589934588 items, one more is a second launch of 1; 262150 items at 1000 a grid are 263 launches that tile them",
                 "slots: read slots hold what the entry may produce, write slots the source and 16 bytes, both at multiples of 256",
                 "staged: the caller's descriptor at its slot's offset; a stored entry that fits is cut to uncomp_size, every other capacity stays",
                 "packed: uncomp_size 0, 1, 255, 256, 257 land at 0, 0, 256, 512, 768 and end at 1280",
                 "range: the first and the last byte of an allocation pass, one before and one behind do not, ptr + len that wraps does not"):
        assert line in p.stdout, p.stdout[-1500:]
