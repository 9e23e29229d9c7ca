"""Byte-plane entries without a GPU: the layout, the row table, the work items and the launches of k_plane_copy
(zpack_amd/csrc/plane_copy_plan.h) under ASan + UBSan, the layout against a numpy model, and the new symbols of both libraries."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import zpack_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tools", "hostfuzz", "run_plane_copy_plan.sh")
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")


def sizes_of(k):
    return [0, 1, k - 1, k, k + 1, 16 * k - 1, 16 * k + 1, 1024 * k - 1, 1024 * k + 1, 16384 - 1, 16384 + 1, 3 * 16384 + 5]


def grouped(a, k):
    """the layout as a numpy model: byte p of every whole element, plane after plane, then the tail"""
    a = np.asarray(a, dtype=np.uint8)
    m = a.size // k
    return np.concatenate([a[:m * k].reshape(m, k).T.reshape(-1), a[m * k:]])


def test_the_model_is_the_layout_the_header_states():
    for k in (1, 2, 4, 8):
        for n in sizes_of(k):
            plain = np.arange(n, dtype=np.uint64).astype(np.uint8) ^ np.uint8(0x5A)
            stored = grouped(plain, k)
            m = n // k
            assert stored.size == n
            for p in range(k):
                assert np.array_equal(stored[p * m:(p + 1) * m], plain[p:m * k:k])      # stored[p*m + j] = plain[j*k + p]
            assert np.array_equal(stored[k * m:], plain[k * m:])                          # the tail stays
            if k == 1:
                assert np.array_equal(stored, plain)


@needs_gxx
def test_plane_copy_plan_under_asan_ubsan():
    p = subprocess.run(["bash", SCRIPT], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    for line in ("layout: 48 rows (k in 1, 2, 4, 8; n around k, 16 k, 1024 k, one piece and three): split is a permutation, join inverts it, "
                 "the items tile the bytes once; 358160 of 358949 bytes take the wide path",
                 "rows: as given with element size and direction, none for the empty row; item_base ascending without a gap, 15 items searched for land in their rows",
                 "launches: one grid holds 8589934588 items, one more is a second launch of 1; 262150 items at 1000 a grid are 263 launches that tile them"):
        assert line in p.stdout, p.stdout
    assert "FAILED" not in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


@needs_gxx
def test_the_driver_walks_the_items_to_what_the_model_says():
    p = subprocess.run(["bash", SCRIPT, "dump"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    seen = set()
    for line in p.stdout.splitlines():
        f = line.split(" ")
        k, n = int(f[0]), int(f[1])
        got = np.frombuffer(bytes.fromhex(f[2]), dtype=np.uint8)
        i = np.arange(n, dtype=np.uint64)
        plain = ((i * np.uint64(131) + (i >> np.uint64(8)) * np.uint64(7) + np.uint64(1)) & np.uint64(255)).astype(np.uint8)
        assert np.array_equal(got, grouped(plain, k)), (k, n)
        seen.add((k, n))
    assert seen == {(k, n) for k in (1, 2, 4, 8) for n in sizes_of(k)}


def test_both_libraries_export_the_new_symbols():
    codec = C.CDLL(zpack_amd.CODEC_SO)
    for name in ("zpk_codec_plane_copy_device", "zpk_codec_planes_stats", "zpk_codec_encode_batch_dsrc_planes", "zpk_codec_encode_batch_dsink_planes",
                 "zpk_codec_decode_batch_host_dptr_planes", "zpk_codec_decode_batch_dimage_planes"):
        assert hasattr(codec, name), name
    lib = C.CDLL(zpack_amd.ZPACK_SO)
    for name in ("zpack_amd_write_files_device_planes", "zpack_amd_read_files_device_planes"):
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "zpack_codec.h")).read() + open(os.path.join(ROOT, "include", "zpack_amd.h")).read()
    for name in ("zpk_codec_plane_copy_device", "zpk_codec_planes_stats", "zpack_amd_write_files_device_planes", "zpack_amd_read_files_device_planes"):
        assert name + "(" in header, name


def test_element_sizes_are_judged_before_any_context():
    """an element size outside {1, 2, 4, 8} is STREAM_INVALID (21) with or without a device: it is checked first, nothing is written"""
    from tests._libs import ZPackAPI, Reader, Writer, File, FileEntry, CompressOptions
    z = ZPackAPI(zpack_amd.ZPACK_SO)
    L = z.lib
    L.zpack_amd_write_files_device_planes.argtypes = [C.POINTER(Writer), C.POINTER(File), C.c_uint64, C.POINTER(C.c_uint8)]
    L.zpack_amd_read_files_device_planes.argtypes = [C.POINTER(Reader), C.POINTER(C.POINTER(FileEntry)), C.c_uint64, C.POINTER(C.c_void_p),
                                                     C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(C.c_int), C.c_void_p]
    w = Writer()
    assert L.zpack_init_writer_heap(C.byref(w), 0) == 0
    try:
        opts = CompressOptions(2, 0)
        arr = (File * 2)()
        for i in range(2):
            arr[i].filename = b"x%d" % i
            arr[i].buffer = None
            arr[i].size = 64
            arr[i].options = C.pointer(opts)
        for bad in (0, 3, 5, 16, 255):
            assert L.zpack_amd_write_files_device_planes(C.byref(w), arr, 2, (C.c_uint8 * 2)(2, bad)) == 21
            assert w.write_offset == 0 and w.file_count == 0 and not w.zstd_cctx
    finally:
        L.zpack_close_writer(C.byref(w))
    r = Reader()
    path = os.path.join(ROOT, "tests", "golden", "ref_workdir", "archive_lz4.zpk")
    assert L.zpack_init_reader(C.byref(r), path.encode()) == 0
    try:
        ents = (C.POINTER(FileEntry) * 2)(C.pointer(r.file_entries[0]), C.pointer(r.file_entries[1]))
        bufs = (C.c_void_p * 2)(None, None)
        caps = (C.c_size_t * 2)(1 << 20, 1 << 20)
        res = (C.c_int * 2)(-7, -7)
        for bad in (0, 3, 6, 9):
            assert L.zpack_amd_read_files_device_planes(C.byref(r), ents, 2, bufs, caps, (C.c_uint8 * 2)(bad, 4), res, None) == 21
            assert list(res) == [-7, -7] and not r.zstd_dctx
    finally:
        L.zpack_close_reader(C.byref(r))
