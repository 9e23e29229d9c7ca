"""CPU: the reader over an archive image in DEVICE memory (include/zpack_amd.h: zpack_amd_init_reader_device) as far as a machine without a
GPU can see it.  libzpack_amd.so exports the two calls and zpack_amd.h declares them; libzpk_codec.so exports the four codec names behind
them at ABI version 3; NULL arguments are ZPACK_ERROR_STREAM_INVALID (21) and leave the reader untouched; without a HIP device the init is
ZPACK_ERROR_NOT_AVAILABLE (24): there is no CPU fallback; zpk_codec_fetch_device never copies from host memory.
zpack_amd/csrc/dimage_plan.h — the sub-batches of such a read and their staging slots: the very header the codec compiles — runs under
AddressSanitizer + UBSan (tools/hostfuzz/dimage_plan_main.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import zpack_amd
from tests._libs import ZPackAPI, Reader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_INVALID, NOT_AVAILABLE = 21, 24
ZPK_E_NO_DEVICE, ZPK_E_INVALID = -1, -2
NEW_CODEC_NAMES = ["zpk_codec_fetch_device", "zpk_codec_decode_batch_dimage", "zpk_codec_dimage_stats"]


@pytest.fixture(scope="module")
def Z():
    z = ZPackAPI(zpack_amd.ZPACK_SO)
    z.lib.zpack_amd_init_reader_device.argtypes = [C.POINTER(Reader), C.c_void_p, C.c_size_t]
    z.lib.zpack_amd_reader_device_image.argtypes = [C.POINTER(Reader), C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    return z


def _no_device():
    L = zpack_amd.lib()
    L.zpk_codec_device_count.restype = C.c_int
    return L.zpk_codec_device_count() <= 0


def test_the_library_exports_the_two_calls_and_the_header_declares_them(Z):
    hdr = open(os.path.join(ROOT, "include", "zpack_amd.h")).read()
    for name in ("zpack_amd_init_reader_device", "zpack_amd_reader_device_image"):
        assert getattr(Z.lib, name) is not None
        assert re.search(r"ZPACK_EXPORT\s+int\s+%s\s*\(" % name, hdr), name
    assert "zpack_amd_" not in open(os.path.join(ROOT, "include", "zpack.h")).read()    # zpack.h stays the reference's header


def test_the_codec_exports_the_four_new_names_at_abi_version_3():
    L = zpack_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "zpack_codec.h")).read()
    for name in NEW_CODEC_NAMES:
        assert getattr(L, name) is not None
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert re.search(r"#define\s+ZPK_OPT_DIMAGE_CHUNK\s+11\b", hdr) and zpack_amd.OPT_DIMAGE_CHUNK == 11
    assert L.zpk_codec_abi_version() == 3
    assert re.search(r"#define\s+ZPK_CODEC_ABI_VERSION\s+3\b", hdr)
    assert hasattr(zpack_amd.Codec, "decode_batch_dimage") and hasattr(zpack_amd.Codec, "dimage_stats")


def test_null_arguments_are_stream_invalid_and_leave_the_reader_alone(Z):
    r = Reader()
    keep = (C.c_uint8 * 64)()
    assert Z.lib.zpack_amd_init_reader_device(None, C.addressof(keep), 64) == STREAM_INVALID
    assert Z.lib.zpack_amd_init_reader_device(C.byref(r), None, 64) == STREAM_INVALID
    assert bytes(r) == bytes(C.sizeof(Reader))                                        # all zero: no size, no table, no context
    p, dev = C.c_void_p(1), C.c_int(7)
    assert Z.lib.zpack_amd_reader_device_image(C.byref(r), C.byref(p), C.byref(dev)) == 0
    assert p.value is None and dev.value == -1                                        # not a reader over a device image
    assert Z.lib.zpack_amd_reader_device_image(None, C.byref(p), C.byref(dev)) == STREAM_INVALID


def test_without_a_device_the_init_is_not_available(Z, golden_dir):
    """... and with one, an image in HOST memory is turned down by the pointer check (tests/test_gpu_device_image.py has the rest)"""
    arc = open(os.path.join(golden_dir, "ref_workdir", "archive_lz4.zpk"), "rb").read()
    keep = (C.c_uint8 * len(arc)).from_buffer_copy(arc)
    r = Reader()
    want = NOT_AVAILABLE if _no_device() else STREAM_INVALID
    assert Z.lib.zpack_amd_init_reader_device(C.byref(r), C.addressof(keep), len(arc)) == want               # never dereferenced
    assert bytes(r) == bytes(C.sizeof(Reader))
    out = (C.c_uint8 * 16)()
    e = (C.c_uint8 * 48)()
    Z.lib.zpack_read_raw_file.argtypes = [C.POINTER(Reader), C.c_void_p, C.c_void_p, C.c_size_t]
    assert Z.lib.zpack_read_raw_file(C.byref(r), C.addressof(e), C.addressof(out), 0) == 1        # ZPACK_ERROR_ARCHIVE_NOT_LOADED: nothing was opened


def test_fetch_device_never_copies_from_host_memory():
    L = zpack_amd.lib()
    L.zpk_codec_fetch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    src = (C.c_uint8 * 64)(*([0x5A] * 64))
    dst = (C.c_uint8 * 64)(*([0xA5] * 64))
    for args in ((C.addressof(src), C.addressof(dst), 64), (C.addressof(src), None, 64), (None, C.addressof(dst), 64), (C.addressof(src), C.addressof(dst), 1 << 62)):
        assert L.zpk_codec_fetch_device(*args) in (ZPK_E_INVALID, ZPK_E_NO_DEVICE), args
    assert bytes(dst) == b"\xA5" * 64 and bytes(src) == b"\x5A" * 64
    if _no_device():
        assert L.zpk_codec_fetch_device(C.addressof(src), C.addressof(dst), 64) == ZPK_E_NO_DEVICE
        assert L.zpk_codec_dimage_stats(None, None) == ZPK_E_INVALID


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
def test_dimage_plan_under_asan_ubsan():
    p = subprocess.run(["bash", os.path.join(ROOT, "tools", "hostfuzz", "run_dimage_plan.sh")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    for line in ("slots: capacities 0, 1, 255, 256, 257, 65536, 307200 take 0, 256, 256, 256, 512, 65536, 307200 bytes of staging",
                 "cuts: at a chunk of 65536 they are 3 sub-batches of 5, 1, 1 entries and 1280, 65536, 307200 bytes",
                 "cuts: at a chunk of 1048576 they are 1 of 7 entries and 374016 bytes, at the default of 4294967296 bytes 1 of 7 entries and 374016 bytes",
                 "alone: a slot of 17920000 bytes at a chunk of 65536 is a sub-batch of its own between its neighbours (1, 1, 3, 1 entries)",
                 "empty: a batch of no entries is no sub-batch; 1000 entries without bytes are one, at 300 entries a sub-batch 4",
                 "wrap: capacities within 255 bytes of 2^64 take the largest slot, 18446744073709551360; slots of that size and of 2^63 never share a sub-batch whose sum would wrap",
                 "random: 2000 batches at 9 chunks each,"):
        assert line in p.stdout, p.stdout[-1500:]
