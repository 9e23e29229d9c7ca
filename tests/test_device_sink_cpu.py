"""CPU: the writer whose sink is an archive image in DEVICE memory (include/zpack_amd.h: zpack_amd_init_writer_device) as far as a machine
without a GPU can see it.  libzpack_amd.so exports the two calls and zpack_amd.h declares them; libzpk_codec.so exports the codec names
behind them at ABI version 3; NULL arguments are ZPACK_ERROR_STREAM_INVALID (21) and leave the writer untouched; without a HIP device the
init is ZPACK_ERROR_NOT_AVAILABLE (24) — there is no CPU fallback — and the writer stays unopened; zpk_codec_store_device never copies
into host memory.  tests/test_gpu_device_sink.py has the rest."""
import ctypes as C
import os
import re

import pytest

import zpack_amd
from tests._libs import ZPackAPI, Writer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRITER_NOT_OPENED, STREAM_INVALID, NOT_AVAILABLE = 2, 21, 24
ZPK_E_NO_DEVICE, ZPK_E_INVALID = -1, -2
NEW_CODEC_NAMES = ["zpk_codec_store_device", "zpk_codec_encode_batch_dsink", "zpk_codec_dsink_stats", "zpk_codec_stream_sync"]


@pytest.fixture(scope="module")
def Z():
    z = ZPackAPI(zpack_amd.ZPACK_SO)
    z.lib.zpack_amd_init_writer_device.argtypes = [C.POINTER(Writer), C.c_void_p, C.c_size_t]
    z.lib.zpack_amd_writer_device_image.argtypes = [C.POINTER(Writer), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    return z


def _no_device():
    L = zpack_amd.lib()
    L.zpk_codec_device_count.restype = C.c_int
    return L.zpk_codec_device_count() <= 0


def test_the_library_exports_the_two_calls_and_the_header_declares_them(Z):
    hdr = open(os.path.join(ROOT, "include", "zpack_amd.h")).read()
    for name in ("zpack_amd_init_writer_device", "zpack_amd_writer_device_image"):
        assert getattr(Z.lib, name) is not None
        assert re.search(r"ZPACK_EXPORT\s+int\s+%s\s*\(" % name, hdr), name
    assert "zpack_amd_" not in open(os.path.join(ROOT, "include", "zpack.h")).read()    # zpack.h stays the reference's header


def test_the_codec_exports_the_new_names_at_abi_version_3():
    L = zpack_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "zpack_codec.h")).read()
    for name in NEW_CODEC_NAMES:
        assert getattr(L, name) is not None
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert L.zpk_codec_abi_version() == 3
    assert re.search(r"#define\s+ZPK_CODEC_ABI_VERSION\s+3\b", hdr)
    assert hasattr(zpack_amd.Codec, "encode_batch_dsink") and hasattr(zpack_amd.Codec, "dsink_stats")
    from zpack_amd import device_io
    assert callable(device_io.write_archive_device)
    assert device_io.archive_capacity([0, 65536], ["a", "bc"], zpack_amd.METHOD_NONE) == 10 + 65536 + 20 + (35 + 1) + (35 + 2) + 12


def test_null_arguments_are_stream_invalid_and_leave_the_writer_alone(Z):
    w = Writer()
    keep = (C.c_uint8 * 64)()
    assert Z.lib.zpack_amd_init_writer_device(None, C.addressof(keep), 64) == STREAM_INVALID
    assert Z.lib.zpack_amd_init_writer_device(C.byref(w), None, 64) == STREAM_INVALID
    assert bytes(w) == bytes(C.sizeof(Writer))                                        # all zero: no sink, no table, no context
    assert Z.lib.zpack_write_header(C.byref(w)) == WRITER_NOT_OPENED


def test_the_image_of_any_other_writer_is_null(Z):
    p, cap, dev = C.c_void_p(1), C.c_size_t(7), C.c_int(7)
    w = Writer()
    assert Z.lib.zpack_amd_writer_device_image(C.byref(w), C.byref(p), C.byref(cap), C.byref(dev)) == 0          # never opened
    assert (p.value, cap.value, dev.value) == (None, 0, -1)
    assert Z.lib.zpack_init_writer_heap(C.byref(w), 0) == 0
    p, cap, dev = C.c_void_p(1), C.c_size_t(7), C.c_int(7)
    assert Z.lib.zpack_amd_writer_device_image(C.byref(w), C.byref(p), C.byref(cap), C.byref(dev)) == 0          # a heap writer
    assert (p.value, cap.value, dev.value) == (None, 0, -1)
    assert Z.lib.zpack_amd_writer_device_image(C.byref(w), None, None, None) == 0
    Z.lib.zpack_close_writer(C.byref(w))
    assert Z.lib.zpack_amd_writer_device_image(None, C.byref(p), C.byref(cap), C.byref(dev)) == STREAM_INVALID


def test_without_a_device_the_init_is_not_available_and_the_writer_stays_unopened(Z):
    """... and with one, an image in HOST memory is turned down by the pointer check"""
    keep = (C.c_uint8 * 4096)(*([0x5A] * 4096))
    w = Writer()
    want = NOT_AVAILABLE if _no_device() else STREAM_INVALID
    assert Z.lib.zpack_amd_init_writer_device(C.byref(w), C.addressof(keep), 4096) == want                       # never written to
    assert bytes(w) == bytes(C.sizeof(Writer))
    assert Z.lib.zpack_write_header(C.byref(w)) == WRITER_NOT_OPENED
    assert Z.lib.zpack_write_data_header(C.byref(w)) == WRITER_NOT_OPENED
    assert Z.lib.zpack_write_cdr(C.byref(w)) == WRITER_NOT_OPENED
    assert bytes(keep) == b"\x5A" * 4096
    Z.lib.zpack_close_writer(C.byref(w))                                              # closing a writer that was never opened is harmless


def test_store_device_never_copies_into_host_memory():
    L = zpack_amd.lib()
    L.zpk_codec_store_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    src = (C.c_uint8 * 64)(*([0x5A] * 64))
    dst = (C.c_uint8 * 64)(*([0xA5] * 64))
    for args in ((C.addressof(dst), C.addressof(src), 64), (C.addressof(dst), None, 64), (None, C.addressof(src), 64), (C.addressof(dst), C.addressof(src), 1 << 62)):
        assert L.zpk_codec_store_device(*args) in (ZPK_E_INVALID, ZPK_E_NO_DEVICE), args
    assert bytes(dst) == b"\xA5" * 64 and bytes(src) == b"\x5A" * 64
    if _no_device():
        assert L.zpk_codec_store_device(C.addressof(dst), C.addressof(src), 64) == ZPK_E_NO_DEVICE
        assert L.zpk_codec_dsink_stats(None, None) == ZPK_E_INVALID and L.zpk_codec_stream_sync(None) == ZPK_E_INVALID
        placed, nbytes = C.c_uint64(9), C.c_uint64(9)
        L.zpk_codec_encode_batch_dsink.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        assert L.zpk_codec_encode_batch_dsink(None, None, 0, None, 0, None, 0, None, C.byref(placed), C.byref(nbytes)) == ZPK_E_INVALID
