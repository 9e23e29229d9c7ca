"""CPU: the verdict-only read (include/zpack_amd.h: zpack_amd_test_files; include/zpack_codec.h: zpk_codec_verify_batch_host, _dimage,
zpk_codec_verify_stats) as far as a machine without a GPU can see it.  Both libraries export the names and the headers declare them, at ABI
version 3 with the pinned sets unchanged; NULL arguments are ZPACK_ERROR_STREAM_INVALID (21) before any context exists; an empty batch is
ZPACK_OK; without a HIP device the call is ZPACK_ERROR_NOT_AVAILABLE (24) on the three archives of the reference: there is no CPU
fallback.  tests/test_gpu_verify.py has the rest."""
import ctypes as C
import os
import re

import pytest

import zpack_amd
from tests._libs import ZPackAPI, Reader, FileEntry, u8p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, STREAM_INVALID, NOT_AVAILABLE = 0, 21, 24
ZPK_E_INVALID = -2
PFE = C.POINTER(FileEntry)
CODEC_NAMES = ["zpk_codec_verify_batch_host", "zpk_codec_verify_batch_dimage", "zpk_codec_verify_stats"]


@pytest.fixture(scope="module")
def Z():
    z = ZPackAPI(zpack_amd.ZPACK_SO)
    z.lib.zpack_amd_test_files.argtypes = [C.POINTER(Reader), C.POINTER(PFE), C.c_uint64, C.POINTER(C.c_int), C.c_void_p]
    return z


def _no_device():
    L = zpack_amd.lib()
    L.zpk_codec_device_count.restype = C.c_int
    return L.zpk_codec_device_count() <= 0


def test_both_libraries_export_the_names_and_the_headers_declare_them(Z):
    hdr = open(os.path.join(ROOT, "include", "zpack_amd.h")).read()
    assert Z.lib.zpack_amd_test_files is not None
    assert re.search(r"ZPACK_EXPORT\s+int\s+zpack_amd_test_files\s*\(", hdr)
    assert "zpack_amd_" not in open(os.path.join(ROOT, "include", "zpack.h")).read()    # zpack.h stays the reference's header
    L = zpack_amd.lib()
    chdr = open(os.path.join(ROOT, "include", "zpack_codec.h")).read()
    for name in CODEC_NAMES:
        assert getattr(L, name) is not None
        assert re.search(r"\bint\s+%s\s*\(" % name, chdr), name
    assert L.zpk_codec_abi_version() == 3 and re.search(r"#define\s+ZPK_CODEC_ABI_VERSION\s+3\b", chdr)
    assert re.search(r"ZPK_DS2_COUNT\s*=\s*16\b", chdr)                                # decode_stats2 keeps its 16 words
    for name in ("verify_batch_host", "verify_batch_dimage", "verify_stats"):
        assert hasattr(zpack_amd.Codec, name)
    from zpack_amd import device_io
    assert callable(device_io.test_files)


def test_null_arguments_are_stream_invalid_before_any_context_exists(Z, golden_dir):
    arc = open(os.path.join(golden_dir, "ref_workdir", "archive_lz4.zpk"), "rb").read()
    rc, r, keep = Z.open_memory(arc)
    assert rc == OK and r.file_count == 2
    ents = (PFE * 2)(C.pointer(r.file_entries[0]), C.pointer(r.file_entries[1]))
    res = (C.c_int * 2)(-7, -7)
    before = int(r.last_return)
    assert Z.lib.zpack_amd_test_files(None, ents, 2, res, None) == STREAM_INVALID
    assert Z.lib.zpack_amd_test_files(C.byref(r), None, 2, res, None) == STREAM_INVALID
    assert Z.lib.zpack_amd_test_files(C.byref(r), ents, 2, None, None) == STREAM_INVALID
    assert not r.zstd_dctx and list(res) == [-7, -7] and int(r.last_return) == before  # no context was made, nothing was set
    Z.close_reader(r)
    L = zpack_amd.lib()
    for name in CODEC_NAMES[:2]:
        assert getattr(L, name)(None, None, C.c_uint64(0), None, C.c_uint64(1), None) == ZPK_E_INVALID
    assert L.zpk_codec_verify_stats(None, None) == ZPK_E_INVALID


def test_an_empty_batch_is_ok(Z, golden_dir):
    arc = open(os.path.join(golden_dir, "ref_workdir", "archive_zstd.zpk"), "rb").read()
    rc, r, keep = Z.open_memory(arc)
    assert rc == OK
    assert Z.lib.zpack_amd_test_files(C.byref(r), None, 0, None, None) == OK          # (no array is looked at, no context is made)
    assert not r.zstd_dctx
    Z.close_reader(r)
    empty = Reader()
    assert Z.lib.zpack_amd_test_files(C.byref(empty), None, 0, None, None) == OK


@pytest.mark.skipif(not _no_device(), reason="needs a machine WITHOUT a GPU")
@pytest.mark.parametrize("name", ["archive_none.zpk", "archive_zstd.zpk", "archive_lz4.zpk"])
def test_without_a_device_the_call_is_not_available(Z, golden_dir, name):
    arc = open(os.path.join(golden_dir, "ref_workdir", name), "rb").read()
    rc, r, keep = Z.open_memory(arc)
    assert rc == OK and r.file_count == 2
    ents = (PFE * 2)(C.pointer(r.file_entries[0]), C.pointer(r.file_entries[1]))
    res = (C.c_int * 2)(-7, -7)
    assert Z.lib.zpack_amd_test_files(C.byref(r), ents, 2, res, None) == NOT_AVAILABLE          # never a verdict from the CPU
    assert list(res) == [-7, -7]
    Z.close_reader(r)
    rf = Reader()
    path = os.path.join(golden_dir, "ref_workdir", name)
    assert Z.lib.zpack_init_reader(C.byref(rf), path.encode()) == OK
    ents = (PFE * 2)(C.pointer(rf.file_entries[0]), C.pointer(rf.file_entries[1]))
    assert Z.lib.zpack_amd_test_files(C.byref(rf), ents, 2, res, None) == NOT_AVAILABLE and list(res) == [-7, -7]
    Z.close_reader(rf)
