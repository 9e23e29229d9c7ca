"""The base check without a GPU: zpack_amd/csrc/span_hash_plan.h — which device spans one wave hashes and which the whole chip, the
partial-sum layout, the launches — walked under ASan + UBSan the way the kernels walk it (tools/hostfuzz/span_hash_plan_main.cpp) and
pinned at the threshold; the new symbols of both libraries and what the calls answer before they need a device; and the torch view's
manifest: "base_xxh3" written, read back, absent in an older archive, refused when malformed."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

import zpack_amd
from zpack_amd import device_io
from tests._libs import ZPackAPI, Reader, FileEntry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tools", "hostfuzz", "run_span_hash_plan.sh")
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
STREAM_INVALID, NOT_AVAILABLE = 21, 24


def _no_device():
    lib = zpack_amd.lib()
    lib.zpk_codec_device_count.restype = C.c_int
    return lib.zpk_codec_device_count() <= 0


# ------------------------------------------------------------------------------------------------ the plan

@needs_gxx
def test_span_hash_plan_under_asan_ubsan():
    p = subprocess.run(["bash", SCRIPT], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert ("span hash plan: 4225 rows in 32705280 bytes (3910 one wave, 315 chip-wide in 504 groups, 371 launches): every byte in front of the last "
            "stripe loaded once, the last stripe closes the row, no load leaves a row, one slot of partial sums per block and row, every split "
            "reaches each row and group once") in p.stdout, p.stdout
    assert "FAILED" not in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


@needs_gxx
def test_the_compiled_plan_at_the_threshold_the_partial_sum_bases_and_a_small_group_limit():
    """a threshold of 4 KiB and at most 4 groups per launch.  The rows of the mixed call: 4096 (3 full blocks in front of the last byte's:
    one group), 300, 4096 + 65536 (67 blocks: two groups), 0, 4096 + 1025 (5 blocks: one), 240, 65 * 65536 + 1 (4160 blocks: 65 groups)."""
    p = subprocess.run(["bash", SCRIPT, "--pin", "4096", "4"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    out = p.stdout.split("\n")
    assert "pin split: len 4095 threshold 4096 -> one wave" in out                      # threshold - 1, threshold, threshold + 1
    assert "pin split: len 4096 threshold 4096 -> chip-wide" in out
    assert "pin split: len 4097 threshold 4096 -> chip-wide" in out
    assert "pin split: len 1024 threshold 1 -> one wave; len 1025 threshold 1 -> chip-wide; len 1099511627776 threshold never -> one wave" in out
    assert "pin rows: W0 w0 W1 w1 W2 w2 W3" in out                                      # each table in the order given
    assert "pin part_base: 0 64 192 256 | part_blocks 4416 groups 69 nwave 3 nwide 4" in out      # multiples of 64, ascending; 64 + 128 + 64 + 4160 slots
    launches = [l for l in out if l.startswith("pin launches of 69 groups at a limit of 4:")]
    assert len(launches) == 1
    cuts = re.findall(r"\[(\d+),\+(\d+)\) grid (\d+)", launches[0])
    assert len(cuts) == 18 and [int(a) for a, _, _ in cuts] == list(range(0, 72, 4))    # 17 launches of 4 groups and one of 1, one workgroup each
    assert [int(b) for _, b, _ in cuts] == [4] * 17 + [1] and all(int(g) == 1 for _, _, g in cuts)
    assert "pin launches at the grid limit: 1, [0,+69) grid 18" in out                  # four groups per workgroup
    # the same split at the default threshold, which is the stored spans' (256 KiB)
    p = subprocess.run(["bash", SCRIPT, "--pin", str(256 << 10), "4"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "pin split: len 262143 threshold 262144 -> one wave" in p.stdout and "pin split: len 262144 threshold 262144 -> chip-wide" in p.stdout


# ------------------------------------------------------------------------------------------------ the libraries

def test_both_libraries_export_the_new_calls_and_the_headers_declare_them():
    codec = C.CDLL(zpack_amd.CODEC_SO)
    codec_names = ("zpk_codec_hash_spans_device", "zpk_codec_decode_batch_host_dptr_delta_checked", "zpk_codec_decode_batch_dimage_delta_checked",
                   "zpk_codec_base_check_stats")
    for name in codec_names:
        assert hasattr(codec, name), name
    lib = C.CDLL(zpack_amd.ZPACK_SO)
    lib_names = ("zpack_amd_hash_device", "zpack_amd_read_files_device_delta_checked")
    for name in lib_names:
        assert hasattr(lib, name), name
    codec_h = open(os.path.join(ROOT, "include", "zpack_codec.h")).read()
    for name in codec_names:
        assert re.search(r"\bint\s+%s\s*\(" % name, codec_h), name
    assert "typedef struct zpk_hash_span { uint64_t addr, len; } zpk_hash_span;" in codec_h
    assert re.search(r"#define\s+ZPK_CODEC_ABI_VERSION\s+3\b", codec_h)                 # additive: the ABI version stays
    assert re.search(r"#define\s+ZPK_OPT_SPAN_HASH_MIN\s+12\b", codec_h) and zpack_amd.OPT_SPAN_HASH_MIN == 12
    amd_h = open(os.path.join(ROOT, "include", "zpack_amd.h")).read()
    for name in lib_names:
        assert re.search(r"ZPACK_EXPORT\s+int\s+%s\s*\(" % name, amd_h), name
    # the new status: one value in both headers and in both Python views, outside enum zpack_result (0 .. 24), which zpack.h keeps
    m = re.search(r"#define\s+ZPACK_AMD_ERROR_BASE_MISMATCH\s+(\d+)", amd_h)
    k = re.search(r"#define\s+ZPK_R_BASE_MISMATCH\s+(\d+)", codec_h)
    assert m and k and int(m.group(1)) == int(k.group(1)) == zpack_amd.R_BASE_MISMATCH == device_io.BASE_MISMATCH and int(m.group(1)) > 24
    zpack_h = open(os.path.join(ROOT, "include", "zpack.h")).read()
    assert "BASE_MISMATCH" not in zpack_h and "zpack_amd_" not in zpack_h and len(re.findall(r"^ZPACK_EXPORT\b", zpack_h, flags=re.M)) == 54
    assert re.search(r"ZPACK_ERROR_FILENAME_TOO_LONG,\s*ZPACK_ERROR_NOT_AVAILABLE\s*\};", zpack_h)             # ... whose last value is 24
    assert zpack_amd.HASH_SPAN.itemsize == 16 and zpack_amd.HASH_SPAN.names == ("addr", "len")
    assert callable(zpack_amd.Codec.hash_spans_device) and callable(zpack_amd.Codec.base_check_stats) and callable(device_io.hash_tensors)


def test_null_arrays_are_stream_invalid_and_no_device_is_not_available():
    lib = ZPackAPI(zpack_amd.ZPACK_SO).lib
    u64, vp = C.c_uint64, C.c_void_p
    lib.zpack_amd_hash_device.argtypes = [C.POINTER(vp), C.POINTER(C.c_size_t), u64, C.POINTER(u64), vp]
    lib.zpack_amd_read_files_device_delta_checked.argtypes = [C.POINTER(Reader), C.POINTER(C.POINTER(FileEntry)), u64, C.POINTER(vp), C.POINTER(C.c_size_t),
                                                              C.POINTER(C.c_uint8), C.POINTER(vp), C.POINTER(u64), C.POINTER(C.c_int), vp]
    ptrs, sizes, out = (vp * 2)(None, None), (C.c_size_t * 2)(0, 0), (u64 * 2)(7, 7)
    assert lib.zpack_amd_hash_device(None, sizes, 2, out, None) == STREAM_INVALID
    assert lib.zpack_amd_hash_device(ptrs, None, 2, out, None) == STREAM_INVALID
    assert lib.zpack_amd_hash_device(ptrs, sizes, 2, None, None) == STREAM_INVALID
    assert list(out) == [7, 7]
    r = Reader()
    path = os.path.join(ROOT, "tests", "golden", "ref_workdir", "archive_lz4.zpk")
    assert lib.zpack_init_reader(C.byref(r), path.encode()) == 0 and r.file_count == 2
    try:
        ents = (C.POINTER(FileEntry) * 2)(C.pointer(r.file_entries[0]), C.pointer(r.file_entries[1]))
        bufs, caps, bases = (vp * 2)(None, None), (C.c_size_t * 2)(1 << 20, 1 << 20), (vp * 2)(None, None)
        want, res = (u64 * 2)(1, 2), (C.c_int * 2)(-7, -7)
        rd = lib.zpack_amd_read_files_device_delta_checked
        assert rd(None, ents, 2, bufs, caps, None, bases, want, res, None) == STREAM_INVALID
        assert rd(C.byref(r), None, 2, bufs, caps, None, bases, want, res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, None, caps, None, bases, want, res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, bufs, None, None, bases, want, res, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, bufs, caps, None, bases, want, None, None) == STREAM_INVALID
        assert rd(C.byref(r), ents, 2, bufs, caps, (C.c_uint8 * 2)(3, 4), bases, want, res, None) == STREAM_INVALID
        assert list(res) == [-7, -7] and not r.zstd_dctx                                # judged first: no context, no result
        if _no_device():
            assert rd(C.byref(r), ents, 2, bufs, caps, None, bases, want, res, None) == NOT_AVAILABLE
            assert rd(C.byref(r), ents, 2, bufs, caps, None, bases, None, res, None) == NOT_AVAILABLE
            assert lib.zpack_amd_hash_device(ptrs, sizes, 2, out, None) == NOT_AVAILABLE
            assert list(res) == [-7, -7] and list(out) == [7, 7]
    finally:
        lib.zpack_close_reader(C.byref(r))


# ------------------------------------------------------------------------------------------------ the torch view's manifest

HEX = {"a": "%016x" % 0x0123456789ABCDEF, "b": "%016x" % 5}


def test_the_manifest_round_trips_base_xxh3_and_an_older_one_is_accepted():
    new = {"entries": ["a", "b"], "base_id": "step 7", "base_xxh3": HEX}
    assert device_io._delta_manifest_valid(new)
    assert device_io._parse_delta_manifest(json.loads(json.dumps(new))) == (["a", "b"], "step 7", {"a": 0x0123456789ABCDEF, "b": 5})
    old = {"entries": ["a", "b"], "base_id": None}                                      # as written before the bases were hashed: read as ever, no check
    assert device_io._delta_manifest_valid(old) and device_io._parse_delta_manifest(old) == (["a", "b"], None, None)
    assert device_io._parse_delta_manifest(None) == ([], None, None)                    # no manifest at all
    assert device_io._delta_manifest_valid({"entries": [], "base_id": None, "base_xxh3": {}})


@pytest.mark.parametrize("field", [
    pytest.param(["0" * 16, "1" * 16], id="a-list"),
    pytest.param({"a": HEX["a"]}, id="a-name-missing"),
    pytest.param(dict(HEX, c="0" * 16), id="a-name-too-many"),
    pytest.param(dict(HEX, b="5"), id="too-short"),
    pytest.param(dict(HEX, b="0" * 17), id="too-long"),
    pytest.param(dict(HEX, b="000000000000000G"), id="not-hex"),
    pytest.param(dict(HEX, b="000000000000000A"), id="upper-case"),
    pytest.param(dict(HEX, b=5), id="a-number"),
    pytest.param(None, id="null"),
])
def test_a_malformed_base_xxh3_is_refused(field):
    assert not device_io._delta_manifest_valid({"entries": ["a", "b"], "base_id": "step 7", "base_xxh3": field})


def test_a_malformed_manifest_raises_from_the_reader_like_any_malformed_manifest():
    """_read_json_entry is what turns an invalid value into the ValueError read_files_device raises; driven here through a stand-in
    reader whose one entry holds the JSON (no device: the host read is replaced)"""
    def read_manifest(value):
        text = json.dumps(value).encode()

        class FakeLib:
            @staticmethod
            def zpack_read_file(_r, _e, raw, size, _ctx):
                C.memmove(raw, text, size)
                return 0

        table = (device_io.FileEntry * 1)(device_io.FileEntry(device_io.DELTA_MANIFEST.encode(), 0, len(text), len(text), 0, 0))
        r = device_io.Reader()
        r.file_count, r.file_entries = 1, table
        return device_io._read_delta_manifest(FakeLib, r)

    with pytest.raises(ValueError, match="delta.json does not parse"):
        read_manifest({"entries": ["a"], "base_id": None, "base_xxh3": {"a": "xyz"}})
    with pytest.raises(ValueError, match="delta.json does not parse"):
        read_manifest({"entries": ["a"], "base_id": None, "base_xxh3": {}})
    assert read_manifest({"entries": ["a"], "base_id": None, "base_xxh3": {"a": "0" * 15 + "7"}}) == (["a"], None, {"a": 7})
    assert read_manifest({"entries": ["a"], "base_id": "s"}) == (["a"], "s", None)
