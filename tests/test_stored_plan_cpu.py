"""CPU: the large stored entries of a device-resident call, as zpack_amd/csrc/stored_plan.h decides them for zpk_codec_decode_big_batch_device
and zpk_codec_decode_big_device (the harness compiles the very header the codec includes) under AddressSanitizer + UBSan.  The rule over
the lengths 1024, 1025, 2048, 2049, 65536, 65537, 66560, 66561, 2^32 - 1, 2^32 + 1025 and six thresholds, every guard failed once next
to the last value that passes it; the span table — rows and destination offsets as given, part_base ascending in multiples of 64 and
disjoint, the group count, a launch that is full; the verdict as a table (tools/hostfuzz/stored_plan_main.cpp)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
def test_stored_plan_under_asan_ubsan():
    p = subprocess.run(["bash", os.path.join(ROOT, "tools", "hostfuzz", "run_stored_plan.sh")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "rule: 33 of 60 entries taken over the lengths and thresholds, 8 guards failed once each: exactly by the rule" in p.stdout, p.stdout[-1000:]
    assert "table: 9 spans, 131081 groups: rows and destination offsets as given, part_base ascending in multiples of 64 and disjoint" in p.stdout, p.stdout[-1000:]
    assert "full: an entry whose groups do not fit the launch is left out" in p.stdout, p.stdout[-1000:]
    assert "verdict: OK, hash mismatch, hash mismatch skipped" in p.stdout, p.stdout[-1000:]


def test_stored_span_option_number_of_the_python_view_matches_the_header():
    import zpack_amd
    hdr = open(os.path.join(ROOT, "include", "zpack_codec.h")).read()
    m = re.search(r"#define\s+ZPK_OPT_STORED_SPAN_MIN\s+(\d+)", hdr)
    assert m and int(m.group(1)) == zpack_amd.OPT_STORED_SPAN_MIN == 10
    others = {int(x) for x in re.findall(r"ZPK_OPT_[A-Z0-9_]+\s*=\s*(\d+)", hdr)}
    assert zpack_amd.OPT_STORED_SPAN_MIN not in others
    assert re.search(r"#define\s+ZPK_CODEC_ABI_VERSION\s+3\b", hdr)
