"""CPU: a large entry's route on the read side, as zpack_amd/csrc/dec_plan.h decides it for zpk_codec_decode_batch_host,
zpk_codec_decode_big_device and zpk_codec_decode_big_batch_device (the harness compiles the very header the codec includes) under
AddressSanitizer + UBSan.  The candidate rule as a table — every guard of lib/zpack_read.c:328-331 failed once next to the last value that
passes it, the three methods and unknown ones, the window [split_min, 4 GiB], the option off, the slot test of the device forms — and its
agreement with stored_span_takes for stored entries; the chooser over 47 batches against the decisions recorded from the pj_choose it
replaced, order included; the staging layout of k_big_walk; the hash verdict as a table (tools/hostfuzz/dec_plan_main.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
def test_dec_plan_under_asan_ubsan():
    p = subprocess.run(["bash", os.path.join(ROOT, "tools", "hostfuzz", "run_dec_plan.sh")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "rule: 81 rows, 39 candidates of the host form, 42 not: exactly by the rule, the device forms and stored_span_takes agree" in p.stdout, p.stdout[-1000:]
    assert "choose: 47 batches, 846 candidates, 394 kept: every batch as recorded, order included" in p.stdout, p.stdout[-1000:]
    assert "layout: 12 candidates: tables 16-aligned, ascending and disjoint, capacities those of the walkers, total the end of the last table; none: no walk" in p.stdout, p.stdout[-1000:]
    assert "verdict: OK, hash mismatch, hash mismatch skipped; detail 0, produced = uncomp_size, the hash as computed" in p.stdout, p.stdout[-1000:]
