"""CPU: the bounded steps of the stream reader as zpack_amd/csrc/stream_plan.h states them for dstream_fast_lz4 and dstream_fast_zstd
(the harness compiles the very header the codec includes) under AddressSanitizer + UBSan.  The intake rule and the go rule as tables —
every refusal and every RESTART once next to the last value that passes; whole streams simulated without a GPU over synthetic LZ4 frames
whose block headers are all lz4_stream_blocks reads (full, short and stored blocks; totals of 0, 1, 240, 241, 65535, 65536, 64 x 64 KiB
+- 1 and more; windows of 1 byte to 9 MiB, fixed and random), with the LZ4 constants and with 128 KiB blocks behind histories of 128 KiB,
1 MiB and 15 MiB for the Zstandard ones: every block in exactly one step and in order, every 64 KiB group handed to the partial sums once
and to the chain once, the finish once and last, the one-launch hash exactly when the entry ends in its first step, every position the
hash reads inside the device window, the partial sums inside their region, the last min(have, cap) bytes kept as history, the pending
bytes bounded; the two device layouts (tools/hostfuzz/stream_plan_main.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKED = ("every block in one step, every group summed and chained once, the finish once and last, every read inside the window; "
           "pending <= a step + the window in %d streams")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
def test_stream_plan_under_asan_ubsan():
    p = subprocess.run(["bash", os.path.join(ROOT, "tools", "hostfuzz", "run_stream_plan.sh")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "intake: 11 rows, 3 refused (21 below what was taken, 10 above 2^46), never more than the entry has; the pending buffer grows by need + 1 MiB" in p.stdout, p.stdout[-2000:]
    assert "go: 24 rows, 8 run, 7 wait, 9 RESTART: exactly by the rule; LZ4 64 / 4, Zstandard 64 / 2; verdict 0 or 15" in p.stdout, p.stdout[-2000:]
    for name, counts, stated in (("streams lz4", "510 streams, 486526 calls, 999 steps, 240 ended in the first step, 489 carries", 176),
                                 ("streams zstd window 128 KiB", "510 streams, 456080 calls, 939 steps, 283 ended in the first step, 425 carries", 175),
                                 ("streams zstd window 1024 KiB", "478 streams, 400357 calls, 742 steps, 282 ended in the first step, 159 carries", 176),
                                 ("streams zstd window 15360 KiB", "478 streams, 436775 calls, 746 steps, 282 ended in the first step, 19 carries", 172)):
        assert "%s: %s: %s" % (name, counts, CHECKED % stated) in p.stdout, (name, p.stdout[-3000:])
    assert ("layout: LZ4 13 regions, 37957120 bytes as recorded; Zstandard 96 shapes: 12 scratch regions 256-aligned, 7 persistent ones 64-aligned, "
            "all ascending and disjoint, totals the end of the last region") in p.stdout, p.stdout[-2000:]
