"""CPU: the decisions of the host-pointer read path (zpk_codec_decode_batch_host, its _dptr forms, zpk_codec_verify_batch_host), as
zpack_amd/csrc/host_plan.h states them (the harness compiles the very header the codec includes) under AddressSanitizer + UBSan.  Each
function against the loop it replaced, copied into the harness as it stood, over random batches below 2^62 with no case skipped — the
cut and what a sub-batch holds, the gathered image, the pieces of the pipeline, the shares of the staged copies, the groups of
frame-parallel entries — and against properties that hold without a model: sub-batches partition the batch at multiples of 256, a
saturated slot goes alone and is refused, gathered payloads are disjoint and alone pass the offset guard, pieces partition entries and
output with none below its minimum and each of the five refusals reached, every byte of every entry is moved exactly once by 1 and by
4 threads, frames lie inside their entries; the small rules as tables, the short-decode rule over every status value of
tests/golden/status_cases.json (tools/hostfuzz/host_plan_main.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
def test_host_plan_under_asan_ubsan():
    p = subprocess.run(["bash", os.path.join(ROOT, "tools", "hostfuzz", "run_host_plan.sh")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "cut: 3000 batches, 114899 sub-batches as the earlier loop cut them, 0 skipped; they partition the batch, slots at multiples of 256, " \
           "only a single entry exceeds its chunk; a saturated slot goes alone and is refused" in p.stdout, p.stdout[-2000:]
    assert "image: 5377 sub-batches sparse; every gathered layout as the earlier block" in p.stdout, p.stdout[-2000:]
    assert "pieces: 160 sub-batches as the earlier loop, 69 taken" in p.stdout and "5 refusals reached" in p.stdout, p.stdout[-2000:]
    assert "shares: 22 ranges, 5569 moves as the earlier lambda; with 1 and 4 threads every byte of every entry moved once, none outside" in p.stdout, p.stdout[-2000:]
    assert "groups: 1500 batches, 7739 groups as the earlier loops, 2714 over the source alone" in p.stdout, p.stdout[-2000:]
    assert "rules: sat_add, host_delivered, host_deliver_dense as tables; host_short_decode over 8 golden status values: 0 and 15 alone" in p.stdout, p.stdout[-2000:]
