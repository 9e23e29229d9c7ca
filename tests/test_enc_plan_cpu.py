"""CPU: an entry written in pieces, as zpack_amd/csrc/enc_plan.h decides it for the three writers (the harness compiles the very header the
codec includes) under AddressSanitizer + UBSan.  The plan: sizes 0, 1, PIECE - 1, PIECE, PIECE + 1, 2 PIECE, 3 PIECE + 17, 2 MiB, 2^32 - 1,
2^32, 2^32 + PIECE + 1 for the three methods at split_min 1, 2 MiB and ~0 — split exactly by the rule, the pieces tile their entry, every
capacity the bound of its own size, slots 256-aligned, ascending and disjoint, out_total / max_cap right, ZPK_EF_PIECE on the pieces of
split entries only.  The frame envelope against bytes written out from the two format specifications and through the header parsers of
host_walk.h (the Zstandard header with eight bytes of content size included); the verdict as a table (tools/hostfuzz/enc_plan_main.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
def test_enc_plan_under_asan_ubsan():
    p = subprocess.run(["bash", os.path.join(ROOT, "tools", "hostfuzz", "run_enc_plan.sh")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "plan: 99 entries, 33 split, 147582 pieces: split exactly by the rule" in p.stdout, p.stdout[-1000:]
    assert "envelope: LZ4, Zstandard with 4 and 8 bytes of content size and with none, stored" in p.stdout, p.stdout[-1000:]
    assert "verdict: a frame that fits exactly, one byte less, a failing piece" in p.stdout, p.stdout[-1000:]
