"""CPU: the block walk over ONE large frame in the form k_big_walk runs on the device (walk_lz4_single_into, walk_zstd_single_into in
zpack_amd/csrc/host_walk.h: the same rules as the vector walkers, compiled for both sides, filling a table of fixed capacity) under
AddressSanitizer + UBSan.  Intact frames at the capacities nb - 1, nb and nb + 1, frames of several thousand one-byte blocks, and mutated
frames (flips in frame and block headers, truncation, trailing bytes, longer sizes): the table form accepts exactly what the vector form
accepts and the table holds, the tables are byte-identical, and every table is a heap allocation of exactly `capacity` elements, so a
block written behind it stops the run (tools/hostfuzz/big_walk_main.cpp)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
def test_fixed_capacity_walkers_equal_the_vector_walkers_under_asan_ubsan():
    p = subprocess.run(["bash", os.path.join(ROOT, "tools", "hostfuzz", "run_big_walk.sh"), "40000"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "every other table identical" in p.stdout and "the table form agrees with the vector form" in p.stdout, p.stdout[-1000:]
    m = re.search(r"mutated LZ4 frames \((\d+) accepted\) and \d+ mutated Zstandard frames \((\d+) accepted\)", p.stdout)
    assert m and int(m.group(1)) > 100 and int(m.group(2)) > 100, p.stdout[-1000:]

