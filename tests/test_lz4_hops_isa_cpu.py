"""The two hop loops of lz4_walk (lz4_wave.h) carry no boolean round the loop: the exit test is the `and` of two compares' lane masks,
the visit bit is a shifted inline constant, the old-mask test reads the same bit.  Cross-compiled to gfx950 assembly (no GPU needed,
about 40 s) and counted by tools/isa_lz4_loops.py, as tests/test_lz4_lean_isa_cpu.py does.

The limits are the counts of the shipped listing (profiles/r35/r35_isa_static_counts.txt), set against the build with the carried flag
(-DLZ4W_LEAN_HOPS=0: 78 / 79 vector instructions in the first walk / the re-walk with the loop's header block, 75 / 73 without it):

  * with the header block both loops are 3 below that build: 75 and 76.  The instructions that went are mostly the header's (the
    v_cndmask / v_cmp_ne pair that made a lane mask of the flag), so
  * without the header block the loops are 1 and 2 below it: 74 and 71, not the 3 the change was asked to reach under that convention.
    No spelling compiled reached it without scalar-register spills in the batch loop; along the path an iteration runs when no lane
    takes the general decoder the loops execute 22 and 24 vector instructions where they executed 25 and 27.
  * no scalar-register spill in either walk; the batch loop keeps its 633 vector instructions and 42 spill lane accesses; the kernel
    keeps 64 VGPRs, no scratch, at most 5120 bytes of LDS, 8 waves per SIMD."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("isa_lz4_loops", os.path.join(ROOT, "tools", "isa_lz4_loops.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("isa_hops") / "zpk_codec.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-function", "--cuda-device-only", "-S",
                           "-o", out, os.path.join(ROOT, "zpack_amd", "csrc", "zpk_codec.hip")], stderr=subprocess.DEVNULL)
    r = _tool().lz4_loops(open(out).read(), "k_lz4_wave")
    print(r)
    return r


def test_hop_loops_are_below_the_carried_flag_build(counts):
    r = counts
    assert r["hop1"]["valu"] <= 78 - 3 and r["hop2"]["valu"] <= 79 - 3, r
    assert r["hop1"]["valu_sans_header"] <= 74 and r["hop2"]["valu_sans_header"] <= 71, r
    assert r["hop1"]["spill"] == 0 and r["hop2"]["spill"] == 0, r


def test_batch_loop_and_kernel_shape_are_kept(counts):
    r = counts
    assert r["batch"]["valu"] <= 633 and r["batch"]["spill"] <= 42, r
    m = r["meta"]
    assert m["vgprs"] <= 64 and m["scratch"] == 0 and m["lds"] <= 5120, m
    assert m["occupancy"] is None or m["occupancy"] == 8, m
