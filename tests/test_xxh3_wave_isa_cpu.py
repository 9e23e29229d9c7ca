"""The XXH3 verify pass at the end of every entry of k_lz4_wave (xxh3_64_wave) takes four 1 KiB blocks per step: one DPP row of
the wave per block, the 16 stripes of a block summed inside the row, and only the four block sums handed across rows.  This test
cross-compiles the codec to gfx950 assembly (no GPU needed) and holds the loop to what that layout is for: fewer vector
instructions per 4 KiB step than the 213 of the loop it replaced (one block spread over the whole wave, a 16-lane reduction per
block), and at most 16 ds_bpermute (4 blocks x 4 dwords; the old loop had 64).  tools/isa_lz4_loops.py hash_loop() does the counting."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    h = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return h if os.path.exists(h) else None


def _tool():
    spec = importlib.util.spec_from_file_location("isa_lz4_loops", os.path.join(ROOT, "tools", "isa_lz4_loops.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("isa") / "zpk_codec.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-function", "--cuda-device-only", "-S",
                           "-o", out, os.path.join(ROOT, "zpack_amd", "csrc", "zpk_codec.hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_hash_loop_of_hot_lz4_kernel(listing):
    h = _tool().hash_loop(listing, "k_lz4_wave")
    print(h)
    assert h["loads"] == 4 and h["mad_u64"] == 24, h          # one step = 4 KiB: four 16-byte loads per lane, 8 + 16 multiplications
    assert h["valu"] < 213, h
    assert h["ds_bpermute"] <= 16, h


def test_hash_loop_keeps_its_prefetch(listing):
    """two loads stay in flight while the other two are consumed: no wait for ALL outstanding loads inside the loop (what a copied
    load register or a guarded load makes the compiler do)"""
    h = _tool().hash_loop(listing, "k_lz4_wave")
    assert h["waitcnt_vm0"] == 0, h
