"""CPU: the types that own the codec's HIP resources — device buffers, pinned blocks, events, streams (zpack_amd/csrc/codec_res.h, the very
header the codec compiles) — under a stand-alone driver (tools/hostfuzz/codec_res_main.cpp) built with AddressSanitizer + UBSan against a
counting stand-in for the HIP runtime (tools/hostfuzz/fakehip): nothing stays alive, nothing is freed twice, a refused creation leaves an
empty object and the last error where the codec expects it."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "tools", "hostfuzz", "run_codec_res.sh")
CSRC = os.path.join(ROOT, "zpack_amd", "csrc")


def test_owning_types_under_asan_ubsan():
    p = subprocess.run(["bash", RUN], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = p.stdout.strip().split("\n")
    m = re.fullmatch(r"full: (\d+) creating calls, every type created, used, regrown and destroyed, nothing alive at the end", lines[0])
    assert m and int(m.group(1)) >= 14, lines[0]                  # (14 objects are created in a run, some more than once)
    assert lines[1] == ("failing: the creation refused at each of the calls 1..%s in turn: the object empty, the error cleared by the buffers "
                        "and left by the others, the rest destroyed cleanly" % m.group(1)), lines[1]
    assert lines[2:] == ["untouched: default-constructed objects are destroyed without one call",
                         "twice: ready() and ensure() a second time create nothing and keep what the first made",
                         "ok"], p.stdout[-1500:]
    assert "FAILED" not in p.stdout and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-2000:]


def test_resources_are_created_and_released_by_the_owning_types_only():
    calls = re.compile(r"\b(hipFree|hipHostFree|hipEventDestroy|hipStreamDestroy|hipMalloc|hipHostMalloc|hipEventCreate(?:WithFlags)?|"
                       r"hipStreamCreate(?:WithFlags|WithPriority)?)\s*\(")
    text = re.compile(r'"(?:[^"\\]|\\.)*"|//.*')                # (an error message or a comment may name a call)
    gone = re.compile(r"\bzstd_hint\b|\blz4_hint\b|\bbufs\[|\bpins\[")
    for name in sorted(os.listdir(CSRC)):
        src = open(os.path.join(CSRC, name)).read()
        assert not gone.search(src), name
        if name != "codec_res.h":
            found = [m.group(1) for line in src.split("\n") for m in calls.finditer(text.sub("", line))]
            assert not found, (name, found)


def test_code_object_report_of_the_built_library_against_itself():
    """tools/code_objects.py, the recipe behind profiles/r25/r25_code_objects.md: the library build() made has one gfx950 code object per
    .hip file, each with kernels, and compares identical to itself"""
    so = os.path.join(ROOT, "zpack_amd", "libzpk_codec.so")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "code_objects.py"), so, so, "--names", "zpk_codec.hip", "row_copy.hip", "sink_commit.hip"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-1500:])
    rows = [l for l in p.stdout.split("\n") if l.startswith("| ") and ".hip |" in l]
    assert [r.split("|")[1].strip() for r in rows] == ["zpk_codec.hip", "row_copy.hip", "sink_commit.hip"], p.stdout[:1500]
    for r in rows:
        f = [x.strip() for x in r.split("|")]
        assert int(f[2]) > 0 and f[3] == f[4] and int(f[5]) > 0 and f[6] == f[7], r
    for k in ("k_lz4_wave", "k_span_copy", "k_sink_place"):
        assert k in p.stdout
    for k in ("k_span_copy", "k_plane_copy", "k_delta_copy", "k_window_copy"):    # the four row copies, all of row_copy.hip
        assert k in p.stdout
    assert "twin" not in p.stdout and b"twin" not in open(so, "rb").read()         # no kernel compiled a second time under another name: no symbol, device or host
    assert p.stdout.strip().endswith("RESULT: identical")
