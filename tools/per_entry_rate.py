#!/usr/bin/env python3
"""Developer: the rate an UNMODIFIED per-entry caller gets — the reference's read loop (tests/read_archive.c:21-35: one
zpack_read_file per entry, CDR order, one buffer, NULL dctx), timed by a small C driver (tools/per_entry_rate.c) that dlopen()s
the library under test, so that no Python runs inside the loop.

  tools/per_entry_rate.py [--out FILE] [--quick]

Workloads (benchdata): 20 000 x 64 KiB LZ4 and 8 000 x 256 KiB Zstandard level 3, each read memory-backed and file-backed by
  ra-on    libzpack_amd.so, read-ahead at its default (and at the caps of --caps, memory-backed)
  ra-off   libzpack_amd.so with ZPACK_AMD_READ_AHEAD=0 (the per-call path: one device batch per entry)
  ref      the compiled reference, one thread (oracle/_ref/libzpack_ref.so, when it was built)
plus random-order passes (2 x CALLS calls, two runs each of read-ahead on and off, taking turns; the mean is reported).  The
in-order ra-off pass times the first CALLS calls only (a per-call read of one entry costs milliseconds)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zpack_amd                                   # noqa: E402
from benchdata import datagen as dg                # noqa: E402

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libzpack_ref.so")
MIB = 1 << 20


def build_driver(d):
    exe = os.path.join(d, "per_entry_rate")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tools", "per_entry_rate.c"), "-ldl"])
    return exe


def run(exe, lib, arc, mode, order, calls, env_extra=None, timeout=600):
    env = dict(os.environ)
    env.pop("ZPACK_AMD_READ_AHEAD", None)
    env.update(env_extra or {})
    p = subprocess.run([exe, lib, arc, mode, order, str(calls)], env=env, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError("%s %s %s %s -> %d\n%s%s" % (os.path.basename(lib), mode, order, env_extra, p.returncode, p.stdout, p.stderr))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a tenth of the entries (a rehearsal of the tool itself)")
    ap.add_argument("--caps", default="64,1024", help="extra read-ahead caps in MiB, memory-backed in-order only")
    a = ap.parse_args()
    scale = 10 if a.quick else 1
    workloads = [("lz4_64k", 20000 // scale, 64 << 10, dg.LZ4, 0, 2000 // scale),
                 ("zstd3_256k", 8000 // scale, 256 << 10, dg.ZSTD, 3, 400 // scale)]
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as d:
        exe = build_driver(d)
        have_ref = os.path.exists(REF_SO)
        say("per-entry read loop (tests/read_archive.c:21-35): zpack_read_file per entry, NULL dctx, one buffer; GiB/s of decoded output")
        say("(GiB/s over all calls; the first call of this library also creates its context: GPU runtime and codec, 0.1-0.3 s)")
        say("reference: %s" % ("oracle/_ref/libzpack_ref.so, one thread" if have_ref else "not built here"))
        for name, n, size, method, level, calls in workloads:
            b = dg.Batch(n, size, method=method, level=level, seed=1)
            arc = os.path.join(d, name + ".zpk")
            b.archive.tofile(arc)
            say("")
            say("%s: %d entries, %.1f MiB compressed, %.1f MiB decoded" % (name, n, len(b.archive) / MIB, b.total_uncomp / MIB))
            b.close()
            for mode in ("mem", "file"):
                res = {}
                res["ra-on"] = run(exe, zpack_amd.ZPACK_SO, arc, mode, "seq", 0)
                res["ra-off"] = run(exe, zpack_amd.ZPACK_SO, arc, mode, "seq", calls, {"ZPACK_AMD_READ_AHEAD": "0"})
                if have_ref:
                    res["ref"] = run(exe, REF_SO, arc, mode, "seq", 0)
                # random order: 2 x CALLS calls, twice each, on and off taking turns; the mean of the two runs is reported
                rr = {"on": [], "off": []}
                for rep in range(2):
                    rr["on"].append(run(exe, zpack_amd.ZPACK_SO, arc, mode, "rand", 2 * calls))
                    rr["off"].append(run(exe, zpack_amd.ZPACK_SO, arc, mode, "rand", 2 * calls, {"ZPACK_AMD_READ_AHEAD": "0"}))
                for k in ("on", "off"):
                    a0, a1 = rr[k]
                    res["rand ra-%s" % k] = dict(a0, seconds=(a0["seconds"] + a1["seconds"]) / 2, gib_s=(a0["gib_s"] + a1["gib_s"]) / 2,
                                                 us_per_call=(a0["us_per_call"] + a1["us_per_call"]) / 2,
                                                 runs_gib_s=[a0["gib_s"], a1["gib_s"]])
                if have_ref:
                    res["rand ref"] = run(exe, REF_SO, arc, mode, "rand", calls)
                if mode == "mem":
                    for cap in [int(x) for x in a.caps.split(",") if x]:
                        res["ra-on cap %d MiB" % cap] = run(exe, zpack_amd.ZPACK_SO, arc, mode, "seq", 0, {"ZPACK_AMD_READ_AHEAD": str(cap * MIB)})
                for v in res.values():      # the rate past the first call, which creates the library's context (GPU runtime, codec)
                    rest = v["seconds"] - v["first_call_ms"] / 1e3
                    v["gib_s_after_first"] = v["bytes"] * (v["calls"] - 1) / v["calls"] / rest / 2**30 if rest > 0 and v["calls"] > 1 else 0.0
                for k, v in res.items():
                    say("  %-5s %-22s %6d calls  %9.2f us/call  %8.3f GiB/s  first call %7.2f ms, then %8.3f GiB/s  %8d page faults" % (
                        mode, k, v["calls"], v["us_per_call"], v["gib_s"], v["first_call_ms"], v["gib_s_after_first"], v["minflt"]))
                    rows.append(dict(workload=name, target=k, **v))
                on, off = res["ra-on"]["gib_s"], res["ra-off"]["gib_s"]
                ratio = "  %-5s in order: read-ahead / per-call = %.1fx" % (mode, on / off if off else float("inf"))
                if have_ref:
                    ratio += ", read-ahead / one reference thread = %.2fx (past the first call: %.2fx)" % (
                        on / res["ref"]["gib_s"], res["ra-on"]["gib_s_after_first"] / res["ref"]["gib_s_after_first"])
                ratio += "; random order, read-ahead on / off = %.3f (runs: on %s, off %s GiB/s)" % (
                    res["rand ra-on"]["gib_s"] / res["rand ra-off"]["gib_s"],
                    "/".join("%.4f" % x for x in res["rand ra-on"]["runs_gib_s"]), "/".join("%.4f" % x for x in res["rand ra-off"]["runs_gib_s"]))
                say(ratio)
    say("")
    say("json " + json.dumps(rows))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
