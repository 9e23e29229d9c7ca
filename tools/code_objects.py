#!/usr/bin/env python3
"""The gfx950 code objects of two builds of libzpk_codec.so, compared: the bytes of .text and every defined FUNC / OBJECT symbol with
its address, size, type and binding (the kernels, their .kd descriptors, the device variables).  A refactor of host code must leave
both as they are; a build that adds a .hip file behind the parent's must leave the parent's as they are (the added code objects are
listed, not compared).  Prints a markdown report; exit status 1 when anything differs.

  python tools/code_objects.py PARENT/zpack_amd/libzpk_codec.so zpack_amd/libzpk_codec.so [--names zpk_codec.hip span_copy.hip ...]

The .hip_fatbin section holds one offload bundle per .hip file, in the order of the compile line (zpack_amd/build.py).  The symbol
__hip_cuid_<hash> is left out: clang derives its name from the path of the source file, so it differs between two directories."""
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def tool(name):
    for d in ("/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    t = shutil.which(name)
    if not t:
        raise SystemExit("%s not found" % name)
    return t


def code_objects(so, work):
    """[(text bytes, [symbol lines])] per bundle of `so`"""
    fat = os.path.join(work, "fatbin")
    subprocess.check_call([tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fat])
    blob = open(fat, "rb").read()
    starts = []
    at = blob.find(MAGIC)
    while at >= 0:
        starts.append(at)
        at = blob.find(MAGIC, at + 1)
    out = []
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else len(blob)
        bundle, co, text = (os.path.join(work, "%s%d" % (n, k)) for n in ("bundle", "co", "text"))
        open(bundle, "wb").write(blob[s:e])
        subprocess.check_call([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + bundle, "--output=" + co])
        subprocess.check_call([tool("llvm-objcopy"), "-O", "binary", "--only-section=.text", co, text])
        syms = []
        for line in subprocess.check_output([tool("llvm-readelf"), "-s", "-W", co], text=True).split("\n"):
            f = line.split()
            if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6] != "UND" and not f[7].startswith("__hip_cuid_"):
                syms.append("%s %7d %-6s %-6s %s" % (f[1], int(f[2], 0), f[3], f[4], f[7]))
        out.append((open(text, "rb").read(), sorted(syms)))
    return out


def main():
    args = [a for a in sys.argv[1:]]
    names = []
    if "--names" in args:
        k = args.index("--names")
        names = args[k + 1:]
        args = args[:k]
    if len(args) != 2:
        raise SystemExit(__doc__)
    with tempfile.TemporaryDirectory() as wa, tempfile.TemporaryDirectory() as wb:
        a, b = code_objects(args[0], wa), code_objects(args[1], wb)
    same = len(a) <= len(b)                      # (a build may ADD code objects behind the parent's: those are listed, not compared)
    sha = lambda x: hashlib.sha256(x).hexdigest()[:16]
    print("| code object | .text bytes | .text sha256 (parent) | .text sha256 (this build) | symbols | symbol listing sha256 (parent) | (this build) |")
    print("|---|---|---|---|---|---|---|")
    for k in range(min(len(a), len(b))):
        (ta, sa), (tb, sb) = a[k], b[k]
        la, lb = "\n".join(sa).encode(), "\n".join(sb).encode()
        same = same and ta == tb and sa == sb
        print("| %s | %d%s | `%s` | `%s` | %d%s | `%s` | `%s` |" % (names[k] if k < len(names) else "bundle %d" % k, len(ta), "" if len(ta) == len(tb) else " / %d" % len(tb),
                                                                 sha(ta), sha(tb), len(sa), "" if len(sa) == len(sb) else " / %d" % len(sb), sha(la), sha(lb)))
    for k in range(len(a), len(b)):
        tb, sb = b[k]
        print("| %s (added) | %d | | `%s` | %d | | `%s` |" % (names[k] if k < len(names) else "bundle %d" % k, len(tb), sha(tb), len(sb), sha("\n".join(sb).encode())))
    print("\n(sha256 shortened to its first 16 hex digits.)\n")
    for k in range(min(len(a), len(b))):
        sa, sb = a[k][1], b[k][1]
        print("## %s: the kernels (FUNC symbols; address, size)%s\n\n```" % (names[k] if k < len(names) else "bundle %d" % k, " — identical in both builds" if sa == sb else ""))
        for s in sb:
            f = s.split()
            if f[2] == "FUNC":
                print("%s %6s %s" % (f[0], f[1], f[4]))
        print("```\n")
        for s in sorted(set(sa) ^ set(sb)):
            print("DIFFERS: %s %s" % ("parent" if s in sa else "this  ", s))
    print("RESULT: %s" % ("identical" if same else "DIFFERENT"))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
