#!/usr/bin/env python3
"""The gfx950 code objects of two builds of libzpk_codec.so, compared.  Prints a markdown report; exit status 1 when anything differs.

  python tools/code_objects.py PARENT/zpack_amd/libzpk_codec.so zpack_amd/libzpk_codec.so [--names zpk_codec.hip row_copy.hip ...]
  python tools/code_objects.py --by-kernel PARENT/zpack_amd/libzpk_codec.so zpack_amd/libzpk_codec.so

By position (the default): the bytes of .text and every defined FUNC / OBJECT symbol with its address, size, type and binding (the
kernels, their .kd descriptors, the device variables), code object k of one build against code object k of the other.  A refactor of
host code must leave both as they are; a build that adds a .hip file behind the parent's must leave the parent's as they are (the added
code objects are listed, not compared).

By kernel (--by-kernel): for a build that has other .hip files than its parent, where positions say nothing.  Every kernel of the parent
(a FUNC symbol with a .kd descriptor) is looked up BY NAME in this build, in whichever code object it lies; compared are the bytes of
[address, address + size) and, from the AMDGPU metadata note, its VGPR, SGPR and AGPR counts, private and group segment sizes and max
flat workgroup size.  The parent's kernels that are gone and the kernels that are new are listed, not compared.  Code object 0
(zpk_codec.hip) is compared by position as well.

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
    """[(text bytes, [symbol lines], {kernel name: (its bytes, its figures in the metadata note)})] per bundle of `so`"""
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
        out.append((open(text, "rb").read(), sorted(syms), kernels_of(co, open(text, "rb").read(), syms)))
    return out


FIGURES = (".vgpr_count", ".sgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".max_flat_workgroup_size")


def kernels_of(co, text, syms):
    """{name: (bytes of [address, address + size), [the FIGURES of its entry in the AMDGPU metadata note])} of one code object"""
    text_addr = None
    for line in subprocess.check_output([tool("llvm-readelf"), "-S", "-W", co], text=True).split("\n"):
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) > 4 and f[1] == ".text":
            text_addr = int(f[3], 16)
    meta, cur = {}, None                         # the note is YAML of a fixed shape: a kernel's scalar fields stand at one indent
    for line in subprocess.check_output([tool("llvm-readelf"), "--notes", co], text=True).split("\n"):
        if line.startswith("  - "):
            cur = {}
            line = "    " + line[4:]
        if cur is not None and line.startswith("    .") and ":" in line:
            k, v = line.strip().split(":", 1)
            cur[k] = v.strip()
            if k == ".name":
                meta[cur[".name"]] = cur
    funcs = {}
    for s in syms:
        addr, size, typ, _, name = s.split()
        if typ == "FUNC":
            funcs[name] = (int(addr, 16), int(size))
    out = {}
    for name, (addr, size) in funcs.items():
        if name + ".kd" in {x.split()[4] for x in syms}:
            m = meta.get(name, {})
            out[name] = (text[addr - text_addr:addr - text_addr + size], [m.get(k, "?") for k in FIGURES])
    return out


def by_kernel(a, b):
    sha = lambda x: hashlib.sha256(x).hexdigest()[:16]
    where = lambda cos: {name: (k, v) for k, co in enumerate(cos) for name, v in co[2].items()}
    ka, kb = where(a), where(b)
    same = a[0][0] == b[0][0] and a[0][1] == b[0][1]
    print("Code object 0 by position: .text %d bytes `%s` / `%s`, %d symbols: %s\n" % (len(a[0][0]), sha(a[0][0]), sha(b[0][0]), len(a[0][1]), "identical" if same else "DIFFERENT"))
    print("| kernel | code object (parent) | (this build) | bytes | sha256 (parent) | (this build) | vgpr, sgpr, agpr, scratch, LDS, max workgroup (parent) | (this build) | |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in sorted(ka, key=lambda n: (ka[n][0], n)):
        if name not in kb:
            continue
        (ca, (ta, fa)), (cb, (tb, fb)) = ka[name], kb[name]
        ok = ta == tb and fa == fb and "?" not in fa
        same = same and ok
        print("| `%s` | %d | %d | %d%s | `%s` | `%s` | %s | %s | %s |" % (name, ca, cb, len(ta), "" if len(ta) == len(tb) else " / %d" % len(tb), sha(ta), sha(tb),
                                                                   ", ".join(fa), ", ".join(fb), "identical" if ok else "DIFFERENT"))
    print("\n(sha256 shortened to its first 16 hex digits; the figures are those of the AMDGPU metadata note.)\n")
    gone, new = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    print("Kernels of the parent that are gone: %s\n" % (", ".join("`%s` (code object %d)" % (n, ka[n][0]) for n in gone) or "none"))
    print("Kernels that are new: %s\n" % (", ".join("`%s` (code object %d)" % (n, kb[n][0]) for n in new) or "none"))
    print("RESULT: %s (%d kernels compared, %d gone, %d new)" % ("identical" if same else "DIFFERENT", len(set(ka) & set(kb)), len(gone), len(new)))
    return 0 if same else 1


def main():
    args = [a for a in sys.argv[1:] if a != "--by-kernel"]
    names = []
    if "--names" in args:
        k = args.index("--names")
        names = args[k + 1:]
        args = args[:k]
    if len(args) != 2:
        raise SystemExit(__doc__)
    with tempfile.TemporaryDirectory() as wa, tempfile.TemporaryDirectory() as wb:
        a, b = code_objects(args[0], wa), code_objects(args[1], wb)
    if "--by-kernel" in sys.argv[1:]:
        return by_kernel(a, b)
    same = len(a) <= len(b)                      # (a build may ADD code objects behind the parent's: those are listed, not compared)
    sha = lambda x: hashlib.sha256(x).hexdigest()[:16]
    print("| code object | .text bytes | .text sha256 (parent) | .text sha256 (this build) | symbols | symbol listing sha256 (parent) | (this build) |")
    print("|---|---|---|---|---|---|---|")
    for k in range(min(len(a), len(b))):
        (ta, sa), (tb, sb) = a[k][:2], b[k][:2]
        la, lb = "\n".join(sa).encode(), "\n".join(sb).encode()
        same = same and ta == tb and sa == sb
        print("| %s | %d%s | `%s` | `%s` | %d%s | `%s` | `%s` |" % (names[k] if k < len(names) else "bundle %d" % k, len(ta), "" if len(ta) == len(tb) else " / %d" % len(tb),
                                                                 sha(ta), sha(tb), len(sa), "" if len(sa) == len(sb) else " / %d" % len(sb), sha(la), sha(lb)))
    for k in range(len(a), len(b)):
        tb, sb = b[k][:2]
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
