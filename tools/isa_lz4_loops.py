#!/usr/bin/env python3
"""Static instruction counts of the loops of one kernel in a gfx950 assembly listing (hipcc -S --cuda-device-only).

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-function --cuda-device-only -S -o zpk_codec.s zpack_amd/csrc/zpk_codec.hip
  python tools/isa_lz4_loops.py zpk_codec.s [k_lz4_wave]

The compiler annotates every basic block with the loop it belongs to; the loop tree is rebuilt from those comments and every loop gets
counts of its OWN blocks (those of the loops inside it left out; the batch loop also inclusive): vector instructions, lane reads / writes that are scalar-register
spills (v_readlane / v_writelane on the VGPRs the kernel's prologue comments name as SGPR spill slots: in practice the highest
numbered ones, taken here as the registers that v_writelane writes with an SGPR source and v_readlane reads back into an SGPR),
s_nop, v_mov.  `valu_sans_header` leaves the loop's header block out as well: the convention under which the kernel was first
measured (679 / 82 / 81 / 79 for batch / rounds / hop1 / hop2 of the general walker's build; with the header 681 / 82 / 84 / 87).
lz4_loops() names the loops of k_lz4_wave the decoder's structure defines:

  batch   the loop over batches of 64 sequences: the largest loop that holds the token-list read (ds_read_u16) and a child loop
  rounds  the copy-rounds loop inside it: the largest child loop of the batch loop
  hop1/2  the two token-chain walks (first walk, fix-up walk): the loops without children that read three single bytes from LDS
          and shift a 64-bit mask (v_lshlrev_b64 / v_lshrrev_b64), in program order

hash_loop() reports the XXH3 verify pass (xxh3_64_wave, one iteration = 4 KiB): the loop with at least four v_mad_u64_u32 and 16-byte
global loads; vector instructions, ds_bpermute, v_mov and 16-byte loads per iteration, blocks of inner loops included.
"""
import re
import sys


def kernel_body(text, name):
    """the lines of function `name` (between its label and .Lfunc_end)"""
    lines = text.splitlines()
    sym = "_Z%d%s" % (len(name), name)                      # the kernel's mangled name starts with its length and its name
    start = next(i for i, l in enumerate(lines) if re.match(r"(%s|%s)\w*:" % (re.escape(sym + "P"), re.escape(name)), l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def kernel_meta(text, name):
    """scratch bytes, VGPRs, LDS bytes, occupancy from the kernel's trailer comments / .amdhsa directives"""
    sym = "_Z%d%sP" % (len(name), name)
    tail = text[text.index(".amdhsa_kernel " + sym):]
    tail = tail[:tail.index(".end_amdhsa_kernel") + 4000]
    out = {}
    for key, pat in (("vgprs", r"\.amdhsa_next_free_vgpr (\d+)"), ("scratch", r"\.amdhsa_private_segment_fixed_size (\d+)"),
                     ("lds", r"\.amdhsa_group_segment_fixed_size (\d+)"), ("sgprs", r"\.amdhsa_next_free_sgpr (\d+)"),
                     ("occupancy", r"; Occupancy: (\d+)"), ("code_bytes", r"; codeLenInByte = (\d+)")):
        m = re.search(pat, tail)
        out[key] = int(m.group(1)) if m else None
    return out


class Loop:
    def __init__(self, header, depth):
        self.header, self.depth, self.parent, self.children = header, depth, None, []
        self.own = []                       # instructions of blocks whose innermost loop is this one
        self.head = []                      # ... of them, the header block's

    def insts(self):
        r = list(self.own)
        for c in self.children:
            r += c.insts()
        return r


def loops_of(body):
    loops, order = {}, []
    # pass 1: block -> loop from the comment lines that follow a label
    blocks = []                             # (label, [comment lines], [instructions])
    for l in body:
        s = l.strip()
        if re.match(r"\.LBB\d+_\d+:", s) or s.startswith("; %bb."):
            blocks.append([s.split(":")[0].lstrip("."), [s], []])
            continue
        if not blocks:
            continue
        if s.startswith(";"):
            blocks[-1][1].append(s)
            continue
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        blocks[-1][2].append(s)
    # (a block may be laid out in front of its loop's header: headers first, then the members)
    for label, comments, insts in blocks:
        txt = "\n".join(comments)
        m_hdr = re.search(r"Loop Header: Depth=(\d+)", txt)
        if m_hdr:
            lp = Loop(label.lstrip("L"), int(m_hdr.group(1)))
            loops[lp.header] = lp
            order.append(lp)
            parents = re.findall(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", txt)
            if parents:
                lp.parent = max(parents, key=lambda p: int(p[1]))[0]
            lp.own += insts
            lp.head = list(insts)
    for label, comments, insts in blocks:
        txt = "\n".join(comments)
        m_in = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", txt)
        if m_in and not re.search(r"Loop Header: Depth=", txt):
            loops[m_in.group(1)].own += insts
    for lp in order:
        if lp.parent and lp.parent in loops:
            loops[lp.parent].children.append(lp)
    return order


def spill_vgprs(body):
    """VGPRs used as SGPR spill slots: written by v_writelane from an SGPR AND read back by v_readlane"""
    w, r = set(), set()
    for l in body:
        s = l.strip()
        m = re.match(r"v_writelane_b32 (v\d+), s\d+, \d+", s)
        if m:
            w.add(m.group(1))
        m = re.match(r"v_readlane_b32 s\d+, (v\d+), \d+", s)
        if m:
            r.add(m.group(1))
    return w & r


def count(insts, spills):
    c = dict(valu=0, spill=0, s_nop=0, v_mov=0, total=len(insts))
    for s in insts:
        op = s.split()[0]
        if op.startswith("v_"):
            c["valu"] += 1
        if op in ("v_mov_b32", "v_mov_b64", "v_mov_b32_e32", "v_mov_b64_e32"):
            c["v_mov"] += 1
        if op == "s_nop":
            c["s_nop"] += 1
        m = re.match(r"v_writelane_b32 (v\d+), s\d+, \d+", s) or re.match(r"v_readlane_b32 s\d+, (v\d+), \d+", s)
        if m and m.group(1) in spills:
            c["spill"] += 1
    return c


def lz4_loops(text, name="k_lz4_wave"):
    body = kernel_body(text, name)
    spills = spill_vgprs(body)
    order = loops_of(body)

    def has(insts, pat):
        return sum(1 for s in insts if re.match(pat, s))
    batch_c = [lp for lp in order if lp.children and has(lp.own, r"ds_read_u16")]
    if not batch_c:
        raise RuntimeError("k_lz4_wave: no batch loop recognised")
    batch = max(batch_c, key=lambda lp: len(lp.insts()))
    rounds = max(batch.children, key=lambda lp: len(lp.insts()))
    around, lp = set(), batch                       # the batch loop and the loops around it
    by_header = {x.header: x for x in order}
    while lp is not None:
        around.add(lp.header)
        lp = by_header.get(lp.parent)
    hops = [lp for lp in order if lp.header not in around and has(lp.own, r"ds_read_u8") >= 3 and has(lp.own, r"v_lsh[lr]rev_b64|v_lshl_b64|v_lshr_b64")]
    if len(hops) != 2:
        raise RuntimeError("k_lz4_wave: %d hop loops recognised, expected the first walk and the fix-up walk" % len(hops))
    # OWN counts: the loop's blocks without those of the loops inside it (the rare out-of-line paths inside a hop are loops of their own)
    def both(lp):
        c = count(lp.own, spills)
        h = count(lp.head, spills)
        c["valu_sans_header"] = c["valu"] - h["valu"]      # the convention of the first measurement (parent: 679 / 82 / 81 / 79)
        return c
    res = dict(batch=both(batch), rounds=both(rounds), hop1=both(hops[0]), hop2=both(hops[1]), batch_inclusive=count(batch.insts(), spills))
    whole = [s.strip() for s in body if s.strip() and not s.strip().startswith((";", ".")) and not s.strip().endswith(":")]
    res["kernel"] = count(whole, spills)
    res["spill_vgprs"] = sorted(spills)
    res["meta"] = kernel_meta(text, name)
    return res


def hash_loop(text, name="k_lz4_wave"):
    """the XXH3 loop of kernel `name`: static counts per iteration (4 KiB of input)"""
    body = kernel_body(text, name)

    def has(insts, pat):
        return sum(1 for s in insts if re.match(pat, s))
    cands = [lp for lp in loops_of(body) if has(lp.insts(), r"v_mad_u64_u32") >= 4 and has(lp.insts(), r"global_load_dwordx4")]
    if not cands:
        raise RuntimeError("%s: no hash loop recognised" % name)
    lp = min(cands, key=lambda l: len(l.insts()))          # the innermost of them
    insts = lp.insts()
    c = count(insts, spill_vgprs(body))
    return dict(valu=c["valu"], ds_bpermute=has(insts, r"ds_bpermute_b32"), v_mov=c["v_mov"], loads=has(insts, r"global_load_dwordx4"),
                mad_u64=has(insts, r"v_mad_u64_u32"), permlane_swap=has(insts, r"v_permlane(16|32)_swap"), lds_reads=has(insts, r"ds_read"),
                waitcnt_vm0=has(insts, r"s_waitcnt vmcnt\(0\)"), v_mov_b64=has(insts, r"v_mov_b64"), total=c["total"])


if __name__ == "__main__":
    t = open(sys.argv[1]).read()
    r = lz4_loops(t, sys.argv[2] if len(sys.argv) > 2 else "k_lz4_wave")
    for k in ("meta", "spill_vgprs", "kernel", "batch", "batch_inclusive", "rounds", "hop1", "hop2"):
        print(k, r[k])
    print("hash", hash_loop(t, sys.argv[2] if len(sys.argv) > 2 else "k_lz4_wave"))
