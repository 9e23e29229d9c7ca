#!/usr/bin/env python3
"""CPU model of which batches seq_exec_batch (seq_exec.h, section 3a) assembles in LDS, and why it refuses the others.  The chunking is
lz4_block_wave's (lz4_wave.h): a chunk holds the tokens of 3840 block bytes from the chain position, its sequences are executed 64 at a
time, their token positions are listed in windows of 576.  A batch is assembled when total + 48 <= room and it holds no piece longer
than 32 bytes and no self-overlapping match (the shipped executor also takes literal runs longer than 32 bytes; under the piece rule,
`self_asm`, also self-overlapping matches of at most 32 bytes, which a lane copies in pieces off, off, 2 off, 4 off ... through the same
round body: pieces() counts them); room = the bytes of the stage that are dead:

  own    up to the batch's own first token (the rule of the builds before the room was extended)
  next   up to the NEXT batch's first token; for a chunk's last batch up to the chain's exit (at most 3904); at a window boundary of the
         token list `own`

Developer tool, no GPU.  tests/test_gpu_lz4_asm_batches.py uses plan() to check that its hand-built blocks sit where they mean to.
  tools/sim/lz4_asm_share.py [mix] [entries]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

SEG, WAVE, NREC, SLACK = 60, 64, 576, 64
CHUNK = SEG * WAVE
OWN_MAX, ASM_PRE, ASM_SLACK = 32, 32, 16


def sequences(d):
    """-> [(token position, ll, ml, off, next token position)] of one well-formed block (the last sequence has ml = 0)"""
    C = len(d); p = 0; out = []
    while p < C:
        t0 = p
        tok = int(d[p]); p += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                b = int(d[p]); p += 1; ll += b
                if b != 255: break
        p += ll
        if p >= C:
            out.append((t0, ll, 0, 0, C)); break
        off = int(d[p]) | (int(d[p + 1]) << 8); p += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = int(d[p]); p += 1; ml += b
                if b != 255: break
        out.append((t0, ll, ml + 4, off, p))
    return out


def pieces(ml, off):
    """copy steps of one match under the piece rule: min(ml, off) bytes from its source, then from its own start as many bytes as are
    valid there (off, 2 off, 4 off ...) until ml bytes are written; 1 for a plain match"""
    n, done = 1, min(ml, off)
    while done < ml:
        done += min(ml - done, done); n += 1
    return n


def plan(d):
    """-> one dict per batch of the block, in execution order: chunk, index in the chunk, first / count (sequence numbers in the block),
    cpos, out (output position of the batch in the block), total, room_own, room_next, and the kinds of pieces that keep it direct;
    for the piece rule: self_short / self_long (a self-overlapping match of at most / more than 32 bytes), self_count (how many of
    either), self_steps (copy steps of the batch's worst self-overlapping match of at most 32 bytes, 0 without one)"""
    seqs = sequences(d)
    C = len(d); out = []; i = 0; cpos = 0; ci = 0; opos = 0
    while i < len(seqs):
        tok_end = min(C, cpos + CHUNK)
        j = i
        while j < len(seqs) and seqs[j][0] < tok_end: j += 1
        chain_exit = seqs[j - 1][4]
        for b0 in range(i, j, WAVE):
            bs = seqs[b0:min(b0 + WAVE, j)]
            bw = (b0 - i) % NREC
            own = bs[0][0] - cpos
            if bw + len(bs) == NREC: nxt = own
            elif b0 + WAVE >= j: nxt = min(chain_exit - cpos, CHUNK + SLACK)
            else: nxt = seqs[b0 + WAVE][0] - cpos
            total = sum(s[1] + s[2] for s in bs)
            out.append(dict(chunk=ci, index=(b0 - i) // WAVE, first=b0, count=len(bs), cpos=cpos, out=opos, total=total, room_own=own,
                            room_next=max(nxt, own),
                            lit_long=any(s[1] > OWN_MAX for s in bs), match_long=any(s[2] > OWN_MAX and s[2] <= s[3] for s in bs),
                            self16=any(s[2] > s[3] >= 16 for s in bs), self1=any(s[2] > s[3] and s[3] < 16 for s in bs),
                            self_short=any(s[3] < s[2] <= OWN_MAX for s in bs), self_long=any(s[2] > s[3] and s[2] > OWN_MAX for s in bs),
                            self_count=sum(1 for s in bs if s[2] > s[3]),
                            self_steps=max([pieces(s[2], s[3]) for s in bs if s[3] < s[2] <= OWN_MAX], default=0)))
            opos += total
        i = j; cpos = chain_exit; ci += 1
    return out


def assembled(b, rule, long_lit=False, self_asm=False):
    """rule: "own" / "next" (the room); long_lit: a literal run longer than 32 bytes does not keep the batch direct; self_asm: nor does a
    self-overlapping match of at most 32 bytes (the piece rule)"""
    selfs = b["self_long"] if self_asm else (b["self16"] or b["self1"])
    return b["total"] + ASM_PRE + ASM_SLACK <= b["room_" + rule] and not ((b["lit_long"] and not long_lit) or b["match_long"] or selfs)


if __name__ == "__main__":
    import numpy as np
    from benchdata import datagen as dg
    from tools.sim.lz4_walk_sim import blocks_of
    mix = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    b = dg.Batch(n, 65536, 65536, method=dg.LZ4, level=0, seed=1, mix=mix)
    st = dict(batches=0, asm_own=0, asm_next=0, asm_ship=0, room_only=0, piece_only=0, both=0, fits_next=0, fits_1536=0, first=0, bytes=0,
              lit_long=0, match_long=0, self16=0, self1=0, chunks=0,
              ship_bytes=0, asm_self=0, asm_self_bytes=0, only_short=0, only_short_bytes=0, only_any=0, seqs=0, selfs=0, selfs_short=0)
    steps = {}
    for e in range(n):
        fr = b.archive[int(b.offsets[e]):int(b.offsets[e]) + int(b.comp_sizes[e])]
        for blk in blocks_of(fr):
            for q in sequences(np.asarray(blk)):
                st["seqs"] += 1; st["selfs"] += q[2] > q[3]; st["selfs_short"] += q[3] < q[2] <= OWN_MAX
            for p in plan(np.asarray(blk)):
                ship, new = assembled(p, "next", True), assembled(p, "next", True, True)
                st["ship_bytes"] += p["total"] * ship; st["asm_self"] += new; st["asm_self_bytes"] += p["total"] * new
                st["only_short"] += new and not ship; st["only_short_bytes"] += p["total"] * (new and not ship)
                fits = p["total"] + ASM_PRE + ASM_SLACK <= p["room_next"]
                st["only_any"] += fits and not ship and not p["match_long"] and (p["self_short"] or p["self_long"])
                if new and not ship: steps[p["self_steps"]] = steps.get(p["self_steps"], 0) + 1
                piece = p["lit_long"] or p["match_long"] or p["self16"] or p["self1"]
                room = p["total"] + ASM_PRE + ASM_SLACK > p["room_own"]
                st["batches"] += 1; st["bytes"] += p["total"]; st["chunks"] += p["index"] == 0
                st["asm_own"] += assembled(p, "own"); st["asm_next"] += assembled(p, "next"); st["asm_ship"] += assembled(p, "next", True)
                st["room_only"] += room and not piece; st["piece_only"] += piece and not room; st["both"] += room and piece
                st["fits_next"] += p["total"] + ASM_PRE + ASM_SLACK <= p["room_next"]
                st["fits_1536"] += p["total"] + ASM_PRE + ASM_SLACK <= 1536
                for k in ("lit_long", "match_long", "self16", "self1"):
                    st[k] += p[k] and p["total"] + ASM_PRE + ASM_SLACK <= p["room_next"]
    nb = st["batches"]
    print("mix %d, %d entries: %d batches in %d chunks (%.1f per chunk), mean output %.0f B" % (mix, n, nb, st["chunks"], nb / st["chunks"], st["bytes"] / nb))
    for k, label in (("asm_own", "assembled, room up to the batch's own first token"), ("room_only", "  direct only for lack of that room"),
                     ("piece_only", "  direct only for a long or self-overlapping piece"), ("both", "  both"),
                     ("fits_next", "total + 48 fits the room up to the NEXT batch's first token"), ("asm_next", "assembled under that rule"),
                     ("asm_ship", "assembled under that rule, long literal runs allowed"),
                     ("lit_long", "  fits, holds a literal run > 32"), ("match_long", "  fits, holds a plain match > 32"),
                     ("self16", "  fits, holds a self-overlapping match, offset >= 16"), ("self1", "  fits, holds a self-overlapping match, offset < 16"),
                     ("fits_1536", "total + 48 <= 1536")):
        print("  %-62s %5.1f %%" % (label, 100.0 * st[k] / nb))
    nby = st["bytes"]
    print("the piece rule (a self-overlapping match of at most 32 bytes is copied in pieces inside the assembled batch):")
    for label, k, kb in (("assembled as shipped (batches / bytes)", "asm_ship", "ship_bytes"),
                         ("has the room, kept direct ONLY by self-overlapping matches of length <= 32", "only_short", "only_short_bytes"),
                         ("assembled under the piece rule", "asm_self", "asm_self_bytes")):
        print("  %-76s %5.1f %% / %5.1f %%" % (label, 100.0 * st[k] / nb, 100.0 * st[kb] / nby))
    print("  %-76s %5.1f %%" % ("... the same, any length", 100.0 * st["only_any"] / nb))
    print("  self-overlapping matches, total: %d of %d sequences; of length <= 32: %.1f %%" % (st["selfs"], st["seqs"], 100.0 * st["selfs_short"] / max(st["selfs"], 1)))
    print("  copy steps of the worst lane in the batches the rule moves: " + ", ".join("%d (%d batches)" % (k, v) for k, v in sorted(steps.items())))
