"""Output slots of a device decode batch at any address: layouts, refusal, the guard check and the case lists of
tests/test_slot_layouts_cpu.py (the helper itself and the inputs, on the CPU) and tests/test_gpu_slot_confinement.py (the device).
Not a test module.  Nothing here needs a GPU, and torch is imported only inside run_layout.

The output image of a batch is the slice [lead, lead + dst_size) of a larger allocation; the `lead` bytes in front of it and the `tail`
bytes behind it are guard zones of at least GUARD bytes that belong to no entry.  `dst_offset` is relative to the slice, so where `lead`
is odd the `dst` pointer the library is given is misaligned itself.

A case is a dict(label, method, frame, uncomp, cap, hash): one archive entry.  assemble() puts the frames of a list back to back into
an archive image, verdicts() asks the oracle about every entry."""
import collections
import ctypes as C

import numpy as np

GUARD = 4096
GAPS = (1, 3, 8, 15, 16, 17, 31, 64, 5)
LAYOUTS = ("aligned", "gapped", "packed", "packed_reversed")
FILLS = (0xA5, 0x5A)
NONE, ZSTD, LZ4 = 0, 1, 2
OK, BUFFER_TOO_SMALL, HASH_MISMATCH = 0, 12, 15

Placed = collections.namedtuple("Placed", "dst_offset dst_size lead tail")


def covers(starts):
    """the starts reach every residue mod 16 and at least 32 residues mod 128"""
    s = np.asarray(starts, dtype=np.uint64)
    return len(set((s % np.uint64(16)).tolist())) == 16 and len(set((s % np.uint64(128)).tolist())) >= 32


def lay_out(caps, layout, cover=True):
    """caps: the capacity of every slot -> Placed(dst_offset[], dst_size, lead, tail).
    aligned          what the decoder tests have used so far: every slot on a 256-byte grid with at least 64 bytes behind it
    gapped           slot i is followed by GAPS[i % len(GAPS)] guard bytes; the first slot begins at byte 1 of the slice, the slice ends
                     with the last slot
    packed           back to back, no byte between two slots; the slice begins at an odd address and ends with the last slot
    packed_reversed  packed, entry i + 1 in front of entry i
    In the three layouts off the grid the starts of the batch must reach every residue mod 16 and 32 residues mod 128 (absolute: `lead`
    included), or the batch proves less than it is meant to: that is asserted here.  cover=False is the caller's word that its batch is
    too short for that and is not meant to show it (the twelve entries of big_cases, a hand-made image of five slots)."""
    caps = np.asarray(caps, dtype=np.uint64)
    n = len(caps)
    assert layout in LAYOUTS, layout
    offs = np.zeros(n, dtype=np.uint64)
    if layout == "aligned":
        stride = (caps + np.uint64(255 + 64)) & ~np.uint64(255)
        if n > 1:
            offs[1:] = np.cumsum(stride[:-1])
        return Placed(offs, int(stride.sum()) + 256, GUARD, GUARD)
    if layout == "gapped":
        at = 1
        for i in range(n):
            offs[i] = at
            at += int(caps[i]) + GAPS[i % len(GAPS)]
        size = int(offs[-1] + caps[-1]) if n else 1
        lead = GUARD + 5
    else:
        ends = np.cumsum(caps)
        size = int(ends[-1]) if n else 0
        offs[:] = (ends - caps) if layout == "packed" else (np.uint64(size) - ends)
        lead = GUARD + 1
    assert size == (int((offs + caps).max()) if n else size), "nothing lies behind the last slot inside dst"
    if cover:
        assert covers(offs + np.uint64(lead)), (layout, "the slot addresses of this batch do not reach all 16 residues mod 16 and 32 mod 128")
    return Placed(offs, size, lead, GUARD + 5)


def refuse(desc, which):
    """A copy of a laid-out batch in which every second entry ("even": 0, 2, ..; "odd": 1, 3, ..) has dst_capacity = uncomp_size - 1: the
    classification refuses it with BUFFER_TOO_SMALL before a decoder sees it, every dst_offset stays, and the refused entry's whole slot
    is guard bytes directly against both neighbours.  Entries with uncomp_size 0 cannot be refused this way and stay."""
    assert which in ("even", "odd"), which
    d = desc.copy()
    for i in range(0 if which == "even" else 1, len(d), 2):
        if int(d[i]["uncomp_size"]) > 0:
            d[i]["dst_capacity"] = int(d[i]["uncomp_size"]) - 1
    return d


def is_live(desc):
    """the entries a decoder may write for: the classification lets them through its capacity rule (zpk_codec.hip, k_classify)"""
    return desc["dst_capacity"] >= desc["uncomp_size"]


def outside_untouched(image, lead, desc, fill, labels=None, limit=32):
    """Every byte of the whole allocation `image` that lies in no live slot — the two guard zones, the gaps and the slots of refused
    entries — must still be `fill`.  -> [(absolute index, value, label of the nearest live entry, distance to its slot, "front" |
    "behind")] of the first `limit` bytes that are not; distance 1 is the byte next to the slot.  [] means confined."""
    image = np.asarray(image)
    live = np.nonzero(is_live(desc))[0]
    lo = desc["dst_offset"][live].astype(np.int64) + lead
    hi = lo + desc["dst_capacity"][live].astype(np.int64)
    assert len(live) == 0 or (lo.min() >= 0 and hi.max() <= len(image))
    inside = np.zeros(len(image), dtype=bool)
    for a, b in zip(lo.tolist(), hi.tolist()):
        inside[a:b] = True
    out = []
    for k in np.nonzero(~inside & (image != fill))[0][:limit].tolist():
        if len(live) == 0:
            out.append((k, int(image[k]), None, None, None))
            continue
        dist = np.where(k < lo, lo - k, k - hi + 1)           # (k is in no live slot: k < lo or k >= hi for every one)
        j = int(np.argmin(dist))
        e = int(live[j])
        out.append((k, int(image[k]), e if labels is None else labels[e], int(dist[j]), "front" if k < lo[j] else "behind"))
    return out


def run_layout(codec, arc, desc, placed, fill, call="batch"):
    """One device batch: `desc` is laid out by `placed` (lay_out) and perhaps refused.  The whole allocation is filled with `fill`, the
    library gets the slice -> (results, the whole allocation as the device left it, decode_stats()).
    call: "batch" = decode_batch_device, "big" = decode_big_batch_device.  arc: bytes, or a uint8 tensor already on the device."""
    import torch
    import zpack_amd
    dev = torch.device("cuda:0")
    src = arc if isinstance(arc, torch.Tensor) else torch.from_numpy(np.frombuffer(bytes(arc), dtype=np.uint8).copy()).to(dev)
    whole = torch.full((placed.lead + placed.dst_size + placed.tail,), fill, dtype=torch.uint8, device=dev)
    dst = whole[placed.lead:placed.lead + placed.dst_size]
    assert dst.data_ptr() == whole.data_ptr() + placed.lead and dst.numel() == placed.dst_size
    n = len(desc)
    if call == "big":
        res = codec.decode_big_batch_device(src, desc, dst)
    else:
        ddesc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        dres = torch.zeros(n * zpack_amd.DECODE_RESULT.itemsize, dtype=torch.uint8, device=dev)
        codec.decode_batch_device(src, ddesc, n, dst, dres)
        torch.cuda.synchronize()
        res = dres.cpu().numpy().view(zpack_amd.DECODE_RESULT).copy()
    torch.cuda.synchronize()
    return res, whole.cpu().numpy(), codec.decode_stats()


# ---- batches and the oracle's verdicts ------------------------------------------------------------------------------------------------

def assemble(cases):
    """the frames back to back from byte 16 of an archive image with 64 bytes behind the last -> (image, descriptors without dst_offset)"""
    import zpack_amd
    desc = np.zeros(len(cases), dtype=zpack_amd.DECODE_DESC)
    at, parts = 16, [b"\0" * 16]
    for i, c in enumerate(cases):
        desc[i]["src_offset"] = at
        desc[i]["comp_size"] = len(c["frame"])
        desc[i]["uncomp_size"] = c["uncomp"]
        desc[i]["dst_capacity"] = c["cap"]
        desc[i]["expect_hash"] = c["hash"]
        desc[i]["method"] = c["method"]
        parts.append(bytes(c["frame"]))
        at += len(c["frame"])
    parts.append(b"\0" * 64)
    return b"".join(parts), desc


def placed_desc(desc, placed):
    d = desc.copy()
    d["dst_offset"] = placed.dst_offset
    return d


Verdict = collections.namedtuple("Verdict", "status produced hash bytes")


def verdicts(arc, desc, fill):
    """The oracle's verdict on every entry, its buffer pre-filled with `fill` as the device's slot is: the reference hashes uncomp_size
    bytes of the caller's buffer whatever the codec produced (lib/zpack_read.c:466), so where a frame ends early the verdict depends on
    what lay there.  bytes = the first uncomp_size bytes of the oracle's buffer (status OK or hash mismatch), else None."""
    from tests._libs import oracle
    L = oracle().lib
    a = np.frombuffer(bytes(arc), dtype=np.uint8)
    src = a.ctypes.data_as(C.POINTER(C.c_uint8))
    out = []
    for d in desc:
        cap, usz = int(d["dst_capacity"]), int(d["uncomp_size"])
        buf = np.full(max(1, cap), fill, dtype=np.uint8)
        got, h = C.c_uint64(0), C.c_uint64(0)
        rc = L.orc_entry_decode(src, len(a), int(d["src_offset"]), int(d["comp_size"]), usz, int(d["expect_hash"]), int(d["method"]),
                                buf.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(got), C.byref(h))
        out.append(Verdict(rc, got.value, h.value, buf[:usz].copy() if rc in (OK, HASH_MISMATCH) else None))
    return out


def family(c):
    """the kernel that the classification gives the entry to (k_classify; test_gpu_lz4_lean._has_plain_header)"""
    if c["method"] == NONE:
        return "k_stored"
    if c["method"] == ZSTD:
        return "k_zstd_fse / k_zstd_exec"
    if len(c["frame"]) < (c["uncomp"] >> 3):
        return "k_lz4_left"
    from tests.test_gpu_lz4_lean import _has_plain_header
    return "k_lz4_wave" if _has_plain_header(c["frame"]) else "k_lz4_general"


# ---- the case lists: the hand-built lists of the tree as they are, as cases -----------------------------------------------------------

def _case(label, method, frame, uncomp, cap, h):
    return dict(label=label, method=method, frame=bytes(frame), uncomp=int(uncomp), cap=int(cap), hash=int(h))


def _lz4_blocks(cs, prefix=""):
    """cases of test_gpu_lz4_asm_batches / lz4_overlap_blocks (a frame and offset positions) with the oracle's plaintext and its XXH3"""
    from benchdata import datagen as dg
    from tests._libs import oracle
    out = []
    for c in cs:
        rc, plain = oracle().lz4f_decode(c["frame"], 1 << 17)
        assert rc == 0 and 0 < len(plain) <= 65536 + 64, (c["label"], rc, len(plain))
        x = _case(prefix + c["label"], LZ4, c["frame"], len(plain), len(plain), dg.xxh3(np.frombuffer(plain, dtype=np.uint8)))
        x["offs"], x["target"] = c["offs"], c.get("target")
        out.append(x)
    return out


def lz4_overlap(left):
    """lz4_overlap_blocks.all_blocks(left): k_lz4_wave's (left False) and, behind a trailing run, k_lz4_left's"""
    from tests import lz4_overlap_blocks as blocks
    from tests.test_gpu_lz4_asm_batches import _case as block_case
    cs = []
    for b in blocks.all_blocks(left):
        c = block_case(b["label"], b["blk"], b["data"], left)
        c["target"] = b["target"]
        cs.append(c)
    return _lz4_blocks(cs, "left: " if left else "")


def lz4_batches():
    """the room, straddle and long-literal cases of test_gpu_lz4_asm_batches, for k_lz4_wave and k_lz4_left"""
    from tests import test_gpu_lz4_asm_batches as B
    lits = [c for left in (False, True) for c in B._piece_cases(left) if c["label"].startswith(("lit ", "literal "))]
    for c in lits:
        c["label"] = ("left: " if c["left"] else "") + c["label"]
    room = B._room_cases(False) + [dict(c, label="left: " + c["label"]) for c in B._room_cases(True)]
    return _lz4_blocks(room + B._straddle_cases() + lits)


def lz4_general(golden_dir):
    """the frames that are not one whole plain frame — the fixtures of the compiled reference and the frames with checksums, a
    dictionary id, a second frame, a skippable frame — which k_lz4_general decodes (test_gpu_lz4_lean._foreign_cases)"""
    from tests._libs import oracle
    from tests.test_gpu_lz4_lean import _foreign_cases
    return [_case(c["label"], LZ4, c["frame"], c["uncomp"], c["cap"], c["hash"]) for c in _foreign_cases(oracle(), golden_dir)]


def from_batch(b, prefix):
    arc = b.archive.tobytes()
    return [_case("%s %d (%d bytes)" % (prefix, i, int(b.uncomp_sizes[i])), int(b.methods[i]),
                  arc[int(b.offsets[i]):int(b.offsets[i]) + int(b.comp_sizes[i])], b.uncomp_sizes[i], b.uncomp_sizes[i], b.hashes[i]) for i in range(b.n)]


def lz4_generated():
    from benchdata import datagen as dg
    return (from_batch(dg.Batch(96, 1, 400, method=dg.LZ4, level=0, seed=31, mix=-1), "lz4 tiny") +
            from_batch(dg.Batch(32, 1000, 70000, method=dg.LZ4, level=0, seed=32, mix=-1), "lz4 blocks"))


def zstd_cases():
    """every case of zstd_asm.CASES as test_zstd_asm_cpu.judged makes it an entry (a case with a capacity of its own keeps it), and one
    generated batch"""
    from benchdata import datagen as dg
    from tests import zstd_asm as Z
    from tests.test_zstd_asm_cpu import judged
    out = []
    for c in Z.CASES:
        j = judged(c)
        x = _case(c["label"], ZSTD, c["frame"], j["uncomp"], j["cap"], j["hash"])
        x["group"], x["intact"], x["expect"] = c["group"], j["rc"] == 0, c["expect"]
        out.append(x)
    return out, from_batch(dg.Batch(64, 1, 70000, method=dg.ZSTD, level=3, seed=33, mix=-1), "zstd")


STORED_SIZES = (0, 1, 15, 16, 17, 239, 240, 241, 1023, 1024, 1025, 3000)


def stored_cases(rounds=16):
    """the sizes around the 16-byte and 240-byte steps of k_stored, each `rounds` times, rotated, so that every size meets many addresses"""
    from benchdata import datagen as dg
    out = []
    for r in range(rounds):
        for k in range(len(STORED_SIZES)):
            n = STORED_SIZES[(k + r) % len(STORED_SIZES)]
            plain = dg.fill(dg.RANDOM, 34, r * 16 + k, n)
            out.append(_case("stored %d bytes, round %d" % (n, r), NONE, plain.tobytes(), n, n, dg.xxh3(plain)))
    return out


DAMAGE = ("offset 0", "offset beyond the output", "output one byte short", "entry one byte short")


def damaged(cases, damage):
    """the four kinds of test_gpu_lz4_asm_overlap on cases that carry offset positions and a batch under test"""
    out = []
    for c in cases:
        c = dict(c, label="%s: %s" % (damage, c["label"]))
        if damage.startswith("offset"):
            k = 64 * c["target"] + 31
            f = bytearray(c["frame"])
            f[c["offs"][k]:c["offs"][k] + 2] = b"\x00\x00" if damage == "offset 0" else b"\xff\xff"
            c["frame"] = bytes(f)
        elif damage == "output one byte short":
            c["cap"] -= 1
        else:
            c["uncomp"] -= 1
            c["cap"] -= 1
        out.append(c)
    return out


def interleave(*lists):
    out = []
    for k in range(max(len(x) for x in lists)):
        out += [x[k] for x in lists if k < len(x)]
    return out


def big_cases():
    """small entries for the block-parallel readers and k_stored_span: group I of zstd_asm.CASES, LZ4 frames of 3 x 64 KiB + 1 and
    64 KiB + 5 bytes, a stored entry of 1025 bytes.  What a slot's address changes for k_pj_gather and k_zpj_init is the alignment of their
    word stores: their first word is whole whenever a chunk begins at a multiple of 4 bytes OF THE ENTRY (every frame here is one chunk,
    which begins at 0), their last word is partial because the sizes are no multiples of 4.  k_stored_span works on addresses: its first
    and last words are partial.  The order is the one in which the gapped layout gives the entries that are worth the whole chip
    (BIG_WHOLE_CHIP) slots that begin and end off a 4-byte boundary (tests/test_slot_layouts_cpu.py asserts it)"""
    from benchdata import datagen as dg
    group_i = [c for c in zstd_cases()[0] if c["group"] == "I"]
    out = group_i[-1:]
    for n in (3 * 65536 + 1, 65536 + 5):
        plain = dg.fill(dg.TEXT, 35, n & 15, n)
        out.append(_case("lz4 text %d bytes" % n, LZ4, dg.compress(dg.LZ4, 0, plain), n, n, dg.xxh3(plain)))
    plain = dg.fill(dg.RANDOM, 35, 2, 1025)
    out.append(_case("stored 1025 bytes", NONE, plain.tobytes(), 1025, 1025, dg.xxh3(plain)))
    return out + group_i[:-1]


BIG_WHOLE_CHIP = ("lz4 text %d bytes" % (3 * 65536 + 1), "stored 1025 bytes", "large blocks, far offsets inherited",
                  "two blocks of 120 KiB, repeat codes at LL = 0 inherited: large enough to be worth the reader")


def groups(golden_dir):
    """name -> case list of every batch the device tests run through the one-wave launch"""
    wave, left = lz4_overlap(False), lz4_overlap(True)
    hand, generated = zstd_cases()
    general = lz4_general(golden_dir)
    stored = stored_cases()
    g = collections.OrderedDict()
    g["lz4 overlap"] = wave + left
    batches = lz4_batches()
    g["lz4 batches, general, generated"] = interleave(batches, general, lz4_generated())
    g["zstd"] = interleave(hand, generated)
    g["stored"] = stored
    both = wave + left
    for dmg in DAMAGE:             # every damaged block among six intact ones (an odd period: refusing every second entry keeps the ratio)
        g["lz4 " + dmg] = interleave(damaged(both, dmg), *[both[k:] + both[:k] for k in range(6)])
    # (seven lists: with an odd period every kernel has live entries in both halves when every second entry is refused)
    g["mixed"] = interleave(wave[::3], [c for c in hand if c["group"] != "I"], stored, left[::3], general, generated[::2], batches[::3])
    return g
