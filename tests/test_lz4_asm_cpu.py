"""The hand-built LZ4 frames of tests/lz4_asm.py before they go near a GPU.  liblz4 (the library the compiled reference links), driven
by the reference's call loop (lib/zpack_read.c:414-439: all the input, the remaining capacity), the oracle and — where it was built —
the compiled reference must agree on every case of groups A to G: status, bytes and hash, at the entry's capacity and at 64 bytes
more.  The case table's `walk` / `nblocks` are checked against a Python restatement of walk_lz4_single_to, and every label's claim
about the geometry against a small block walker over the frame itself.  The strict walker of tests/lz4_frames.py is not applied: these
frames break its encoder rules on purpose.

Group L pins a difference as it stands: liblz4 refuses a block in which the literals of a sequence that carries a match end less than
8 bytes before the block's end (unless its shortcut for 10 to 14 literals takes the sequence) or the extension bytes of a match length
end less than 5 bytes before it; orc_lz4_block_decode and the device decoders accept both.  Whoever aligns them finds the cases here."""
import ctypes as C
import ctypes.util
import struct

import numpy as np
import pytest

from tests import lz4_asm as A
from tests import zpk
from tests._libs import have_ref, oracle, ref

LZ4 = 2
FILL = 0xA5                  # what lies in every buffer before a judge writes to it (the device tests fill their slots with it)
OK, BUFFER_TOO_SMALL, DECOMPRESS_FAILED, HASH_MISMATCH, FILE_INCOMPLETE = 0, 12, 13, 15, 17
WRAPPED_REFUSED = {}         # label -> reason: wrapped blocks of group C that liblz4 refuses after all (at most a tenth of them; none today)


_liblz4 = None


def liblz4():
    global _liblz4
    if _liblz4 is None:
        z = C.CDLL(ctypes.util.find_library("lz4"))
        z.LZ4F_createDecompressionContext.restype = C.c_size_t
        z.LZ4F_createDecompressionContext.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        z.LZ4F_freeDecompressionContext.argtypes = [C.c_void_p]
        z.LZ4F_decompress.restype = C.c_size_t
        z.LZ4F_decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
        z.LZ4F_isError.argtypes = [C.c_size_t]
        _liblz4 = z
    return _liblz4


def liblz4_read(frame, uncomp, cap, want_hash):
    """zpack_read_file for an LZ4 entry with liblz4 as its codec -> (status, the buffer, bytes produced)"""
    buf = np.full(max(1, cap), FILL, dtype=np.uint8)
    if len(frame) == 0:
        return OK, buf, 0
    if cap < uncomp:
        return BUFFER_TOO_SMALL, buf, 0
    z = liblz4()
    ctx = C.c_void_p()
    assert not z.LZ4F_isError(z.LZ4F_createDecompressionContext(C.byref(ctx), 100))
    src = np.frombuffer(frame, dtype=np.uint8)
    try:
        at_in, at_out, last = 0, 0, 1
        while cap - at_out > 0 and len(src) - at_in > 0:                 # lib/zpack_read.c:414-439
            dn, sn = C.c_size_t(cap - at_out), C.c_size_t(len(src) - at_in)
            last = z.LZ4F_decompress(ctx, buf.ctypes.data + at_out, C.byref(dn), src.ctypes.data + at_in, C.byref(sn), None)
            if z.LZ4F_isError(last):
                return DECOMPRESS_FAILED, buf, at_out
            at_in += sn.value
            at_out += dn.value
        if last != 0:
            return (FILE_INCOMPLETE if cap - at_out > 0 else BUFFER_TOO_SMALL), buf, at_out
    finally:
        z.LZ4F_freeDecompressionContext(ctx)
    return (OK if oracle().xxh3(buf[:uncomp]) == want_hash else HASH_MISMATCH), buf, at_out


def oracle_read(arc, off, comp, uncomp, cap, want_hash):
    buf = np.full(max(1, cap), FILL, dtype=np.uint8)
    a = np.frombuffer(arc, dtype=np.uint8)
    got, h = C.c_uint64(0), C.c_uint64(0)
    u8p = C.POINTER(C.c_uint8)
    rc = oracle().lib.orc_entry_decode(a.ctypes.data_as(u8p), len(a), off, comp, uncomp, want_hash, LZ4, buf.ctypes.data_as(u8p), cap, C.byref(got), C.byref(h))
    return rc, buf, got.value


def reference_read(arc, cap):
    R = ref()
    rr, reader, keep = R.open_memory(arc)
    assert rr == 0
    buf = np.full(max(1, cap), FILL, dtype=np.uint8)
    rc = R.lib.zpack_read_file(C.byref(reader), C.byref(reader.file_entries[0]), buf.ctypes.data_as(C.POINTER(C.c_uint8)), cap, None)
    R.close_reader(reader)
    return rc, buf


_plain = {}
_judged = {}


def plain_hash(c):
    """the XXH3 the entry carries: of the bytes the oracle decodes from the case's frame (hash_of: from that case's), 0 when it decodes none"""
    base = c if c["hash_of"] is None else [x for x in A.CASES if x["label"] == c["hash_of"]][0]
    if base["label"] not in _plain:
        buf = np.zeros(base["uncomp"] + 65536 + 64, dtype=np.uint8)
        f = np.frombuffer(base["frame"], dtype=np.uint8)
        got = C.c_size_t(0)
        u8p = C.POINTER(C.c_uint8)
        rc = oracle().lib.orc_lz4f_decode(f.ctypes.data_as(u8p), len(f), buf.ctypes.data_as(u8p), len(buf), C.byref(got))
        _plain[base["label"]] = (rc, buf[:got.value])
    rc, plain = _plain[base["label"]]
    return oracle().xxh3(plain[:c["uncomp"]]) if rc == 0 and len(plain) >= c["uncomp"] else 0


def judged(c):
    """the oracle's verdict on a case as an archive entry at its own capacity (the record the device tests compare with):
    dict(rc, out = the buffer as the oracle leaves it, produced, hash = the hash the entry carries, arc, off)"""
    if c["label"] not in _judged:
        h = plain_hash(c)
        arc = zpk.assemble([c["frame"]], [("f", 10, len(c["frame"]), c["uncomp"], h, LZ4)])
        rc, out, got = oracle_read(arc, 10, len(c["frame"]), c["uncomp"], c["cap"], h)
        _judged[c["label"]] = dict(rc=rc, out=out, produced=got, hash=h, arc=arc, off=10)
    return _judged[c["label"]]


# ---- walk_lz4_single_to (zpack_amd/csrc/host_walk.h:182-202) and lz4_single_header (:125-136), restated ------------------------------

def walk(p, uncomp):
    """-> (accepted, blocks, independent)"""
    comp = len(p)
    if comp >= 0x7FFF0000 or uncomp >= 0x7FFF0000 or comp < 7:
        return False, 0, 0
    if p[:4] != b"\x04\x22\x4d\x18":
        return False, 0, 0
    flg, bd = p[4], p[5]
    if (flg >> 6) != 1 or (flg & 0x17) or bd != 0x40:
        return False, 0, 0
    hdr = 7 + (8 if flg & 0x08 else 0)
    if comp < hdr or ((A.xxh32(p[4:hdr - 1]) >> 8) & 0xFF) != p[hdr - 1]:
        return False, 0, 0
    if comp < hdr + 4 or ((flg & 0x08) and struct.unpack_from("<Q", p, 6)[0] != uncomp):
        return False, 0, 0
    q, nb = hdr, 0
    while True:
        if comp - q < 4:
            return False, 0, 0
        w = struct.unpack_from("<I", p, q)[0]
        q += 4
        if w == 0:
            break
        n = w & 0x7FFFFFFF
        if n == 0 or n > 65536 or n > comp - q:
            return False, 0, 0
        nb += 1
        q += n
    return (q == comp and nb >= 4), (nb if q == comp and nb >= 4 else 0), (flg >> 5) & 1


# ---- a block walker: what a frame's blocks and sequences are, from its bytes ---------------------------------------------------------

def sequences(d):
    """the sequences of one block: [(output position, literal length, literal position, offset, match length, block position behind the
    sequence)] (offset 0, match length 0: the last sequence) or None when the tokens run out of the block"""
    out, p, o = [], 0, 0
    while True:
        if p >= len(d):
            return None
        t = d[p]; p += 1
        ll = t >> 4
        if ll == 15:
            while True:
                if p >= len(d): return None
                ll += d[p]; p += 1
                if d[p - 1] != 255: break
        lp = p
        p += ll
        if p > len(d):
            return None
        if p == len(d):
            out.append((o, ll, lp, 0, 0, p))
            return out
        if p + 2 > len(d):
            return None
        off = d[p] | (d[p + 1] << 8); p += 2
        ml = (t & 15) + 4
        if ml == 19:
            while True:
                if p >= len(d): return None
                ml += d[p]; p += 1
                if d[p - 1] != 255: break
        out.append((o, ll, lp, off, ml, p))
        o += ll + ml


def frame_blocks(f):
    """[(stored, payload, sequences or None, output bytes, output offset)] of a frame that has the plain header and no block checksums"""
    hdr = 7 + (8 if f[4] & 0x08 else 0)
    q, at, out = hdr, 0, []
    while True:
        w = struct.unpack_from("<I", f, q)[0]; q += 4
        if w == 0:
            return out
        n = w & 0x7FFFFFFF
        d = f[q:q + n]; q += n
        if w >> 31:
            out.append((True, d, None, n, at)); at += n
        else:
            s = sequences(d)
            size = (s[-1][0] + s[-1][1]) if s else 0
            out.append((False, d, s, size, at)); at += size


def in_liblz4s_rule(d, s):
    return all(len(d) - (lp + ll) >= 8 and (ml < 19 or len(d) - e >= 5) for o, ll, lp, off, ml, e in s if ml)


CASES = A.CASES
GROUPS = "ABCDEFG"


def test_the_table_holds_every_group():
    n = {g: sum(1 for c in CASES if c["group"] == g) for g in GROUPS + "L"}
    assert n["A"] >= 11 and n["B"] >= 6 and n["C"] >= 13 + 314 and n["D"] >= 10 and n["E"] >= 7 and n["F"] == 19 and n["G"] == 12 and n["L"] >= 12, n
    assert sum(1 for c in CASES if c["label"].startswith("C: wrapped")) == 314
    assert len(WRAPPED_REFUSED) <= 31
    assert len(set(c["label"] for c in CASES)) == len(CASES)


def test_walk_and_nblocks_of_the_table_are_the_walkers():
    for c in CASES:
        ok, nb, indep = walk(c["frame"], c["uncomp"])
        assert (ok, nb) == (c["walk"], c["nblocks"]), (c["label"], ok, nb)
        assert not ok or bool(indep) == c["independent"], c["label"]
        assert c["walk"] or not c["reader"], c["label"]


@pytest.mark.parametrize("group", list(GROUPS))
def test_liblz4_the_oracle_and_the_reference_agree(group):
    seen = 0
    for c in CASES:
        if c["group"] != group or c["label"] in WRAPPED_REFUSED:
            continue
        seen += 1
        j = judged(c)
        for cap in (c["cap"], c["cap"] + 64):
            lrc, lbuf, lgot = liblz4_read(c["frame"], c["uncomp"], cap, j["hash"])
            orc, obuf, ogot = oracle_read(j["arc"], j["off"], len(c["frame"]), c["uncomp"], cap, j["hash"])
            pinned = c["claims"].get("liblz4_status")           # a damaged offset of 0: the difference as it stands (tests/lz4_asm.py, group G)
            if pinned is not None:
                assert (lrc, orc) == (pinned, DECOMPRESS_FAILED), (c["label"], cap, "liblz4", lrc, "oracle", orc)
                assert not have_ref() or reference_read(j["arc"], cap)[0] == pinned, (c["label"], cap, "reference")
                continue
            assert lrc == orc, (c["label"], cap, "liblz4", lrc, "oracle", orc)
            if orc in (OK, HASH_MISMATCH):
                assert lgot == ogot and np.array_equal(lbuf, obuf), (c["label"], cap, "bytes", lgot, ogot)
            if have_ref():
                rrc, rbuf = reference_read(j["arc"], cap)
                assert rrc == orc, (c["label"], cap, "reference", rrc, "oracle", orc)
                if orc in (OK, HASH_MISMATCH):
                    assert np.array_equal(rbuf, obuf), (c["label"], cap, "reference bytes")
        # a reader case is an intact entry; anything the reader must give up or never sees still has ONE verdict, the judges'
        if c["reader"]:
            assert j["rc"] == OK and j["produced"] == c["uncomp"], (c["label"], j["rc"], j["produced"])
        if c["group"] == "G":
            assert j["rc"] != OK, (c["label"], "the damage was not felt")
    assert seen >= 6


def test_every_block_stays_inside_liblz4s_input_rule():
    for c in CASES:
        if c["group"] == "L" or not c["walk"]:
            continue
        for stored, d, s, size, at in frame_blocks(c["frame"]):
            assert stored or s is None or in_liblz4s_rule(d, s), c["label"]
            if s is None and not stored:
                assert c["group"] == "G", c["label"]


def test_the_frames_sit_where_their_labels_say():
    checked = set()
    for c in CASES:
        k = c["claims"]
        if not c["walk"] or c["group"] in "GL":
            continue
        B = frame_blocks(c["frame"])
        label = c["label"]
        sizes, offs = [b[3] for b in B], [b[4] for b in B]
        assert len(B) == c["nblocks"], label
        if not ("beyond" in k or "sizes" in k and max(k["sizes"]) > 65536):
            assert sum(sizes) == c["uncomp"], label
        blk = B[k["block"]] if "block" in k else None
        if "sizes" in k:
            assert sizes == k["sizes"], (label, sizes)
        if "residues4" in k:
            mid = offs[1:]
            assert set(x % 4 for x in mid) >= set(k["residues4"]) and set(x % 32 for x in mid) >= set(k["residues32"]), (label, mid)
            assert {31, 32, 33} <= set(mid), (label, mid)
            assert set(sizes[1:-1]) >= {0, 1, 2, 3, 5, 31, 32, 33, 255, 256, 257, 65535, 65536}, label
            assert B[sizes.index(0)][1] == b"\x00", label
        if "blocks" in k:
            assert len(B) == k["blocks"], label
            if c["group"] == "B":
                assert len(set(sizes)) >= 10, label
        if "starts" in k:
            starts = [s[0] for s in blk[2]]
            assert set(k["starts"]) <= set(starts), (label, starts[:8])
        if "nseq" in k:
            assert len(blk[2]) == k["nseq"], (label, len(blk[2]))
        if "dense" in k:
            assert k["dense"][1] == k["dense"][0] + 1
            for i in k["dense"]:
                s = B[i][2]
                assert sizes[i] == 65536 and all(x[1] == 0 and x[4] == 4 for x in s[:-1]) and len(s) == 16383, label
                assert len(s) <= len(B[i][1]) // 3 + 2, label                                   # the record slots the walker reserves
        if "comp" in k:
            assert len(blk[1]) == k["comp"] and blk[2][-1][2] == k["last_lit_pos"], (label, len(blk[1]), blk[2][-1][2])
        if "reach0" in k:
            for i in k["reach0"]:
                assert any(ml and offs[i] + o + ll == off for o, ll, lp, off, ml, e in B[i][2]), (label, i)
        if "beyond" in k:
            i = k["beyond"]
            assert any(ml and offs[i] + o + ll + 1 == off for o, ll, lp, off, ml, e in B[i][2]), (label, i)
        if "far" in k:
            i, far = k["far"]
            o, ll, lp, off, ml, e = B[i][2][0]
            src = offs[i] + o + ll - off
            assert off == far and sum(1 for b in B if src < b[4] + b[3] and b[4] < src + ml and b[3] <= 30) >= 4, label
        if "offset" in k:
            o, ll, lp, off, ml, e = blk[2][0]
            assert off == k["offset"], label
            if c["independent"]:
                assert o + ll == off - (0 if c["reader"] else 1), label
            else:                                                       # the source begins in front of the block and ends in the match itself
                assert off > o + ll and off < ll + ml and blk[4] > 0, label
        if "offsets" in k:
            assert [b[2][0][3] for b in B] == k["offsets"] and all(b[2][0][4] >= 65500 for b in B), label
        if "stored" in k:
            assert [i for i, b in enumerate(B) if b[0]] == k["stored"], label
            hit = 0
            for b in B:
                for o, ll, lp, off, ml, e in (b[2] or []):
                    src = b[4] + o + ll - off
                    hit += ml != 0 and any(s[0] and src < s[4] + s[3] and s[4] < src + ml for s in B)
            assert hit >= 2, label
        if "boundaries4" in k:
            assert all(5 <= x <= 40 for x in sizes), label
            at = [offs[i] for i in range(A.CHUNK_BLOCKS, len(B), A.CHUNK_BLOCKS)]
            assert [x % 4 for x in at] == k["boundaries4"], (label, at)
            for i in range(A.CHUNK_BLOCKS, len(B), A.CHUNK_BLOCKS):
                s = B[i][2]
                assert s[0][0] == 0 and s[0][1] == 0 and s[0][3] == 1, label                   # the chunk's first byte: an offset-1 match
                assert s[1][0] + s[1][1] < s[1][3] < s[1][0] + s[1][1] + s[1][4], label         # a source on both sides of the boundary
            for i in range(1, len(B)):                                                           # one chain through every block
                assert any(ml and off >= o + ll for o, ll, lp, off, ml, e in B[i][2]) or i % A.CHUNK_BLOCKS == 0, (label, i)
        if "boundary" in k:
            assert offs[A.CHUNK_BLOCKS] == k["boundary"] and (k["boundary"] >> 10) // 64 == 1 and c["uncomp"] > 65536 + 1024, label
        if "chunk_blocks" in k:
            assert len(B) > A.CHUNK_BLOCKS * A.MAX_CHUNKS and -(-len(B) // A.MAX_CHUNKS) == k["chunk_blocks"] and all(b[0] and b[3] == 1 for b in B), label
        if "out" in k:
            assert c["uncomp"] == k["out"], label
        if "big" in k:
            assert len(B) <= 2 * -(-c["uncomp"] // 65536) + 8 and c["uncomp"] > 32 << 20 >> 1, label
            assert offs[A.CHUNK_BLOCKS] == 512 * 33792 and all(x == 33792 for x in sizes), label
        checked.update(k)
    assert checked >= {"sizes", "residues4", "blocks", "starts", "nseq", "dense", "comp", "reach0", "beyond", "far", "offset",
                       "offsets", "stored", "boundaries4", "boundary", "chunk_blocks", "out", "big"}, checked


def test_liblz4s_end_of_block_rule_is_pinned_as_it_stands():
    """group L: the oracle decodes every one of these frames; liblz4 refuses exactly those the table says it refuses, and where it accepts
    the bytes are equal"""
    seen = {True: 0, False: 0}
    for c in CASES:
        if c["group"] != "L":
            continue
        j = judged(c)
        lrc, lbuf, lgot = liblz4_read(c["frame"], c["uncomp"], c["cap"], j["hash"])
        assert j["rc"] == OK and j["produced"] == c["uncomp"], (c["label"], "oracle", j["rc"])
        want = c["claims"]["liblz4"]
        assert lrc == (OK if want else c["claims"].get("liblz4_status", DECOMPRESS_FAILED)), (c["label"], "liblz4", lrc)
        if want:
            assert np.array_equal(lbuf, j["out"]), c["label"]
        # the rule as the table's builders state it says the same, but for the one frame that shows liblz4's shortcut
        rule = all(stored or in_liblz4s_rule(d, s) for stored, d, s, size, at in frame_blocks(c["frame"]))
        assert rule == want or "shortcut" in c["label"] or "liblz4_status" in c["claims"], c["label"]
        seen[want] += 1
    assert seen[True] >= 4 and seen[False] >= 5, seen
