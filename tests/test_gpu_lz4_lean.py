"""The hot LZ4 kernel k_lz4_wave decodes PLAIN frames only (one frame, no checksums, no dictionary id) and finishes an entry only on
a clean end.  Frames whose header is not plain are sent to the general decoder by the classification (k_lz4_general); whatever the
lean kernel does not finish goes to the general decoder behind it (k_lz4_retry) unjudged.  What is right is decided by the oracle
and by the compiled reference's fixtures; the general GPU decoder alone (developer build, ZPK_LZ4_GENERAL=1) is the second witness
for the fields of the result record the oracle does not return."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests import zpk
from tests._libs import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def codec():
    return zpack_amd.Codec(0)


def _device_batch(codec, arc, offs, comp, uncomp, caps, hashes, flags, fill=0xA5):
    """one device batch of LZ4 entries -> (descriptors, results, output image, counters); the output image is pre-filled with `fill`"""
    import torch
    n = len(offs)
    desc = np.zeros(n, dtype=zpack_amd.DECODE_DESC)
    desc["src_offset"] = offs; desc["comp_size"] = comp; desc["uncomp_size"] = uncomp; desc["dst_capacity"] = caps
    desc["expect_hash"] = hashes; desc["method"] = dg.LZ4; desc["flags"] = flags
    slot = (np.maximum(np.array(caps, dtype=np.uint64), np.array(uncomp, dtype=np.uint64)) + np.uint64(255 + 64)) & ~np.uint64(255)
    desc["dst_offset"] = np.concatenate([[0], np.cumsum(slot)])[:-1]
    total = int(slot.sum()) + 256
    dev = torch.device("cuda:0")
    src = torch.from_numpy(np.frombuffer(bytes(arc), dtype=np.uint8).copy()).to(dev)
    dst = torch.full((total,), fill, dtype=torch.uint8, device=dev)
    ddesc = torch.from_numpy(desc.view(np.uint8)).to(dev)
    dres = torch.zeros(n * zpack_amd.DECODE_RESULT.itemsize, dtype=torch.uint8, device=dev)
    codec.decode_batch_device(src, ddesc, n, dst, dres)
    torch.cuda.synchronize()
    return desc, dres.cpu().numpy().view(zpack_amd.DECODE_RESULT).copy(), dst.cpu().numpy(), codec.decode_stats()


@pytest.mark.parametrize("mix,size,n", [(-1, 65536, 256), (dg.TEXT, 65536, 64), (dg.RECORDS, 65536, 64), (dg.RUNS, 65536, 64), (dg.RANDOM, 65536, 64),
                                        (-1, (1, 400), 300), (-1, (1000, 300000), 200), (dg.TEXT, 1 << 20, 8), (dg.RANDOM, (70000, 200000), 16),
                                        (dg.RECORDS, (65536 * 3, 65536 * 3 + 1), 8)])
def test_plain_frames_are_finished_by_the_lean_kernel(codec, mix, size, n):
    """every benchdata class, 1 byte ... 1 MiB, entries of several blocks and of stored blocks, XXH3 verify OFF: every byte equals
    the oracle's, nothing outside the entry's range is touched, and not one entry is handed to the general decoder"""
    o = oracle()
    lo, hi = size if isinstance(size, tuple) else (size, size)
    b = dg.Batch(n, lo, hi, method=dg.LZ4, level=0, seed=29, mix=mix)
    desc, r, out, st = _device_batch(codec, b.archive.tobytes(), b.offsets, b.comp_sizes, b.uncomp_sizes, b.uncomp_sizes, b.hashes,
                                     zpack_amd.DF_SKIP_HASH)
    assert st["lz4"] == n and st["lz4_handed_over"] == 0 and st["lz4_general"] == 0 and st["retried_lz4"] == 0, st
    assert (r["status"] == 0).all(), r[r["status"] != 0][:3]
    assert np.array_equal(r["produced"], b.uncomp_sizes) and np.array_equal(r["hash"], b.hashes)
    arc = b.archive.tobytes()
    for i in range(n):
        d = desc[i]
        a, k = int(d["dst_offset"]), int(d["uncomp_size"])
        rc, want, _, _ = o.entry_decode(arc, int(d["src_offset"]), int(d["comp_size"]), k, int(d["expect_hash"]), 2, k)
        bad = np.nonzero(out[a:a + k] != np.frombuffer(want, dtype=np.uint8)[:k])[0]
        assert rc == 0 and bad.size == 0, (i, "class", int(b.classes[i]), "first bad byte", int(bad[0]) if bad.size else -1, "of", k)
        nxt = int(desc[i + 1]["dst_offset"]) if i + 1 < n else len(out)
        assert (out[a + k:nxt] == 0xA5).all(), ("bytes past the entry were written", i)


# ---- frames the lean kernel must not judge ---------------------------------------------------------------------------------

def _hdr_len(f):
    return 7 + (8 if f[4] & 8 else 0) + (4 if f[4] & 1 else 0)


def _blocks(f):
    """(position of the block header, payload size) of every block of ONE well-formed frame, then the position of the end mark"""
    p, out = _hdr_len(f), []
    while True:
        bh = struct.unpack_from("<I", f, p)[0]
        if bh == 0:
            return out, p
        out.append((p, bh & 0x7FFFFFFF))
        p += 4 + (bh & 0x7FFFFFFF)


def _reheader(o, f, flg_or, extra=b""):
    """the frame with FLG bits set and `extra` descriptor bytes (a dictionary id) in front of a fresh header checksum"""
    h = _hdr_len(f)
    desc = bytes([f[4] | flg_or, f[5]]) + bytes(f[6:h - 1]) + extra
    return bytes(f[:4]) + desc + bytes([(o.xxh32(desc) >> 8) & 0xFF]) + bytes(f[h:])


def _with_content_checksum(o, f, plain):
    return _reheader(o, f, 0x04) + struct.pack("<I", o.xxh32(plain))


def _with_block_checksums(o, f):
    blocks, end = _blocks(f)
    body = b"".join(bytes(f[p:p + 4 + n]) + struct.pack("<I", o.xxh32(bytes(f[p + 4:p + 4 + n]))) for p, n in blocks)
    g = _reheader(o, f, 0x10)
    return g[:_hdr_len(g)] + body + bytes(f[end:])


def _has_plain_header(f):
    """what the classification sends to the lean kernel: magic, version 01, no checksums, no dictionary id, no reserved bits, block code >= 4"""
    f = bytes(f)
    return len(f) >= 11 and f[:4] == b"\x04\x22\x4d\x18" and (f[4] & 0xD7) == 0x40 and not (f[5] & 0x8F) and ((f[5] >> 4) & 7) >= 4


def _is_plain_and_whole(f):
    """what the lean kernel finishes: ONE plain frame whose blocks run exactly to an end mark at the end of the entry"""
    f = bytes(f)
    if not _has_plain_header(f):
        return False
    try:
        _, end = _blocks(f)
    except struct.error:
        return False
    return end + 4 == len(f)


def _foreign_cases(o, golden_dir):
    cases = []
    with open(os.path.join(golden_dir, "foreign_frames.json")) as fh:
        for c in json.load(fh):
            if c["label"].startswith("lz4f:"):
                cases.append(dict(label=c["label"], frame=bytes.fromhex(c["frame"]), uncomp=c["uncomp_size"], hash=c["hash"], cap=c["max_size"],
                                  rc=c["rc"], plain_xxh3=c["plain_xxh3"]))
    # built here, judged by the oracle: checksums on larger entries, a dictionary id, two frames, a skippable frame in front
    text = dg.fill(dg.TEXT, 43, 0, 150000).tobytes()
    recs = dg.fill(dg.RECORDS, 43, 1, 65536).tobytes()
    rnd = dg.fill(dg.RANDOM, 43, 2, 40000).tobytes()
    skip = struct.pack("<II", 0x184D2A50, 3) + b"abc"
    made = [("content checksum", _with_content_checksum(o, dg.compress(dg.LZ4, 0, text), text), text),
            ("content checksum, 64 KiB", _with_content_checksum(o, dg.compress(dg.LZ4, 0, recs), recs), recs),
            ("block checksums", _with_block_checksums(o, dg.compress(dg.LZ4, 0, text)), text),
            ("block checksums, stored block", _with_block_checksums(o, dg.compress(dg.LZ4, 0, rnd)), rnd),
            ("dictionary id", _reheader(o, dg.compress(dg.LZ4, 0, recs), 0x01, struct.pack("<I", 0x1234)), recs),
            ("two frames", dg.compress(dg.LZ4, 0, text[:70000]) + dg.compress(dg.LZ4, 0, text[70000:]), text),
            ("skippable frame in front", skip + dg.compress(dg.LZ4, 0, recs), recs),
            ("plain frame, trailing byte", dg.compress(dg.LZ4, 0, recs) + b"\x00", recs)]
    for label, frame, plain in made:
        arc = zpk.assemble([frame], [("f", 10, len(frame), len(plain), dg.xxh3(plain), 2)])
        rc, _, _, _ = o.entry_decode(arc, 10, len(frame), len(plain), dg.xxh3(plain), 2, len(plain))
        cases.append(dict(label=label, frame=frame, uncomp=len(plain), hash=dg.xxh3(plain), cap=len(plain), rc=rc, plain_xxh3=dg.xxh3(plain)))
    return cases


def _assemble(frames, uncomp, hashes):
    offs, off = [], 10
    for f in frames:
        offs.append(off); off += len(f)
    arc = zpk.assemble(frames, [("f%d" % i, offs[i], len(frames[i]), uncomp[i], hashes[i], 2) for i in range(len(frames))])
    return arc, offs


def test_frames_that_are_not_plain_go_to_the_general_decoder(codec, golden_dir):
    """the lz4f fixtures of the compiled reference and frames with checksums, a dictionary id, a second frame, a skippable frame in
    front, in ONE device batch: verdict and bytes are the fixture's / the oracle's; the classification sends exactly the entries without
    a plain header to k_lz4_general, and the hand-over counter is exactly the number of entries with a plain header that are not one
    whole plain frame"""
    o = oracle()
    cases = _foreign_cases(o, golden_dir)
    assert len(cases) >= 40
    frames = [c["frame"] for c in cases]
    arc, offs = _assemble(frames, [c["uncomp"] for c in cases], [c["hash"] for c in cases])
    desc, r, out, st = _device_batch(codec, arc, offs, [len(f) for f in frames], [c["uncomp"] for c in cases], [c["cap"] for c in cases],
                                     [c["hash"] for c in cases], 0)
    want_handed = want_general = 0
    for i, c in enumerate(cases):
        assert int(r[i]["status"]) == c["rc"], (c["label"], r[i], c["rc"])
        if c["rc"] == 0:
            a = int(desc[i]["dst_offset"])
            assert dg.xxh3(out[a:a + c["uncomp"]]) == c["plain_xxh3"], c["label"]
        on_hot_list = len(c["frame"]) > 0 and c["cap"] >= c["uncomp"] and len(c["frame"]) >= (c["uncomp"] >> 3)
        finished = _is_plain_and_whole(c["frame"]) and c["rc"] in (0, 15)
        want_general += 1 if on_hot_list and not _has_plain_header(c["frame"]) else 0
        want_handed += 1 if on_hot_list and _has_plain_header(c["frame"]) and not finished else 0
    assert want_general >= 10 and want_handed >= 10, (want_general, want_handed)      # both routes are exercised
    assert st["lz4_general"] == want_general and st["lz4_handed_over"] == want_handed and st["retried_lz4"] == 0, (st, want_general, want_handed)


# ---- damaged plain frames --------------------------------------------------------------------------------------------------

def _damaged_set():
    """plain frames damaged one byte at a time (seeded): header bytes, block headers, tokens, the end mark, truncation at every one of
    the last 16 bytes, dst_capacity / uncomp_size one short -> list of (frame, uncomp_size, dst_capacity, expect_hash)"""
    rng = np.random.default_rng(20251)
    out = []
    for cls, size in ((dg.TEXT, 9000), (dg.RECORDS, 70000), (dg.RANDOM, 20000), (dg.TEXT, 700), (dg.TEXT, 200000), (dg.RUNS, 3000), (dg.RECORDS, 65536)):
        plain = dg.fill(cls, 77, 0, size)
        h = dg.xxh3(plain)
        base = dg.compress(dg.LZ4, 0, plain)
        blocks, end = _blocks(base)
        assert end + 4 == len(base)

        def hit(pos, x):
            f = bytearray(base); f[pos] ^= x
            out.append((bytes(f), size, size, h))
        out.append((base, size, size, h))                                # undamaged
        for p in range(_hdr_len(base)):
            for x in (0x01, 0x80, int(rng.integers(1, 256))):
                hit(p, x)
        for p, n in blocks:
            for k in range(4):
                for x in (0x01, 0x80):
                    hit(p + k, x)
        for _ in range(40):                                              # tokens, offsets, literals
            p, n = blocks[int(rng.integers(0, len(blocks)))]
            hit(p + 4 + int(rng.integers(0, n)), int(rng.integers(1, 256)))
        for k in range(4):
            for x in (0x01, 0xFF):
                hit(end + k, x)
        for k in range(1, 17):
            out.append((base[:len(base) - k], size, size, h))
        out.append((base, size, size - 1, h))                            # dst_capacity one short
        out.append((base, size - 1, size - 1, h))                        # the entry claims one byte less than the frame holds
        out.append((base, size + 1, size + 1, h))                        # ... one byte more
    return out


_GENERAL_SCRIPT = r"""
import sys
import numpy as np
import torch
import zpack_amd
z = np.load(sys.argv[1])
codec = zpack_amd.Codec(0)
dev = torch.device("cuda:0")
desc = z["desc"].view(zpack_amd.DECODE_DESC)
n = len(desc)
src = torch.from_numpy(z["arc"]).to(dev)
dst = torch.zeros(int(z["total"]), dtype=torch.uint8, device=dev)
dres = torch.zeros(n * zpack_amd.DECODE_RESULT.itemsize, dtype=torch.uint8, device=dev)
codec.decode_batch_device(src, torch.from_numpy(desc.view(np.uint8)).to(dev), n, dst, dres)
torch.cuda.synchronize()
st = codec.decode_stats()
np.savez(sys.argv[2], res=dres.cpu().numpy(), handed=np.array([st["lz4_handed_over"], st["lz4"], st["lz4_long_runs"], st["lz4_general"]]))
"""


def test_damaged_plain_frames_get_the_general_decoders_record(codec, tmp_path):
    o = oracle()
    cases = _damaged_set()
    n = len(cases)
    assert n >= 500, n
    frames = [c[0] for c in cases]
    arc, offs = _assemble(frames, [c[1] for c in cases], [c[3] for c in cases])
    desc, r, out, st = _device_batch(codec, arc, offs, [len(f) for f in frames], [c[1] for c in cases], [c[2] for c in cases],
                                     [c[3] for c in cases], 0, fill=0)
    # (zero-filled output, like the oracle's buffer: a frame that ends early decodes "successfully" and the XXH3 verdict of
    # lib/zpack_read.c:466 then covers bytes nobody wrote)
    assert st["lz4_handed_over"] > 0, st                                  # or the hand-over was not tested
    # 1. the oracle decides the status (and the bytes of whatever still decodes)
    bad = []
    for i, (f, usz, cap, h) in enumerate(cases):
        rc, want, _, _ = o.entry_decode(arc, offs[i], len(f), usz, h, 2, cap)
        if int(r[i]["status"]) != rc:
            bad.append((i, int(r[i]["status"]), rc))
        elif rc in (0, 15):
            a = int(desc[i]["dst_offset"])
            if out[a:a + usz].tobytes() != want[:usz]:
                bad.append((i, "bytes"))
    assert bad == [], bad[:10]
    # 2. the whole record equals the general decoder's for the same batch (developer build: every LZ4 entry handed over unseen)
    so = os.path.join(os.path.dirname(zpack_amd.CODEC_SO), "dev", "libzpk_codec_dev.so")
    assert os.path.exists(so), "zpack_amd/dev/libzpk_codec_dev.so is built by zpack_amd.build.build_all()"
    inp, outp = str(tmp_path / "batch.npz"), str(tmp_path / "general.npz")
    np.savez(inp, desc=desc.view(np.uint8), arc=np.frombuffer(bytes(arc), dtype=np.uint8), total=np.array(len(out)))
    env = dict(os.environ, ZPACK_AMD_CODEC_SO=so, ZPK_LZ4_GENERAL="1", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", _GENERAL_SCRIPT, inp, outp], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=250, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    g = np.load(outp)
    general = g["res"].view(zpack_amd.DECODE_RESULT)
    handed, on_list, long_runs, not_plain = (int(x) for x in g["handed"])
    assert handed == on_list - long_runs - not_plain and handed > 0, g["handed"]      # the hook really took the hot kernel out
    for field in ("status", "detail", "produced", "hash"):
        diff = np.nonzero(r[field] != general[field])[0]
        assert diff.size == 0, (field, diff[:10], r[diff[:3]], general[diff[:3]])
