"""zpk_codec_decode_big_batch_device: a batch whose compressed bytes and output live in device memory and which holds large entries.
k_big_walk walks the block headers of every large LZ4 / Zstandard entry on the device (the compressed bytes never come to the host), the
entries worth it are decoded block-parallel, everything else by one launch of the one-wave kernels.  Checked here: status, produced,
hash and bytes are those of zpk_codec_decode_batch_device on the same descriptors, of the plaintext and of the real xxHash; nothing is
written outside an entry's slot; the counters say what was walked, accepted and decoded block-parallel.  Frames come from liblz4 /
libzstd (dg.compress), one from this codec's own writer in pieces, one is made by hand."""
import ctypes as C

import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from zpack_amd import METHOD_NONE, METHOD_ZSTD, METHOD_LZ4, OPT_ENC_SPLIT_MIN, OPT_DEC_SPLIT_MIN, OPT_STORED_SPAN_MIN

pytestmark = pytest.mark.gpu
K = 1 << 10
M = 1 << 20
SPLIT = 256 * K                         # the codec's default ZPK_OPT_DEC_SPLIT_MIN
GUARD = 0xEE


@pytest.fixture(scope="module")
def codec():
    c = zpack_amd.Codec(0)
    c.set_option(OPT_DEC_SPLIT_MIN, SPLIT)
    yield c
    c.close()


def _written_in_pieces(codec, plain):
    """An LZ4 entry as zpk_codec_encode_batch_host writes it in 512 KiB pieces (one frame)."""
    from tests.test_gpu_big_entries import _encode
    codec.set_option(OPT_ENC_SPLIT_MIN, 1 * M)
    try:
        res, pay = _encode(codec, [plain], [(METHOD_LZ4, 0)])
    finally:
        codec.set_option(OPT_ENC_SPLIT_MIN, 2 * M)
    return pay[0]


# label, method, level, class, size — the large shapes of the mixed batch (also run alone, one entry per call)
BIG = [("lz4 text 256K", METHOD_LZ4, 0, dg.TEXT, 256 * K), ("lz4 records 256K+1", METHOD_LZ4, 0, dg.RECORDS, 256 * K + 1),
       ("lz4 random 512K", METHOD_LZ4, 0, dg.RANDOM, 512 * K), ("lz4 runs 1M", METHOD_LZ4, 0, dg.RUNS, 1 * M),
       ("lz4 pieces 1M+5", METHOD_LZ4, -1, dg.TEXT, 1 * M + 5),
       ("zstd1 text 256K", METHOD_ZSTD, 1, dg.TEXT, 256 * K), ("zstd3 records 384K+1", METHOD_ZSTD, 3, dg.RECORDS, 384 * K + 1),
       ("zstd9 text 1M+321", METHOD_ZSTD, 9, dg.TEXT, 1 * M + 321), ("zstd random 512K", METHOD_ZSTD, 3, dg.RANDOM, 512 * K),
       ("zstd runs 1M", METHOD_ZSTD, 3, dg.RUNS, 1 * M)]
SMALL = [(m, 1 if m == METHOD_ZSTD else 0, n) for m in (METHOD_NONE, METHOD_LZ4, METHOD_ZSTD) for n in (4 * K, 64 * K)] + [(METHOD_NONE, 0, 300 * K)]


@pytest.fixture(scope="module")
def entries(codec):
    """(label, method, payload, plaintext, hash) of every entry of the mixed batch, made once"""
    out = []
    for i, (label, m, lv, cls, n) in enumerate(BIG):
        plain = dg.fill(cls, 501, i, n)
        pay = _written_in_pieces(codec, plain) if lv < 0 else np.frombuffer(dg.compress(m, lv, plain), dtype=np.uint8)
        out.append((label, m, np.array(pay, dtype=np.uint8), plain, dg.xxh3(plain)))
    for i, (m, lv, n) in enumerate(SMALL):
        plain = dg.fill(i % 2, 502, i, n)
        pay = plain if m == METHOD_NONE else np.frombuffer(dg.compress(m, lv, plain), dtype=np.uint8)
        out.append(("small %d/%d" % (m, n), m, np.array(pay, dtype=np.uint8), plain, dg.xxh3(plain)))
    return out


def _batch(items, tail=64):
    """items: (method, payload, comp_size, uncomp_size, hash, capacity).  The payloads lie back to back from byte 10 of the archive
    (no alignment), the output slots are 256-aligned with 256 guard bytes in front of, between and behind them."""
    offs, pos = [], 10
    for _, pay, _, _, _, _ in items:
        offs.append(pos); pos += len(pay)
    arc = np.zeros(pos + tail, dtype=np.uint8)
    for o, (_, pay, _, _, _, _) in zip(offs, items):
        arc[o:o + len(pay)] = pay
    d = np.zeros(len(items), dtype=zpack_amd.DECODE_DESC)
    at = 256
    for i, (m, pay, cs, us, h, cap) in enumerate(items):
        d[i]["src_offset"] = offs[i]; d[i]["comp_size"] = cs; d[i]["uncomp_size"] = us; d[i]["expect_hash"] = h
        d[i]["dst_offset"] = at; d[i]["dst_capacity"] = cap; d[i]["method"] = m
        at += ((cap + 255) & ~255) + 256
    return arc, d, at


def _run_both(codec, arc, d, dst_size):
    """-> (results, stats, output) of decode_big_batch_device and (results, output) of decode_batch_device, on fresh guard-filled outputs"""
    import torch
    dev = torch.device("cuda:0")
    src = torch.from_numpy(arc).to(dev)
    dst = torch.full((dst_size,), GUARD, dtype=torch.uint8, device=dev)
    r1 = codec.decode_big_batch_device(src, d, dst)
    st = codec.decode_stats()
    out1 = dst.cpu().numpy()
    dst2 = torch.full((dst_size,), GUARD, dtype=torch.uint8, device=dev)
    ddesc = torch.from_numpy(d.view(np.uint8)).to(dev)
    dres = torch.zeros(len(d) * zpack_amd.DECODE_RESULT.itemsize, dtype=torch.uint8, device=dev)
    codec.decode_batch_device(src, ddesc, len(d), dst2, dres)
    torch.cuda.synchronize()
    r0 = dres.cpu().numpy().view(zpack_amd.DECODE_RESULT).copy()
    return r1, st, out1, r0, dst2.cpu().numpy()


def _guards_intact(out, d):
    inside = np.zeros(len(out), dtype=bool)
    for x in d:
        inside[int(x["dst_offset"]):int(x["dst_offset"]) + int(x["dst_capacity"])] = True
    return bool((out[~inside] == GUARD).all())


def _same_verdicts(r1, r0, d, out1, out0, labels):
    for i in range(len(d)):
        key = (labels[i], r1[i], r0[i])
        assert int(r1["status"][i]) == int(r0["status"][i]) and int(r1["produced"][i]) == int(r0["produced"][i]) and int(r1["hash"][i]) == int(r0["hash"][i]), key
        if int(r0["status"][i]) in (0, 15):
            o, n = int(d["dst_offset"][i]), min(int(r0["produced"][i]), int(d["dst_capacity"][i]))
            assert np.array_equal(out1[o:o + n], out0[o:o + n]), key


def _block_count(pay, method):
    """blocks of ONE frame, by its block headers"""
    b = bytes(pay)
    if method == METHOD_LZ4:
        flg = b[4]; q = 7 + (8 if flg & 8 else 0); nb = 0
        while True:
            w = int.from_bytes(b[q:q + 4], "little"); q += 4
            if w == 0:
                return nb
            nb += 1; q += (w & 0x7FFFFFFF) + (4 if flg & 0x10 else 0)
    fhd = b[4]; single = (fhd >> 5) & 1; flag = fhd >> 6
    q = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if single else 0), 2, 4, 8)[flag]
    nb = 0
    while True:
        w = int.from_bytes(b[q:q + 3], "little"); nb += 1
        q += 3 + (1 if (w >> 1) & 3 == 1 else w >> 3)
        if w & 1:
            return nb


def test_mixed_batch_equals_the_one_wave_path(codec, entries):
    """Large entries at the edges of the rules — the smallest sizes taken, stored / raw / RLE blocks, Repeat_Mode tables, an entry written
    in pieces — among small and stored ones, in ONE call."""
    items = [(m, pay, len(pay), len(plain), h, len(plain)) for _, m, pay, plain, h in entries]
    labels = [e[0] for e in entries]
    arc, d, total = _batch(items)
    r1, st, out1, r0, out0 = _run_both(codec, arc, d, total)
    nbig = sum(1 for _, m, _, plain, _ in entries if m != METHOD_NONE and len(plain) >= SPLIT)
    assert nbig == len(BIG)
    assert (st["device_walked"], st["device_walk_accepted"]) == (nbig, nbig), st
    for i, (label, m, pay, plain, h) in enumerate(entries):
        assert int(r1["status"][i]) == 0 and int(r1["produced"][i]) == len(plain) and int(r1["hash"][i]) == h, (label, r1[i])
        o = int(d["dst_offset"][i])
        assert np.array_equal(out1[o:o + len(plain)], plain), label
    _same_verdicts(r1, r0, d, out1, out0, labels)
    assert _guards_intact(out1, d) and _guards_intact(out0, d)


@pytest.mark.parametrize("which", [i for i, b in enumerate(BIG) if b[3] != dg.RANDOM], ids=[b[0] for b in BIG if b[3] != dg.RANDOM])
def test_one_large_entry_per_call_goes_block_parallel(codec, entries, which):
    label, m, pay, plain, h = entries[which]
    arc, d, total = _batch([(m, pay, len(pay), len(plain), h, len(plain))])
    r1, st, out1, r0, out0 = _run_both(codec, arc, d, total)
    assert (st["frame_parallel_entries"], st["frame_parallel_frames"]) == (1, _block_count(pay, m)), (label, st)
    assert (st["device_walked"], st["device_walk_accepted"]) == (1, 1), st
    codec.set_option(OPT_DEC_SPLIT_MIN, 0)
    try:
        r2, st2, out2, _, _ = _run_both(codec, arc, d, total)
    finally:
        codec.set_option(OPT_DEC_SPLIT_MIN, SPLIT)
    assert (st2["frame_parallel_entries"], st2["frame_parallel_frames"], st2["device_walked"]) == (0, 0, 0), (label, st2)
    for r in (r1, r2, r0):
        assert int(r["status"][0]) == 0 and int(r["produced"][0]) == len(plain) and int(r["hash"][0]) == h, (label, r)
    for out in (out1, out2, out0):
        assert np.array_equal(out[256:256 + len(plain)], plain) and _guards_intact(out, d), label


def _block_header_offsets(pay, method):
    b = bytes(pay); offs = []
    if method == METHOD_LZ4:
        q = 7 + (8 if b[4] & 8 else 0)
        while True:
            w = int.from_bytes(b[q:q + 4], "little")
            if w == 0:
                return offs
            offs.append(q); q += 4 + (w & 0x7FFFFFFF)
    fhd = b[4]; single = (fhd >> 5) & 1
    q = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if single else 0), 2, 4, 8)[fhd >> 6]
    while True:
        w = int.from_bytes(b[q:q + 3], "little"); offs.append(q)
        q += 3 + (1 if (w >> 1) & 3 == 1 else w >> 3)
        if w & 1:
            return offs


def test_damaged_copies_get_the_one_wave_verdicts(codec):
    """About forty copies of a 512 KiB LZ4 text entry and a 512 KiB Zstandard-3 text entry, each with one mutation, in one call: status,
    produced and hash are decode_batch_device's entry by entry, the bytes too where the status is OK or hash mismatch, the guards stay."""
    items, labels = [], []
    for m, lv in ((METHOD_LZ4, 0), (METHOD_ZSTD, 3)):
        plain = dg.fill(dg.TEXT, 503, m, 512 * K)
        good = np.array(np.frombuffer(dg.compress(m, lv, plain), dtype=np.uint8))
        h, n, cs = dg.xxh3(plain), len(plain), len(good)
        hdrs = _block_header_offsets(good, m)
        body = hdrs[len(hdrs) // 2] + 40

        def flip(at, bit=0x10):
            b = good.copy(); b[at] ^= bit
            return b
        variants = [("intact", good, cs, n, h, n), ("frame header", flip(4, 0x20), cs, n, h, n), ("frame header 2", flip(5, 0x01), cs, n, h, n),
                    ("first block header", flip(hdrs[0]), cs, n, h, n), ("first block header +1", flip(hdrs[0] + 1, 0x01), cs, n, h, n),
                    ("middle block header", flip(hdrs[len(hdrs) // 2]), cs, n, h, n), ("middle block header +2", flip(hdrs[len(hdrs) // 2] + 2, 0x40), cs, n, h, n),
                    ("last block header", flip(hdrs[-1]), cs, n, h, n), ("last block header bit 0", flip(hdrs[-1], 0x01), cs, n, h, n),
                    ("block body", flip(body), cs, n, h, n), ("block body 2", flip(hdrs[1] + 9, 0x04), cs, n, h, n), ("block body 3", flip(hdrs[-1] + 30, 0x80), cs, n, h, n),
                    ("last byte", flip(cs - 1, 0x02), cs, n, h, n),
                    ("comp_size - 1", good, cs - 1, n, h, n), ("comp_size + 1", good, cs + 1, n, h, n),
                    ("uncomp_size + 1", good, cs, n + 1, h, n + 1), ("uncomp_size - 1", good, cs, n - 1, h, n), ("uncomp_size + 1, capacity as it was", good, cs, n + 1, h, n),
                    ("hash", good, cs, n, h ^ 1, n), ("capacity", good, cs, n, h, n - 1)]
        for label, pay, c, u, hh, cap in variants:
            items.append((m, pay, c, u, hh, cap)); labels.append("%d %s" % (m, label))
    # the last entry ends where the archive ends: the guard `offset + comp_size < file_size` (lib/zpack_read.c:331) fires
    plain = dg.fill(dg.TEXT, 503, METHOD_LZ4, 512 * K)
    good = np.array(np.frombuffer(dg.compress(METHOD_LZ4, 0, plain), dtype=np.uint8))
    items.append((METHOD_LZ4, good, len(good), len(plain), dg.xxh3(plain), len(plain))); labels.append("at the archive's end")
    arc, d, total = _batch(items, tail=0)
    assert int(d["src_offset"][-1] + d["comp_size"][-1]) == len(arc)
    r1, st, out1, r0, out0 = _run_both(codec, arc, d, total)
    print(st, [(l, int(s)) for l, s in zip(labels, r1["status"])])
    _same_verdicts(r1, r0, d, out1, out0, labels)
    assert _guards_intact(out1, d) and _guards_intact(out0, d)
    by = dict(zip(labels, range(len(labels))))
    for m in (METHOD_LZ4, METHOD_ZSTD):
        assert int(r1["status"][by["%d intact" % m]]) == 0 and int(r1["status"][by["%d hash" % m]]) == 15
        assert int(r1["status"][by["%d capacity" % m]]) != 0
    assert int(r1["status"][-1]) != 0
    assert 0 < st["device_walk_accepted"] < st["device_walked"] < len(items), st
    # In a batch of forty the estimate leaves every copy to the one-wave launch.  Each copy alone in a call: the ones the walk accepts go
    # block-parallel, so that path meets the damage too — a flipped body, a wrong hash, a size off by one — and hands back what it must
    par = {}
    for i, it in enumerate(items[:-1]):
        arc1, d1, total1 = _batch([it])
        q1, st1, o1, q0, o0 = _run_both(codec, arc1, d1, total1)
        _same_verdicts(q1, q0, d1, o1, o0, [labels[i]])
        assert int(q1["status"][0]) == int(r1["status"][i]) and _guards_intact(o1, d1), labels[i]
        par[labels[i]] = (st1["device_walk_accepted"], st1["frame_parallel_entries"])
    print(par)
    assert par["2 intact"] == (1, 1) and par["1 intact"] == (1, 1)
    assert par["2 hash"] == (1, 1)                            # LZ4 blocks decode or fail: a wrong XXH3 is the entry's verdict (15), bytes delivered
    assert par["1 hash"] == (1, 0)                            # Zstandard: a wrong XXH3 may be a damaged block: the one-wave decoder's verdict
    assert par["2 block body"][0] == 1 and par["1 block body"][0] == 1 and par["2 comp_size + 1"] == (0, 0) and par["2 capacity"] == (0, 0)


def test_frame_with_more_blocks_than_the_table_is_declined(codec):
    """A valid 256 KiB LZ4 frame of 16-byte stored blocks: 16384 blocks against a table of 2 * 4 + 8.  The walk declines it without writing
    behind its table; the one-wave decoder decodes it."""
    plain = dg.fill(dg.TEXT, 504, 0, 256 * K)
    nb = len(plain) // 16
    blocks = np.zeros((nb, 20), dtype=np.uint8)
    blocks[:, 0] = 16; blocks[:, 3] = 0x80                                   # block size 16, not compressed
    blocks[:, 4:] = plain.reshape(nb, 16)
    frame = np.concatenate([np.array([0x04, 0x22, 0x4D, 0x18, 0x40, 0x40, 0xC0], dtype=np.uint8), blocks.reshape(-1), np.zeros(4, dtype=np.uint8)])
    h = dg.xxh3(plain)
    # next to it, as a check on the frame made by hand: the same plaintext in 4 stored blocks of 64 KiB, which the walk accepts
    b4 = np.zeros((4, 4 + 65536), dtype=np.uint8)
    b4[:, 2] = 0x01; b4[:, 3] = 0x80; b4[:, 4:] = plain.reshape(4, 65536)
    frame4 = np.concatenate([frame[:7], b4.reshape(-1), np.zeros(4, dtype=np.uint8)])
    arc, d, total = _batch([(METHOD_LZ4, frame, len(frame), len(plain), h, len(plain))])
    r1, st, out1, r0, out0 = _run_both(codec, arc, d, total)
    assert (st["device_walked"], st["device_walk_accepted"], st["frame_parallel_entries"]) == (1, 0, 0), st
    assert int(r1["status"][0]) == 0 and int(r1["hash"][0]) == h and np.array_equal(out1[256:256 + len(plain)], plain), r1
    _same_verdicts(r1, r0, d, out1, out0, ["16-byte blocks"])
    assert _guards_intact(out1, d)
    arc, d, total = _batch([(METHOD_LZ4, frame4, len(frame4), len(plain), h, len(plain))])
    r1, st, out1, r0, out0 = _run_both(codec, arc, d, total)
    assert (st["device_walked"], st["device_walk_accepted"]) == (1, 1), st
    assert int(r1["status"][0]) == 0 and np.array_equal(out1[256:256 + len(plain)], plain), r1


def test_arguments_and_a_batch_without_candidates(codec, entries):
    import torch
    dev = torch.device("cuda:0")
    small = [e for e in entries if e[0].startswith("small")]
    items = [(m, pay, len(pay), len(plain), h, len(plain)) for _, m, pay, plain, h in small]
    arc, d, total = _batch(items)
    r1, st, out1, r0, out0 = _run_both(codec, arc, d, total)
    assert (st["device_walked"], st["device_walk_accepted"], st["frame_parallel_entries"]) == (0, 0, 0), st
    assert (r1["status"] == 0).all() and np.array_equal(r1, r0) and np.array_equal(out1, out0)
    for i, (_, m, pay, plain, h) in enumerate(small):
        assert np.array_equal(out1[int(d["dst_offset"][i]):int(d["dst_offset"][i]) + len(plain)], plain) and int(r1["hash"][i]) == h
    src = torch.from_numpy(arc).to(dev)
    dst = torch.full((total,), GUARD, dtype=torch.uint8, device=dev)
    assert len(codec.decode_big_batch_device(src, d[:0], dst)) == 0                          # n == 0: ZPK_OK
    L = codec.L
    L.zpk_codec_decode_big_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    res = np.zeros(len(d), dtype=zpack_amd.DECODE_RESULT)
    assert L.zpk_codec_decode_big_batch_device(codec.h, src.data_ptr(), src.numel(), None, 0, dst.data_ptr(), dst.numel(), None) == 0
    assert L.zpk_codec_decode_big_batch_device(codec.h, src.data_ptr(), src.numel(), None, len(d), dst.data_ptr(), dst.numel(), res.ctypes.data) == -2
    assert L.zpk_codec_decode_big_batch_device(codec.h, src.data_ptr(), src.numel(), d.ctypes.data, len(d), dst.data_ptr(), dst.numel(), None) == -2
    assert L.zpk_codec_decode_big_batch_device(None, src.data_ptr(), src.numel(), d.ctypes.data, len(d), dst.data_ptr(), dst.numel(), res.ctypes.data) == -2
    torch.cuda.synchronize()
    assert bool((dst.cpu().numpy() == GUARD).all())


def test_pinned_blocks_grow_and_are_reused_at_a_smaller_need():
    """The codec's three read-side pinned blocks — the walk's tables, the stored spans' table, the bytes of one entry for the host's walk —
    each grown, grown again and then used at a smaller need, on ONE codec with both thresholds at 64 KiB: decode_big_batch_device with 1,
    48 and 1 entries of 96 KiB (LZ4 text, Zstandard text, stored in turn), then decode_big_device with a 96 KiB LZ4 entry, a 1 MiB one, the
    96 KiB one again and a 96 KiB stored one.  After every call: status, produced, hash and bytes are decode_batch_device's on the same
    descriptors, the guards stand, and the counters are the counts of the call's own descriptors."""
    import torch
    dev = torch.device("cuda:0")
    n = 96 * K
    kinds = [(METHOD_LZ4, 0), (METHOD_ZSTD, 1), (METHOD_NONE, 0)]

    def item(i, size=n):
        m, lv = kinds[i % 3]
        plain = dg.fill(dg.TEXT, 505, i, size)
        pay = plain if m == METHOD_NONE else np.array(np.frombuffer(dg.compress(m, lv, plain), dtype=np.uint8))
        return (m, pay, len(pay), size, dg.xxh3(plain), size), plain

    def accepted(m, pay):                                  # host_walk.h: a frame of at least 4 LZ4 blocks / 2 Zstandard blocks
        return m != METHOD_NONE and _block_count(pay, m) >= (4 if m == METHOD_LZ4 else 2)

    made = [item(i) for i in range(48)]
    big, big_plain = item(48, 1 * M)                       # (48 % 3 == 0: LZ4)
    c = zpack_amd.Codec(0)
    try:
        c.set_option(OPT_DEC_SPLIT_MIN, 64 * K)
        c.set_option(OPT_STORED_SPAN_MIN, 64 * K)
        for count in (1, 48, 1):
            items, plains = [x[0] for x in made[:count]], [x[1] for x in made[:count]]
            arc, d, total = _batch(items)
            r1, st, out1, r0, out0 = _run_both(c, arc, d, total)
            print(count, st)
            _same_verdicts(r1, r0, d, out1, out0, ["%d of %d" % (i, count) for i in range(count)])
            for i, plain in enumerate(plains):
                o = int(d["dst_offset"][i])
                assert int(r1["status"][i]) == 0 and int(r1["produced"][i]) == n and int(r1["hash"][i]) == items[i][4], (count, i, r1[i])
                assert np.array_equal(out1[o:o + n], plain), (count, i)
            assert _guards_intact(out1, d) and _guards_intact(out0, d)
            walked = sum(1 for it in items if it[0] != METHOD_NONE)
            assert st["device_walked"] == walked and st["device_walk_accepted"] == sum(1 for it in items if accepted(it[0], it[1])), (count, st)
            assert st["stored_span_entries"] == count - walked, (count, st)
        singles = [(made[0][0], made[0][1]), (big, big_plain), (made[0][0], made[0][1]), (made[2][0], made[2][1])]
        for k, (it, plain) in enumerate(singles):
            arc, d, total = _batch([it])
            src = torch.from_numpy(arc).to(dev)
            dst = torch.full((total,), GUARD, dtype=torch.uint8, device=dev)
            r = c.decode_big_device(src, d, dst)
            st = c.decode_stats()
            out1 = dst.cpu().numpy()
            print(k, st)
            _, _, _, r0, out0 = _run_both(c, arc, d, total)
            _same_verdicts(np.array([r], dtype=zpack_amd.DECODE_RESULT), r0, d, out1, out0, ["single %d" % k])
            assert int(r["status"]) == 0 and int(r["produced"]) == len(plain) and int(r["hash"]) == it[4], (k, r)
            assert np.array_equal(out1[256:256 + len(plain)], plain) and _guards_intact(out1, d) and _guards_intact(out0, d), k
            assert (st["device_walked"], st["device_walk_accepted"]) == (0, 0), (k, st)              # this call walks on the host
            assert st["stored_span_entries"] == (1 if it[0] == METHOD_NONE else 0), (k, st)
            assert st["frame_parallel_entries"] == (1 if accepted(it[0], it[1]) else 0), (k, st)
    finally:
        c.close()
