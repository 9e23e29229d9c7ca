"""Large STORED entries of a device-resident call, copied and hashed by the whole chip (k_stored_span + k_xxh3_chain, round 17) through
zpk_codec_decode_big_batch_device and zpk_codec_decode_big_device.  Every test judges four things: status / detail / produced / hash
against zpk_codec_decode_batch_device on the same descriptors, the bytes against the plaintext, the hash against the real xxHash
(dg.xxh3), and the 0xEE guard bytes around every slot — the slot here is [dst_offset, dst_offset + uncomp_size) for a finished entry,
and the destination offsets are NOT 256-aligned.  The counters (decode_stats: stored_span_entries, stored_span_groups) say which path
an entry took."""
import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from zpack_amd import METHOD_NONE, METHOD_ZSTD, METHOD_LZ4, OPT_DEC_SPLIT_MIN, OPT_STORED_SPAN_MIN, DF_SKIP_HASH
from tests.test_gpu_big_batch_device import _run_both

pytestmark = pytest.mark.gpu
K = 1 << 10
M = 1 << 20
GUARD = 0xEE
DEFAULT_MIN = 256 * K
EDGE = [1000, 1024, 1025, 1026, 2048, 2049, 3073, 4097, 5121, 4113, 65536, 65537, 66560, 66561, 131073, 1 * M + 321]
SKEW = [0, 1, 7, 15, 16 + 3, 31, 32 + 5, 64, 64 + 9, 127, 128 + 11, 255, 2, 17, 33, 100]      # distance of a slot from a 256-byte boundary


def _groups(n):
    """groups of 64 full 1 KiB blocks of a span of n bytes; the block with the last byte is the chain's"""
    return (((n - 1) >> 10) + 63) // 64


@pytest.fixture(scope="module")
def codec():
    c = zpack_amd.Codec(0)
    c.set_option(OPT_DEC_SPLIT_MIN, DEFAULT_MIN)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain():
    """8 MiB + 3 of bytes that do not repeat: every stored payload of this file is a slice of it"""
    return dg.fill(dg.RANDOM, 1701, 0, 8 * M + 3)


def _stored(plain, n, at=0):
    p = plain[at:at + n]
    return (METHOD_NONE, p, n, n, dg.xxh3(p), n, 0)


def _batch(items, tail=64, dst_size=None):
    """items: (method, payload, comp_size, uncomp_size, hash, capacity, flags).  Payloads back to back from archive byte 10 (every source
    alignment occurs); slot i starts SKEW[i % 16] bytes behind a 256-byte boundary, at least 256 guard bytes between two slots."""
    offs, pos = [], 10
    for it in items:
        offs.append(pos); pos += len(it[1])
    arc = np.zeros(pos + tail, dtype=np.uint8)
    for o, it in zip(offs, items):
        arc[o:o + len(it[1])] = it[1]
    d = np.zeros(len(items), dtype=zpack_amd.DECODE_DESC)
    at = 256
    for i, (m, pay, cs, us, h, cap, fl) in enumerate(items):
        d[i]["src_offset"] = offs[i]; d[i]["comp_size"] = cs; d[i]["uncomp_size"] = us; d[i]["expect_hash"] = h
        d[i]["dst_offset"] = at + SKEW[i % len(SKEW)]; d[i]["dst_capacity"] = cap; d[i]["method"] = m; d[i]["flags"] = fl
        at += ((SKEW[i % len(SKEW)] + max(cap, us) + 255) & ~255) + 256
    return arc, d, (at if dst_size is None else dst_size)


def _guards(out, d, r):
    """everything outside the bytes an entry may write is still 0xEE: uncomp_size bytes for a finished entry, the capacity otherwise"""
    inside = np.zeros(len(out), dtype=bool)
    for x, y in zip(d, r):
        n = int(x["uncomp_size"]) if int(y["status"]) in (0, 15) else int(x["dst_capacity"])
        o = int(x["dst_offset"])
        inside[o:min(o + n, len(out))] = True
    return bool((out[~inside] == GUARD).all())


def _judge(r1, r0, d, out1, out0, plains):
    """plains[i]: the plaintext of an entry that must come out (status 0 or 15), None for one that must fail as the one-wave path says"""
    for i in range(len(d)):
        key = (i, r1[i], r0[i])
        for f in ("status", "detail", "produced", "hash"):
            assert int(r1[f][i]) == int(r0[f][i]), (f,) + key
        if plains[i] is not None:
            p, o = plains[i], int(d["dst_offset"][i])
            assert int(r1["status"][i]) in (0, 15) and int(r1["produced"][i]) == len(p) and int(r1["detail"][i]) == 0, key
            assert int(r1["hash"][i]) == dg.xxh3(p), key
            assert np.array_equal(out1[o:o + len(p)], p) and np.array_equal(out0[o:o + len(p)], p), key
        else:
            assert int(r1["status"][i]) not in (0, 15), key
    assert _guards(out1, d, r1) and _guards(out0, d, r0)


def _edge_items(plain):
    items, at = [], 0
    for k, n in enumerate(EDGE):
        items.append(_stored(plain, n, at)); at += n + 13
    # one entry with trailing bytes in the archive that belong to it but are not plaintext: only uncomp_size bytes may be written
    k = EDGE.index(4113)
    m, p, cs, us, h, cap, fl = items[k]
    items[k] = (m, np.concatenate([p, np.full(5, 0x5A, dtype=np.uint8)]), cs + 5, us, h, cap, fl)
    return items


def test_edge_lengths_alignments_and_trailing_bytes(codec, plain):
    """1 to 5 blocks of the four-deep load loop, a full group with a 1-byte and with a 1024-byte tail, a second group of one block, 17 groups;
    1000 and 1024 bytes have no full block and stay with k_stored."""
    items = _edge_items(plain)
    arc, d, total = _batch(items)
    assert len({int(x) % 16 for x in d["src_offset"]}) >= 10 and len({int(x) % 256 for x in d["dst_offset"]}) == 16
    codec.set_option(OPT_STORED_SPAN_MIN, 1025)
    try:
        r1, st, out1, r0, out0 = _run_both(codec, arc, d, total)
    finally:
        codec.set_option(OPT_STORED_SPAN_MIN, DEFAULT_MIN)
    print(st)
    _judge(r1, r0, d, out1, out0, [it[1][:it[3]] for it in items])
    assert (r1["status"] == 0).all()
    assert st["stored_span_entries"] == 14 and st["stored_span_groups"] == sum(_groups(n) for n in EDGE if n >= 1025), st
    assert st["stored"] == 2 and (st["frame_parallel_entries"], st["frame_parallel_frames"], st["device_walked"]) == (0, 0, 0), st


def test_option_zero_leaves_every_entry_to_the_one_wave_kernel(codec, plain):
    items = _edge_items(plain)
    arc, d, total = _batch(items)
    codec.set_option(OPT_STORED_SPAN_MIN, 1025)
    try:
        r1, st1, out1, _, _ = _run_both(codec, arc, d, total)
        codec.set_option(OPT_STORED_SPAN_MIN, 0)
        r2, st2, out2, r0, out0 = _run_both(codec, arc, d, total)
    finally:
        codec.set_option(OPT_STORED_SPAN_MIN, DEFAULT_MIN)
    assert (st2["stored_span_entries"], st2["stored_span_groups"]) == (0, 0) and st2["stored"] == len(EDGE), st2
    assert st1["stored_span_entries"] == 14 and st1["stored"] == 2, st1
    _judge(r2, r0, d, out2, out0, [it[1][:it[3]] for it in items])
    assert np.array_equal(r1, r2) and np.array_equal(out1, out2)


def test_many_spans_in_one_launch(codec, plain):
    """257 spans of 1 to 11 blocks: the search over part_base finds every group's span"""
    sizes = [1025 + 37 * i for i in range(257)]
    items, at = [], 0
    for n in sizes:
        items.append(_stored(plain, n, at)); at += n + 1
    arc, d, total = _batch(items)
    codec.set_option(OPT_STORED_SPAN_MIN, 1025)
    try:
        r1, st, out1, r0, out0 = _run_both(codec, arc, d, total)
    finally:
        codec.set_option(OPT_STORED_SPAN_MIN, DEFAULT_MIN)
    _judge(r1, r0, d, out1, out0, [it[1] for it in items])
    assert (r1["status"] == 0).all()
    assert st["stored_span_entries"] == 257 and st["stored_span_groups"] == sum(_groups(n) for n in sizes) == 257 and st["stored"] == 0, st


def test_verdicts_are_the_one_wave_paths(codec, plain):
    n = 300 * K
    p = plain[:n]
    h = dg.xxh3(p)
    items = [(METHOD_NONE, p, n, n, h, n, 0),                       # 0 intact
             (METHOD_NONE, p, n, n, h ^ 1, n, 0),                   # 1 wrong expect_hash: 15, bytes delivered
             (METHOD_NONE, p, n, n, h ^ 1, n, DF_SKIP_HASH),        # 2 the same, hash not judged: 0
             (METHOD_NONE, p, n, n + 1, h, n + 1, 0),               # 3 uncomp_size = comp_size + 1: FILE_SIZE_INVALID
             (METHOD_NONE, p, n, n, h, n - 1, 0),                   # 4 dst_capacity = uncomp_size - 1: BUFFER_TOO_SMALL
             (METHOD_NONE, p, n, n, h, n, 0),                       # 5 a slot that reaches past dst_size
             (METHOD_NONE, p, n, n, h, n, 0)]                       # 6 ends exactly where the archive ends: FILE_OFFSET_INVALID
    arc, d, total = _batch(items, tail=0)
    assert int(d["src_offset"][6] + d["comp_size"][6]) == len(arc)
    d[5]["dst_offset"], d[6]["dst_offset"] = int(d["dst_offset"][6]), int(d["dst_offset"][5])      # entry 5 gets the last slot ...
    total = int(d["dst_offset"][5]) + n - 1                          # ... which ends one byte behind dst
    r1, st, out1, r0, out0 = _run_both(codec, arc, d, total)
    print(st, r1)
    _judge(r1, r0, d, out1, out0, [p, p, p, None, None, None, None])
    assert [int(x) for x in r1["status"]] == [0, 15, 0, 18, 12, 12, 16], r1
    assert int(r1["hash"][1]) == h and int(r1["hash"][2]) == h
    assert (st["stored_span_entries"], st["stored_span_groups"]) == (3, 3 * _groups(n)), st


@pytest.fixture(scope="module")
def mixed(plain):
    items, plains = [], []
    for m, lv, n in ((METHOD_LZ4, 0, 1 * M), (METHOD_ZSTD, 3, 512 * K)):                          # both go block-parallel
        t = dg.fill(dg.TEXT, 1702, m, n)
        pay = np.frombuffer(dg.compress(m, lv, t), dtype=np.uint8)
        items.append((m, pay, len(pay), n, dg.xxh3(t), n, 0)); plains.append(t)
    for i, (m, n) in enumerate([(m, n) for m in (METHOD_NONE, METHOD_LZ4, METHOD_ZSTD) for n in (4 * K, 64 * K + 5)]):
        t = dg.fill(i % 2, 1703, i, n)
        pay = t if m == METHOD_NONE else np.frombuffer(dg.compress(m, 1 if m == METHOD_ZSTD else 0, t), dtype=np.uint8)
        items.append((m, pay, len(pay), n, dg.xxh3(t), n, 0)); plains.append(t)
    for n in (300 * K, 1 * M + 5, 8 * M + 3):                                                     # several workgroups per span
        items.append(_stored(plain, n)); plains.append(plain[:n])
    return items, plains


def test_mixed_batch_beside_the_block_parallel_entries(codec, mixed):
    items, plains = mixed
    arc, d, total = _batch(items)
    r1, st1, out1, r0, out0 = _run_both(codec, arc, d, total)
    codec.set_option(OPT_STORED_SPAN_MIN, 0)
    try:
        r2, st2, out2, _, _ = _run_both(codec, arc, d, total)
    finally:
        codec.set_option(OPT_STORED_SPAN_MIN, DEFAULT_MIN)
    print(st1, st2)
    _judge(r1, r0, d, out1, out0, plains)
    assert (r1["status"] == 0).all() and np.array_equal(r1, r2) and np.array_equal(out1, out2)
    assert (st1["stored_span_entries"], st1["stored_span_groups"]) == (3, _groups(300 * K) + _groups(1 * M + 5) + _groups(8 * M + 3)), st1
    assert (st2["stored_span_entries"], st2["stored_span_groups"]) == (0, 0), st2
    for key in ("device_walked", "device_walk_accepted", "frame_parallel_entries", "frame_parallel_frames"):
        assert st1[key] == st2[key], (key, st1, st2)
    assert st1["frame_parallel_entries"] == 2 and st1["stored"] == 2 and st2["stored"] == 5, (st1, st2)


def test_decode_big_device_takes_one_stored_entry(codec, plain):
    import torch
    dev = torch.device("cuda:0")
    n = 1 * M + 5
    arc, d, total = _batch([_stored(plain, n, 3)])
    d[0]["dst_offset"] = 256 + 77
    src = torch.from_numpy(arc).to(dev)
    out = {}
    for name, opt in (("on", DEFAULT_MIN), ("off", 0)):
        codec.set_option(OPT_STORED_SPAN_MIN, opt)
        try:
            dst = torch.full((total,), GUARD, dtype=torch.uint8, device=dev)
            r = codec.decode_big_device(src, d, dst)
            out[name] = (r.copy(), codec.decode_stats(), dst.cpu().numpy())
        finally:
            codec.set_option(OPT_STORED_SPAN_MIN, DEFAULT_MIN)
    (r1, st1, o1), (r2, st2, o2) = out["on"], out["off"]
    _, _, _, r0, o0 = _run_both(codec, arc, d, total)
    r1a, r2a = np.array([r1], dtype=zpack_amd.DECODE_RESULT), np.array([r2], dtype=zpack_amd.DECODE_RESULT)
    _judge(r1a, r0, d, o1, o0, [plain[3:3 + n]])
    _judge(r2a, r0, d, o2, o0, [plain[3:3 + n]])
    assert int(r1["status"]) == 0 and np.array_equal(o1, o2)
    assert (st1["stored_span_entries"], st1["stored_span_groups"], st1["stored"]) == (1, _groups(n), 0), st1
    assert (st2["stored_span_entries"], st2["stored_span_groups"], st2["stored"]) == (0, 0, 1), st2
