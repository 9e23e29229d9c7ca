"""zpk_codec_encode_big_device: large entries that already lie in DEVICE memory are compressed in 512 KiB pieces, one wave each, and their
frames are put together on the device (k_big_gather, k_big_close) — what zpk_codec_encode_batch_host does with a host in the middle.
Checked here: the slots and results are byte for byte those of the host path (and of zpk_codec_encode_batch_device for the entries that
are not split), the frames are valid for the oracle and the compiled reference, nothing is written outside a slot, the output goes
through zpk_codec_pack_batch_device and the device decoders unchanged, and two calls in a row on one stream need no wait between them.

Every test sets OPT_ENC_SPLIT_MIN to 1, so that an entry of 512 KiB + 1 is already written in pieces, and restores 2 MiB."""
import ctypes as C

import numpy as np
import pytest

import zpack_amd
from benchdata import datagen as dg
from tests import zpk
from tests._libs import oracle, have_ref, ref
from zpack_amd import METHOD_NONE, METHOD_ZSTD, METHOD_LZ4, OPT_ENC_SPLIT_MIN

pytestmark = pytest.mark.gpu
M = 1 << 20
PIECE = 512 << 10
R_BUFFER_TOO_SMALL, R_COMPRESS_FAILED = 12, 14
CANARY = 0xEE

CASES = [(METHOD_LZ4, 0, PIECE + 1), (METHOD_LZ4, 0, 2 * PIECE), (METHOD_LZ4, 0, 3 * PIECE + 17),
         (METHOD_ZSTD, 1, PIECE + 1), (METHOD_ZSTD, 1, 2 * PIECE + 70000), (METHOD_ZSTD, 3, PIECE + 1), (METHOD_ZSTD, 3, 2 * PIECE + 70000),
         (METHOD_NONE, 0, 2 * PIECE + 3), (METHOD_LZ4, 9, 2 * PIECE)]
CLASSES = [dg.TEXT, dg.RANDOM, dg.RUNS]


def _header_len(method):
    return {METHOD_NONE: 0, METHOD_LZ4: 7, METHOD_ZSTD: 10}[method]


@pytest.fixture(scope="module")
def codec():
    c = zpack_amd.Codec(0)
    c.set_option(OPT_ENC_SPLIT_MIN, 1)
    yield c
    c.set_option(OPT_ENC_SPLIT_MIN, 2 * M)
    c.close()


class Batch:
    """Plaintexts laid out in one source blob (offsets NOT 16-aligned, 64 bytes of allocation behind the last byte) and one slot per
    entry in one larger tensor, a canary region in front of, between and behind the slots."""

    def __init__(self, plains, methods, caps=None, dst_offsets=None, tail=256):
        """dst_offsets: where the slots start (default: one behind the other's bound, 77 to 89 bytes between them); tail: bytes of
        allocation behind the last slot"""
        self.plains, self.methods, self.n = plains, methods, len(plains)
        self.desc = d = np.zeros(self.n, dtype=zpack_amd.ENCODE_DESC)
        bound = zpack_amd.lib().zpk_codec_compress_bound
        pos, out, end = 5, 131, 0
        for i, (p, (m, lv)) in enumerate(zip(plains, methods)):
            pos += (3, 7, 11, 1)[i % 4]
            if pos % 16 == 0:
                pos += 3
            full = int(bound(m, len(p)))
            cap = full if caps is None or caps[i] is None else caps[i]
            d[i] = (pos, len(p), out if dst_offsets is None else dst_offsets[i], cap, m, lv)
            pos += len(p) + 16
            out += full + 77 + 2 * (i % 7)                                   # (the slots stay where they are whatever `caps` says)
            end = max(end, int(d[i]["dst_offset"]) + cap)
        self.blob = np.zeros(pos + 64, dtype=np.uint8)
        for p, e in zip(plains, d):
            self.blob[int(e["src_offset"]):int(e["src_offset"]) + len(p)] = p
        self.dst_bytes = out + tail if dst_offsets is None else end + tail

    def run(self, codec, desc=None, stream=None, call="big"):
        """-> (slots tensor, results tensor): enqueued, not waited for"""
        import torch
        dev = torch.device("cuda:0")
        desc = self.desc if desc is None else desc
        if not hasattr(self, "src"):
            self.src = torch.from_numpy(self.blob).to(dev)
        dst = torch.full((self.dst_bytes,), CANARY, dtype=torch.uint8, device=dev)
        res = torch.full((len(desc) * zpack_amd.ENCODE_RESULT.itemsize,), 0xAB, dtype=torch.uint8, device=dev)
        if call == "big":
            torch.cuda.synchronize()
            codec.encode_big_device(self.src, desc, dst, res, stream=stream)
        else:
            ddesc = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8)).to(dev)
            torch.cuda.synchronize()
            codec.encode_batch_device(self.src, ddesc, len(desc), dst, res, stream=stream)
            self.keep = ddesc
        return dst, res

    def host(self, codec, desc=None):
        """zpk_codec_encode_batch_host on the same plaintexts -> (results, [payload bytes])"""
        desc = self.desc if desc is None else desc
        n = len(desc)
        outs = [np.full(max(int(e["dst_capacity"]), 1), CANARY, dtype=np.uint8) for e in desc]
        res = np.zeros(n, dtype=zpack_amd.ENCODE_RESULT)
        srcs = [self.blob[int(e["src_offset"]):int(e["src_offset"]) + int(e["size"])].copy() for e in desc]
        sp = (C.c_void_p * n)(*[p.ctypes.data for p in srcs])
        dp = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        rc = codec.L.zpk_codec_encode_batch_host(codec.h, sp, np.ascontiguousarray(desc).ctypes.data, n, dp, res.ctypes.data)
        assert rc == 0, rc
        return res, [o[:int(k)] for o, k in zip(outs, res["comp_size"])]


def _home(dst, res):
    import torch
    torch.cuda.synchronize()
    return dst.cpu().numpy(), res.cpu().numpy().view(zpack_amd.ENCODE_RESULT).copy()


def _same_results(a, b, fields=("status", "comp_size", "hash")):
    for f in fields:
        assert np.array_equal(a[f], b[f]), (f, a[f], b[f])


def _outside_slots_intact(image, desc):
    mask = np.ones(len(image), dtype=bool)
    for e in desc:
        mask[int(e["dst_offset"]):int(e["dst_offset"]) + int(e["dst_capacity"])] = False
    assert (image[mask] == CANARY).all(), "a byte outside every slot was written"


@pytest.fixture(scope="module")
def cases(codec):
    """Every case of every class, encoded ONCE by the new call and once by the host path; shared by the tests below (read only)."""
    plains, methods = [], []
    for ci, cls in enumerate(CLASSES):
        for k, (m, lv, size) in enumerate(CASES):
            plains.append(dg.fill(cls, 1300 + ci, k, size))
            methods.append((m, lv))
    b = Batch(plains, methods)
    b.dst, b.res_dev = b.run(codec)
    b.stats = codec.encode_stats()
    b.image, b.res = _home(b.dst, b.res_dev)
    b.host_res, b.host_pay = b.host(codec)
    return b


def test_split_entries_equal_the_host_path_and_are_valid_frames(codec, cases):
    """All cases in one call.  Each slot's first comp_size bytes, and comp_size, hash and status, are those of zpk_codec_encode_batch_host
    on the same plaintexts at the same split option; the hashes are the real XXH3's; the oracle and the compiled reference decode every
    frame to its plaintext; encode_stats names the split entries and their pieces."""
    b = cases
    assert (b.res["status"] == 0).all(), b.res
    _same_results(b.res, b.host_res)
    assert [int(h) for h in b.res["hash"]] == [dg.xxh3(p) for p in b.plains]
    for i, e in enumerate(b.desc):
        a, k = int(e["dst_offset"]), int(b.res["comp_size"][i])
        assert np.array_equal(b.image[a:a + k], b.host_pay[i]), i
    _outside_slots_intact(b.image, b.desc)
    assert b.stats == dict(split_entries=b.n, pieces=sum((len(p) + PIECE - 1) // PIECE for p in b.plains)), b.stats
    o = oracle()
    for i, (p, e) in enumerate(zip(b.plains, b.desc)):
        a, k = int(e["dst_offset"]), int(b.res["comp_size"][i])
        arc = np.zeros(10 + k + 64, dtype=np.uint8)                                # (the entry inside an archive image: the checker has the reader's offset guards)
        arc[10:10 + k] = b.image[a:a + k]
        rc, out, got, h = o.entry_decode(arc, 10, k, len(p), int(b.res["hash"][i]), b.methods[i][0], len(p))
        assert rc == 0 and got == len(p) and out == p.tobytes(), (i, rc, got)
    if have_ref():
        pay, ents, at = [], [], 10
        for i, (p, e) in enumerate(zip(b.plains, b.desc)):
            a, k = int(e["dst_offset"]), int(b.res["comp_size"][i])
            pay.append(b.image[a:a + k].tobytes())
            ents.append(("e%d" % i, at, k, len(p), int(b.res["hash"][i]), b.methods[i][0]))
            at += k
        R = ref()
        rc, r, keep = R.open_memory(zpk.assemble(pay, ents))
        assert rc == 0
        for i, p in enumerate(b.plains):
            rc, out = R.read_file(r, i, len(p))
            assert rc == 0 and out == p.tobytes(), (i, rc)
        R.close_reader(r)


def _mixed():
    sizes = [(METHOD_LZ4, 0, 1), (METHOD_LZ4, 0, PIECE + 1), (METHOD_ZSTD, 1, 70000), (METHOD_ZSTD, 1, 2 * PIECE + 5), (METHOD_NONE, 0, PIECE),
             (METHOD_NONE, 0, PIECE + 9), (METHOD_ZSTD, 3, PIECE), (METHOD_LZ4, 9, 70000), (METHOD_LZ4, 0, 2 * PIECE)]
    plains = [dg.fill(dg.TEXT if k % 2 else dg.RUNS, 1310, k, n) for k, (_, _, n) in enumerate(sizes)]
    return Batch(plains, [(m, lv) for m, lv, _ in sizes])


def test_mixed_call_leaves_small_entries_to_the_one_wave_path(codec):
    """Entries at or below 512 KiB (1 byte, 70 000, exactly 512 KiB) among split ones: exactly the bytes and results of
    zpk_codec_encode_batch_device for them, the split ones as the host path writes them.  With OPT_ENC_SPLIT_MIN = 0 (never split) the
    call equals zpk_codec_encode_batch_device entirely and encode_stats reads 0 / 0."""
    b = _mixed()
    image, res = _home(*b.run(codec))
    stats = codec.encode_stats()
    one_image, one_res = _home(*b.run(codec, call="batch"))
    host_res, host_pay = b.host(codec)
    small = [i for i, p in enumerate(b.plains) if len(p) <= PIECE]
    assert len(small) == 5 and stats == dict(split_entries=4, pieces=2 + 3 + 2 + 2), stats
    assert (res["status"] == 0).all(), res
    for i, e in enumerate(b.desc):
        a, k = int(e["dst_offset"]), int(res["comp_size"][i])
        if i in small:
            assert res[i] == one_res[i], (i, res[i], one_res[i])
            assert np.array_equal(image[a:a + k], one_image[a:a + k]), i
        else:
            _same_results(res[i:i + 1], host_res[i:i + 1])
            assert np.array_equal(image[a:a + k], host_pay[i]), i
    _outside_slots_intact(image, b.desc)
    codec.set_option(OPT_ENC_SPLIT_MIN, 0)
    try:
        image0, res0 = _home(*b.run(codec))
        stats0 = codec.encode_stats()
    finally:
        codec.set_option(OPT_ENC_SPLIT_MIN, 1)
    assert stats0 == dict(split_entries=0, pieces=0), stats0
    assert np.array_equal(res0, one_res) and np.array_equal(image0, one_image)


@pytest.mark.parametrize("room", ["comp_size - 1", "header only"])
def test_a_frame_that_does_not_fit_fails_inside_its_slot(codec, room):
    """dst_capacity one byte short of the frame (and: the frame header's length only) for one LZ4, one Zstandard and one stored entry, the
    slots between canary regions: COMPRESS_FAILED / BUFFER_TOO_SMALL, comp_size = hash = 0, every byte outside the slots intact, the
    neighbouring entries' results and bytes unchanged."""
    sizes = [(METHOD_LZ4, 0, 70000), (METHOD_LZ4, 0, 2 * PIECE), (METHOD_ZSTD, 1, PIECE + 1), (METHOD_LZ4, 0, PIECE + 1), (METHOD_NONE, 0, 2 * PIECE + 3),
             (METHOD_ZSTD, 1, 70000)]
    plains = [dg.fill(dg.TEXT, 1320, k, n) for k, (_, _, n) in enumerate(sizes)]
    methods = [(m, lv) for m, lv, _ in sizes]
    full = Batch(plains, methods)
    image1, res1 = _home(*full.run(codec))
    assert (res1["status"] == 0).all()
    tight = (1, 2, 4)
    caps = [None] * len(sizes)
    for i in tight:
        caps[i] = int(res1["comp_size"][i]) - 1 if room == "comp_size - 1" else _header_len(methods[i][0])
    b = Batch(plains, methods, caps)
    assert np.array_equal(b.desc["dst_offset"], full.desc["dst_offset"])
    image2, res2 = _home(*b.run(codec))
    for i, e in enumerate(b.desc):
        if i in tight:
            want = R_BUFFER_TOO_SMALL if methods[i][0] == METHOD_NONE else R_COMPRESS_FAILED
            assert (int(res2["status"][i]), int(res2["comp_size"][i]), int(res2["hash"][i])) == (want, 0, 0), (i, res2[i])
        else:
            a, k = int(e["dst_offset"]), int(res1["comp_size"][i])
            assert res2[i] == res1[i] and np.array_equal(image2[a:a + k], image1[a:a + k]), i
    _outside_slots_intact(image2, b.desc)
    # the host path's verdicts for the same capacities
    host_res, _ = b.host(codec)
    _same_results(res2, host_res)


def test_frames_go_through_pack_and_the_device_decoders(codec, cases):
    """The slots and results of the call, as they lie on the device, are packed by zpk_codec_pack_batch_device into an archive image and
    decoded by zpk_codec_decode_batch_device — one entry also by zpk_codec_decode_big_device: statuses 0, bytes equal the plaintext."""
    import torch
    b = cases
    dev = torch.device("cuda:0")
    ddesc = torch.from_numpy(b.desc.view(np.uint8)).to(dev)
    offs = torch.zeros(b.n + 1, dtype=torch.int64, device=dev)
    total = int(b.res["comp_size"].sum())
    packed = torch.full((total + 256,), CANARY, dtype=torch.uint8, device=dev)
    codec.pack_batch_device(b.dst, ddesc, b.res_dev, b.n, packed, offs, int(b.desc["dst_capacity"].max()))
    torch.cuda.synchronize()
    off = offs.cpu().numpy().view(np.uint64)
    assert int(off[-1]) == total and np.array_equal(np.diff(off), b.res["comp_size"])
    d = np.zeros(b.n, dtype=zpack_amd.DECODE_DESC)
    d["src_offset"] = off[:-1]; d["comp_size"] = b.res["comp_size"]; d["uncomp_size"] = b.desc["size"]; d["expect_hash"] = b.res["hash"]
    d["dst_capacity"] = b.desc["size"]; d["method"] = [m for m, _ in b.methods]
    d["dst_offset"] = np.concatenate([[0], np.cumsum((b.desc["size"] + np.uint64(255)) & ~np.uint64(255))])[:-1]
    out_bytes = int(d["dst_offset"][-1] + d["dst_capacity"][-1]) + 64
    out = torch.full((out_bytes,), CANARY, dtype=torch.uint8, device=dev)
    dres = torch.zeros(b.n * zpack_amd.DECODE_RESULT.itemsize, dtype=torch.uint8, device=dev)
    codec.decode_batch_device(packed, torch.from_numpy(d.view(np.uint8)).to(dev), b.n, out, dres)
    torch.cuda.synchronize()
    r = dres.cpu().numpy().view(zpack_amd.DECODE_RESULT)
    assert (r["status"] == 0).all() and np.array_equal(r["produced"], b.desc["size"]) and np.array_equal(r["hash"], b.res["hash"]), r
    home = out.cpu().numpy()
    for i, p in enumerate(b.plains):
        a = int(d["dst_offset"][i])
        assert np.array_equal(home[a:a + len(p)], p), i
    i = 2                                                                        # LZ4, 3 pieces + 17 bytes of text
    out1 = torch.full((out_bytes,), CANARY, dtype=torch.uint8, device=dev)
    r1 = codec.decode_big_device(packed, d[i:i + 1], out1)
    a = int(d["dst_offset"][i])
    assert int(r1["status"]) == 0 and int(r1["hash"]) == int(b.res["hash"][i]) and np.array_equal(out1.cpu().numpy()[a:a + len(b.plains[i])], b.plains[i])


def test_two_calls_in_a_row_on_one_stream(codec, cases):
    """Two calls back to back on one non-default stream, one synchronise behind both: both result arrays and both sets of slots are
    right.  (Each call takes its tables up from pinned memory behind the work the stream still holds; the descriptors handed in may go
    away as soon as a call returns.)"""
    import torch
    b = cases
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    first, second = np.arange(0, 5), np.arange(5, 12)
    da, db = b.desc[first].copy(), b.desc[second].copy()
    dst_a, dst_b = (torch.full((b.dst_bytes,), CANARY, dtype=torch.uint8, device=dev) for _ in range(2))
    res_a, res_b = (torch.full((len(d) * zpack_amd.ENCODE_RESULT.itemsize,), 0xAB, dtype=torch.uint8, device=dev) for d in (da, db))
    torch.cuda.synchronize()                                                     # (torch's fills; nothing waits from here to the synchronise below)
    codec.encode_big_device(b.src, da, dst_a, res_a, stream=s.cuda_stream)
    da[:] = 0                                                                    # consumed before the call returned
    codec.encode_big_device(b.src, db, dst_b, res_b, stream=s.cuda_stream)
    db[:] = 0
    s.synchronize()
    for idx, dst, res in ((first, dst_a, res_a), (second, dst_b, res_b)):
        image, r = _home(dst, res)
        _same_results(r, b.host_res[idx])
        for j, i in enumerate(idx):
            a, k = int(b.desc["dst_offset"][i]), int(r["comp_size"][j])
            assert np.array_equal(image[a:a + k], b.host_pay[i]), i
        _outside_slots_intact(image, b.desc[idx])
