"""Every Zstandard decoder of the tree against the oracle on the hand-built frames of tests/zstd_asm.py (what the frames are, and that
libzstd and the oracle agree on them, is tests/test_zstd_asm_cpu.py).  All cases go into ONE device batch per path.  Expected status,
bytes up to `produced` and `produced` are the oracle's (oracle().entry_decode), the hash is the real XXH3; the bar is bit-exact.

  - the device batch with the XXH3 verify OFF: nothing papers over a wrong fast path
  - the device batch with the verify on, and the counters: a case finishes two-stage unless the case table names the line that declines it
  - the sequence arena of k_zstd_fse against the oracle's sequence trace, word for word
  - group I through the host path, the block-parallel reader and the device walk
  - every case through the resumable stream decoder in chunks of 7 and 1000 bytes"""
import numpy as np
import pytest

import zpack_amd
from tests import zstd_asm as Z
from tests._libs import oracle
from tests.test_zstd_asm_cpu import CAP, judged

pytestmark = pytest.mark.gpu
ZSTD = 1


@pytest.fixture(scope="module")
def codec():
    return zpack_amd.Codec(0)


@pytest.fixture(scope="module")
def cases():
    """every case with the oracle's verdict on it as an archive entry; intact = the oracle (and libzstd) decode it and the hash is right"""
    out = []
    for c in Z.CASES:
        c = dict(c)
        c.update(judged(c))
        c["intact"] = c["rc"] == 0
        out.append(c)
    assert sum(c["intact"] for c in out) >= 130 and sum(not c["intact"] for c in out) >= 25
    return out


def _batch(codec, cs, flags):
    """one device batch -> (descriptors, results, output image, counters, marks of k_zstd_fse / k_zstd_exec, arena words per entry)"""
    import torch
    n = len(cs)
    offs, off = [], 16
    for c in cs:
        offs.append(off)
        off += len(c["frame"])
    arc = b"\0" * 16 + b"".join(c["frame"] for c in cs) + b"\0" * 64
    desc = np.zeros(n, dtype=zpack_amd.DECODE_DESC)
    desc["src_offset"] = offs
    desc["comp_size"] = [len(c["frame"]) for c in cs]
    desc["uncomp_size"] = [c["uncomp"] for c in cs]
    desc["dst_capacity"] = [c["cap"] for c in cs]
    desc["expect_hash"] = [c["hash"] for c in cs]
    desc["method"] = ZSTD
    desc["flags"] = flags
    slot = (np.maximum(desc["dst_capacity"], desc["uncomp_size"]) + np.uint64(255 + 64)) & ~np.uint64(255)
    desc["dst_offset"] = np.concatenate([[0], np.cumsum(slot)])[:-1]
    total = int(slot.sum()) + 256
    dev = torch.device("cuda:0")
    src = torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy()).to(dev)
    dst = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    ddesc = torch.from_numpy(desc.view(np.uint8)).to(dev)
    dres = torch.zeros(n * zpack_amd.DECODE_RESULT.itemsize, dtype=torch.uint8, device=dev)
    codec.decode_batch_device(src, ddesc, n, dst, dres)
    torch.cuda.synchronize()
    st = codec.decode_stats()
    marks = codec.debug_fetch(1, 0, n, np.uint32)
    o = oracle()
    arena = []
    for i, c in enumerate(cs):
        if marks[i] == 0:
            arena.append(None)
            continue
        rc, seqs = o.zstd_sequences(c["frame"], CAP, 1 << 16)
        arena.append((codec.debug_fetch(0, (int(desc[i]["dst_offset"]) + 7) & ~7, max(1, len(seqs)), np.uint64)[:len(seqs)], seqs))
    return desc, dres.cpu().numpy().view(zpack_amd.DECODE_RESULT).copy(), dst.cpu().numpy(), st, marks, arena


def _judge(cs, desc, r, out):
    """status, produced, bytes and hash of every entry against the oracle's, and nothing written behind an entry's slot"""
    bad = []
    for i, c in enumerate(cs):
        a, got = int(desc[i]["dst_offset"]), int(r[i]["status"])
        if got != c["rc"]:
            bad.append((c["label"], "status", got, "oracle", c["rc"]))
            continue
        end = a + max(c["cap"], c["uncomp"])
        if not (out[end:end + 64] == 0xA5).all():
            bad.append((c["label"], "bytes written behind the slot"))
        if c["rc"] != 0:
            continue
        if int(r[i]["produced"]) != c["produced"]:
            bad.append((c["label"], "produced", int(r[i]["produced"]), "oracle", c["produced"]))
        elif out[a:a + c["uncomp"]].tobytes() != c["out"][:c["uncomp"]]:
            w = np.frombuffer(c["out"][:c["uncomp"]], dtype=np.uint8)
            bad.append((c["label"], "first bad byte", int(np.nonzero(out[a:a + c["uncomp"]] != w)[0][0]), "of", c["uncomp"]))
        elif int(r[i]["hash"]) != c["hash"]:
            bad.append((c["label"], "hash"))
    return bad


def _arena_bad(cs, arena):
    bad = []
    for c, a in zip(cs, arena):
        if a is not None and not np.array_equal(a[0], a[1]):
            k = int(np.nonzero(a[0] != a[1])[0][0])
            bad.append((c["label"], "sequence", k, "of", len(a[1]), "arena %x" % int(a[0][k]), "oracle %x" % int(a[1][k])))
    return bad


@pytest.mark.parametrize("which", ["intact", "all"])
def test_device_batch_without_the_hash_equals_the_oracle(codec, cases, which):
    """DF_SKIP_HASH: a wrong pre-decoded sequence or a wrong execution is not caught and repeated by anything"""
    cs = [c for c in cases if c["intact"] or which == "all"]
    desc, r, out, st, marks, arena = _batch(codec, cs, zpack_amd.DF_SKIP_HASH)
    assert st["zstd"] == len(cs) and st["zstd_two_stage"] + st["zstd_fused"] == len(cs), st       # every case reaches a decoder
    assert st["fse_watchdog"] == 0 and st["fse_budget"] == 0 and st["retried_zstd"] == 0, st
    assert _judge(cs, desc, r, out) == []
    assert _arena_bad(cs, arena) == []


@pytest.mark.parametrize("which", ["intact", "all"])
def test_device_batch_with_the_hash_finishes_two_stage_what_the_table_says(codec, cases, which):
    cs = [c for c in cases if c["intact"] or which == "all"]
    desc, r, out, st, marks, arena = _batch(codec, cs, 0)
    assert _judge(cs, desc, r, out) == []
    assert st["fse_watchdog"] == 0 and st["fse_budget"] == 0 and st["retried_zstd"] == 0, st
    assert st["zstd"] == len(cs) and st["zstd_two_stage"] == int((marks == 2).sum()) and st["zstd_two_stage"] + st["zstd_fused"] == len(cs), st
    fell_back = [(c["label"], int(m)) for c, m in zip(cs, marks) if c["intact"] and c["two_stage"] is True and m != 2]
    assert not fell_back, ("not finished two-stage, and not declined by design in the case table", fell_back)
    surprise = [(c["label"], c["two_stage"]) for c, m in zip(cs, marks) if c["intact"] and isinstance(c["two_stage"], str) and m == 2]
    assert not surprise, ("finished two-stage although the case table names a line that declines it", surprise)
    for c in cs:                                        # every intact case of groups C to H says how it finishes
        assert c["two_stage"] is not None or c["group"] in "ABI" or not c["intact"], c["label"]


def test_the_sequence_arena_equals_the_oracles_trace(codec, cases):
    """k_zstd_fse itself against a reference: every entry it marks has the oracle's sequences in its arena region, and it marks every
    intact case of the table that is not declined in front of k_zstd_exec"""
    cs = [c for c in cases if c["intact"]]
    desc, r, out, st, marks, arena = _batch(codec, cs, 0)
    assert _arena_bad(cs, arena) == []
    # not vacuous: every case that must finish two-stage and has sequences was compared
    assert all(a is not None and len(a[1]) == c["expect"].get("sequences", len(a[1])) for c, a in zip(cs, arena) if c["two_stage"] is True)
    assert sum(1 for a in arena if a is not None and len(a[1])) >= 100
    unmarked = [c["label"] for c, m in zip(cs, marks) if c["two_stage"] is True and m == 0]
    assert not unmarked, unmarked


def _one_desc(c, flags=0):
    d = np.zeros(1, dtype=zpack_amd.DECODE_DESC)
    d["src_offset"] = 16; d["comp_size"] = len(c["frame"]); d["uncomp_size"] = c["uncomp"]; d["expect_hash"] = c["hash"]
    d["dst_capacity"] = c["cap"]; d["method"] = ZSTD; d["flags"] = flags
    return d, np.frombuffer(b"\0" * 16 + c["frame"] + b"\0" * 64, dtype=np.uint8).copy()


def test_group_i_through_the_host_path_and_the_block_parallel_reader(codec, cases):
    """OPT_DEC_SPLIT_MIN = 1 sends every entry that qualifies to the block-parallel reader (zstd_pj.h); decode_big_device and
    decode_big_batch_device walk the blocks on the device (k_big_walk).  Verdict, produced, bytes and hash are the oracle's on every
    path.  That the reader RAN is shown by its flag word (zstd_blocks_flags = zpj_last_err: 0 when the reader finished the last frame
    it was given, the reason when it gave it up, and untouched when it was not reached): in front of every run the word is set to the
    OTHER value by a frame known to leave it there, so a case that stayed with the one-wave decoder keeps that value.  The host paths
    give the reader only entries worth a turn of the whole chip (pj_choose): the two large cases must reach it, the small ones may."""
    import torch
    cs = [c for c in cases if c["group"] == "I"]
    assert len(cs) >= 6
    dev = torch.device("cuda:0")
    given_up = [c for c in cs if c["expect"].get("zpj_err")][0]
    finished = [c for c in cs if c["expect"].get("reader")][0]

    def host(c, split):
        d, arc = _one_desc(c)
        codec.set_option(zpack_amd.OPT_DEC_SPLIT_MIN, split)
        try:
            res, outs = codec.decode_batch_host(arc, d)
            flags = codec.decode_stats()["zstd_blocks_flags"]
        finally:
            codec.set_option(zpack_amd.OPT_DEC_SPLIT_MIN, 2 << 20)
        return (int(res[0]["status"]), int(res[0]["produced"]), int(res[0]["hash"]), outs[0][:c["uncomp"]].tobytes()), flags

    def prime(c):
        """leave the flag word at the value that `c` must change if the reader takes it -> that value is non-zero"""
        want_err = not c["expect"].get("zpj_err")
        flags = host(given_up if want_err else finished, 1)[1]
        assert (flags != 0) == want_err, (c["label"], "priming", hex(flags))
        return flags

    assert host(given_up, 1)[1] != 0 and host(finished, 1)[1] == 0 and host(given_up, 1)[1] != 0       # the word follows the reader
    for c in cs:
        d, arc = _one_desc(c)
        accepted = c["expect"].get("block_parallel", True)
        results, flags = {}, {}
        before = prime(c)
        results["default"], flags["default"] = host(c, 2 << 20)
        assert flags["default"] == before, (c["label"], "block-parallel below the default threshold")
        results["split"], flags["split"] = host(c, 1)
        src = torch.from_numpy(arc).to(dev)
        for name in ("big", "big_batch"):
            before = prime(c)
            codec.set_option(zpack_amd.OPT_DEC_SPLIT_MIN, 1)
            try:
                dst = torch.full((c["cap"] + 256,), 0xA5, dtype=torch.uint8, device=dev)
                r = codec.decode_big_device(src, d, dst) if name == "big" else codec.decode_big_batch_device(src, d, dst)[0]
                torch.cuda.synchronize()
                st = codec.decode_stats()
            finally:
                codec.set_option(zpack_amd.OPT_DEC_SPLIT_MIN, 2 << 20)
            h = dst.cpu().numpy()
            assert (h[c["cap"]:] == 0xA5).all(), (c["label"], name, "bytes written behind the slot")
            results[name], flags[name] = (int(r["status"]), int(r["produced"]), int(r["hash"]), h[:c["uncomp"]].tobytes()), st["zstd_blocks_flags"]
            if name == "big_batch":
                assert (st["device_walked"], st["device_walk_accepted"]) == (1, 1 if accepted else 0), (c["label"], st)
            elif accepted and not c["expect"].get("zpj_err"):        # no chooser on this path: the reader's own bytes and hash are the result
                assert st["frame_parallel_entries"] == 1, (c["label"], st)
        want = (c["rc"], c["produced"], c["hash"], c["out"][:c["uncomp"]])
        for name, got in results.items():
            assert got[0] == want[0], (c["label"], name, "status", got[0], want[0])
            if want[0] == 0:
                assert got[1:3] == want[1:3] and got[3] == want[3], (c["label"], name, got[1:3], want[1:3])
        # the per-case record: which paths gave the frame to the reader.  Never the frame with a checksum; always (host path) the two
        # frames large enough to be worth it; and the reader finishes every frame it is given but the one whose block regenerates more
        # than 128 KiB
        ran = {name: flags[name] != before for name in ("split", "big", "big_batch")}
        print("reader ran:", c["label"][:50], ran, {k: hex(v) for k, v in flags.items()})
        for name in ran:
            if ran[name]:
                assert accepted and (flags[name] != 0) == bool(c["expect"].get("zpj_err")), (c["label"], name, hex(flags[name]))
        if c["expect"].get("reader") or c["expect"].get("zpj_err"):
            assert ran["split"], (c["label"], "the reader did not run", hex(flags["split"]))


@pytest.mark.parametrize("chunk", [7, 1000])
def test_stream_steps_agree_with_the_oracle(codec, cases, chunk):
    """k_zstd_stream resumed inside every construct of every case: the final verdict, the bytes and the hash are the one-shot ones"""
    from tests.test_gpu_codec import _stream_decode
    o = oracle()
    bad = []
    for c in cases:
        if c["cap"] != c["uncomp"]:                      # (a stream has no capacity of its own: the case that overflows it is a one-shot case)
            continue
        status, got, first = _stream_decode(codec, c["frame"], ZSTD, c["uncomp"], c["hash"], chunk)
        want = c["rc"]
        if status != want:
            bad.append((c["label"], "stream", status, "oracle", want))
        elif want == 0 and (got != c["out"][:c["uncomp"]] or o.xxh3(got) != c["hash"]):
            bad.append((c["label"], "bytes"))
    assert bad == []
