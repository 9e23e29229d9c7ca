"""The block-parallel LZ4 reader (zpack_amd/csrc/lz4_pj.h, decode_big_lz4_single and pj_finish in zpk_codec.hip) on the hand-built frames
of tests/lz4_asm.py.  What is right was recorded on the CPU (tests/test_lz4_asm_cpu.py: liblz4, the oracle and the compiled reference
agree on every case here): status, produced size, bytes and hash, all bit-exact.

Bytes alone would pass a broken reader: whatever it gets wrong or gives up is silently decoded again by the one-wave decoder.  So the
point of the case-by-case tests is the COUNTER: decode_big_device has no chooser, and frame_parallel_entries / frame_parallel_frames say
whether the reader finished the entry — 1 / the block count exactly for the cases the table marks `reader`, 0 for all others.

Every test lowers OPT_DEC_SPLIT_MIN to 1 (the readers then get every entry that qualifies, however small) and puts the default back.
Every output slot lies at least 4096 bytes inside its tensor, and every byte of the tensor outside the slots must stay 0xA5."""
import contextlib

import numpy as np
import pytest

import zpack_amd
from tests import lz4_asm as A
from tests._libs import oracle
from tests.test_lz4_asm_cpu import FILL, HASH_MISMATCH, LZ4, OK, judged

pytestmark = pytest.mark.gpu
GUARD = 4096
SPLIT_MIN_DEFAULT = 256 << 10            # ZPK_DEC_SPLIT_MIN_DEFAULT (zpack_amd/csrc/dec_plan.h)


@pytest.fixture(scope="module")
def codec():
    return zpack_amd.Codec(0)


@contextlib.contextmanager
def split_min_1(codec):
    codec.set_option(zpack_amd.OPT_DEC_SPLIT_MIN, 1)
    try:
        yield
    finally:
        codec.set_option(zpack_amd.OPT_DEC_SPLIT_MIN, SPLIT_MIN_DEFAULT)


class Table:
    pass


@pytest.fixture(scope="module")
def table():
    """groups A to G with the CPU judges' record on each, their frames back to back in one archive image on the device"""
    import torch
    T = Table()
    T.cases = [dict(c, **judged(c)) for c in A.CASES if c["group"] != "L"]
    assert len(T.cases) >= 390 and sum(c["reader"] for c in T.cases) >= 360
    T.desc = np.zeros(len(T.cases), dtype=zpack_amd.DECODE_DESC)
    at, parts = 16, [b"\0" * 16]
    for i, c in enumerate(T.cases):
        T.desc[i]["src_offset"], T.desc[i]["comp_size"], T.desc[i]["uncomp_size"] = at, len(c["frame"]), c["uncomp"]
        T.desc[i]["dst_capacity"], T.desc[i]["expect_hash"], T.desc[i]["method"] = c["cap"], c["hash"], LZ4
        parts.append(c["frame"])
        at += len(c["frame"])
    parts.append(b"\0" * 64)
    T.arc = b"".join(parts)
    T.src = torch.from_numpy(np.frombuffer(T.arc, dtype=np.uint8).copy()).to(torch.device("cuda:0"))
    return T


def _against_the_record(c, status, produced, h, got):
    """got: the entry's slot, `cap` bytes -> what differs from the judges' record"""
    if status != c["rc"]:
        return (c["label"], "status", status, "judges", c["rc"])
    if c["rc"] not in (OK, HASH_MISMATCH):
        return None
    if produced != c["produced"]:
        return (c["label"], "produced", produced, "judges", c["produced"])
    want = c["out"][:c["uncomp"]]
    if not np.array_equal(got[:c["uncomp"]], want):
        return (c["label"], "first bad byte", int(np.nonzero(got[:c["uncomp"]] != want)[0][0]), "of", c["uncomp"])
    if c["rc"] == OK and h != c["hash"]:
        return (c["label"], "hash", hex(h), hex(c["hash"]))
    return None


def _one(codec, T, i, lead):
    """case i alone through decode_big_device, its slot `lead` bytes inside a tensor of 0xA5 -> [what is wrong]"""
    import torch
    c = T.cases[i]
    whole = torch.full((lead + c["cap"] + GUARD,), FILL, dtype=torch.uint8, device=T.src.device)
    d = T.desc[i:i + 1].copy()
    d["dst_offset"] = lead
    r = codec.decode_big_device(T.src, d, whole)
    torch.cuda.synchronize()
    st = codec.decode_stats()
    h = whole.cpu().numpy()
    bad = []
    x = _against_the_record(c, int(r["status"]), int(r["produced"]), int(r["hash"]), h[lead:lead + c["cap"]])
    if x:
        bad.append(x)
    if not ((h[:lead] == FILL).all() and (h[lead + c["cap"]:] == FILL).all()):
        out = np.nonzero(np.concatenate([h[:lead], np.full(c["cap"], FILL, np.uint8), h[lead + c["cap"]:]]) != FILL)[0]
        bad.append((c["label"], "bytes written outside the slot, the first at", int(out[0]) - lead))
    want = (1, c["nblocks"]) if c["reader"] else (0, 0)
    if (st["frame_parallel_entries"], st["frame_parallel_frames"]) != want:
        bad.append((c["label"], "the reader finished (entries, blocks)", (st["frame_parallel_entries"], st["frame_parallel_frames"]), "the table says", want))
    return bad


@pytest.mark.parametrize("group", list("ABCDEFG"))
def test_decode_big_device_case_by_case(codec, table, group):
    bad, seen = [], 0
    with split_min_1(codec):
        for i, c in enumerate(table.cases):
            if c["group"] == group:
                seen += 1
                bad += _one(codec, table, i, GUARD)
    assert seen >= 6
    assert bad == []


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_the_slot_at_every_residue_mod_4(codec, table, shift):
    """groups B, E and F: the word stores of k_pj_gather at a chunk boundary and at the slot's ends, wherever the slot begins"""
    bad, seen = [], 0
    with split_min_1(codec):
        for i, c in enumerate(table.cases):
            if c["group"] in "BEF":
                seen += 1
                bad += _one(codec, table, i, GUARD + shift)
    assert seen >= 30
    assert bad == []


def _is_candidate(d, archive_size, dst_size):
    """dec_big_candidate_device (zpack_amd/csrc/dec_plan.h) with a split minimum of 1"""
    comp, uncomp, cap, off, dst = (int(d[k]) for k in ("comp_size", "uncomp_size", "dst_capacity", "src_offset", "dst_offset"))
    return 1 <= uncomp <= (4 << 30) and comp != 0 and cap >= uncomp and off <= archive_size and comp < archive_size - off and \
        dst <= dst_size and uncomp <= dst_size - dst


def _laid_out(T, idx):
    """the entries idx of the table in one output image: every slot with GUARD bytes in front of it and behind it -> (desc, image size)"""
    d = T.desc[idx].copy()
    at = GUARD
    for k in range(len(d)):
        d[k]["dst_offset"] = at + k % 4                           # (and the slots at every residue)
        at += int(d[k]["dst_capacity"]) + GUARD + 4
    return d, at


def _judge_image(cs, d, res, image):
    bad = []
    inside = np.zeros(len(image), dtype=bool)
    for k, c in enumerate(cs):
        a = int(d[k]["dst_offset"])
        inside[a:a + c["cap"]] = True
        x = _against_the_record(c, int(res[k]["status"]), int(res[k]["produced"]), int(res[k]["hash"]), image[a:a + c["cap"]])
        if x:
            bad.append(x)
    stray = np.nonzero(~inside & (image != FILL))[0]
    if len(stray):
        bad.append(("bytes written outside every slot, the first at", int(stray[0])))
    return bad


def test_decode_big_batch_device_all_cases_in_one_call(codec, table):
    import torch
    T = table
    d, size = _laid_out(T, np.arange(len(T.cases)))
    dst = torch.full((size,), FILL, dtype=torch.uint8, device=T.src.device)
    with split_min_1(codec):
        res = codec.decode_big_batch_device(T.src, d, dst)
        torch.cuda.synchronize()
        st = codec.decode_stats()
        assert _judge_image(T.cases, d, res, dst.cpu().numpy()) == []
        cand = [k for k in range(len(d)) if _is_candidate(d[k], len(T.arc), size)]
        # the device walk fills a table sized from the entry's stated size alone (walk_lz4_capacity, host_walk.h): a frame the walker's
        # rule accepts but with more blocks than that is declined there
        accepted = [k for k in cand if T.cases[k]["walk"] and T.cases[k]["nblocks"] <= 2 * -(-T.cases[k]["uncomp"] // 65536) + 8]
        assert len(cand) >= 370 and len(accepted) >= 340
        assert (st["device_walked"], st["device_walk_accepted"]) == (len(cand), len(accepted)), st
        finishable = sum(1 for k in accepted if T.cases[k]["reader"])
        assert 1 <= st["frame_parallel_entries"] <= finishable, st           # (the chooser may leave small frames to one wave)
        # the frame of 520 blocks: within its table's capacity of 546, so the device walk accepts it; alone in a call, nothing competes
        # with it and the counters are its own
        big = [k for k, c in enumerate(T.cases) if c["claims"].get("big")]
        assert len(big) == 1 and big[0] in accepted and T.cases[big[0]]["nblocks"] == 520
        d1, size1 = _laid_out(T, np.array(big))
        dst = torch.full((size1,), FILL, dtype=torch.uint8, device=T.src.device)
        res = codec.decode_big_batch_device(T.src, d1, dst)
        torch.cuda.synchronize()
        st = codec.decode_stats()
        assert _judge_image([T.cases[big[0]]], d1, res, dst.cpu().numpy()) == []
        assert (st["device_walked"], st["device_walk_accepted"], st["frame_parallel_entries"], st["frame_parallel_frames"]) == (1, 1, 1, 520), st


def test_decode_batch_host_all_cases_in_one_call(codec, table):
    T = table
    with split_min_1(codec):
        res, outs = codec.decode_batch_host(T.arc, T.desc)
        st = codec.decode_stats()
    bad = []
    for k, c in enumerate(T.cases):
        if c["rc"] == HASH_MISMATCH:                       # (what lay in the buffer is hashed too: the judges' 0xA5, not the zeros of this call)
            continue
        x = _against_the_record(c, int(res[k]["status"]), int(res[k]["produced"]), int(res[k]["hash"]), outs[k])
        if x:
            bad.append(x)
    assert bad == []
    assert 1 <= st["frame_parallel_entries"] <= sum(c["reader"] for c in T.cases), st


@pytest.mark.parametrize("chunk", [7, 1000])
def test_stream_steps_agree_with_the_oracle(codec, table, chunk):
    """groups B, D, E and F through the resumable stream decoder, whose steps run the same kernels on the blocks that have arrived"""
    from tests.test_gpu_codec import _stream_decode
    o = oracle()
    bad, seen = [], 0
    with split_min_1(codec):
        for c in table.cases:
            if c["group"] not in "BDEF":
                continue
            assert c["cap"] == c["uncomp"]
            seen += 1
            status, got, first = _stream_decode(codec, c["frame"], LZ4, c["uncomp"], c["hash"], chunk, out_chunk=1 << 20)
            if status != c["rc"]:
                bad.append((c["label"], "stream", status, "oracle", c["rc"]))
            elif c["rc"] == OK and (got != c["out"][:c["uncomp"]].tobytes() or o.xxh3(got) != c["hash"]):
                bad.append((c["label"], "bytes"))
    assert seen >= 40
    assert bad == []
