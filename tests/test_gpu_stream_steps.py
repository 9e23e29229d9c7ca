"""GPU: the bounded steps of the stream reader (zpk_stream.inc, stream_plan.h) at the smallest entries at which each rule of a step
can go wrong, with the number of steps pinned EXACTLY against an expectation computed here from the frame's block headers and the go
rule: a step runs at the frame's end, at a full table of 64 blocks, or — the first step — from 4 (LZ4) / 2 (Zstandard) complete
blocks on.  LZ4: (4 + 64 + 64 + 5) blocks of 64 KiB + 777 bytes through a 128 KiB input window: the first step by the 4-block rule,
full steps, a history carried beyond 128 KiB, an end step.  Zstandard, levels 3 and 9: (2 + 64 + 3) blocks of 128 KiB + 777 bytes.
Those sizes end 777 bytes behind a 64 KiB group of the XXH3 sections, where it does not matter how the last group is rounded: one
more entry for each codec ends 40000 bytes behind one, in a group of 39 blocks.  For each codec an entry of 1-2 MiB compressed that arrives in one call and ends in its first step (the XXH3 in one launch instead of
sections).  In the counted runs the output window is 8 MiB, so that a step's output leaves in the call that made it; every entry
once more with windows that fit nothing (input 100000, output 300000): bytes and verdict."""
import numpy as np
import pytest

from benchdata import datagen as dg
import zpack_amd
from tests.test_gpu_codec import _stream_decode

pytestmark = pytest.mark.gpu

K, M = 1 << 10, 1 << 20
WINDOW, OUT_WINDOW = 128 * K, 8 * M


@pytest.fixture(scope="module")
def codec():
    return zpack_amd.Codec(0)


def lz4_blocks(frame):
    """-> (header bytes, [bytes of every block, its 4-byte header included]) of one LZ4 frame; the EndMark follows the last block"""
    f = np.frombuffer(frame, dtype=np.uint8)
    hdr = 7 + (8 if f[4] & 0x08 else 0)
    at, blocks = hdr, []
    while True:
        w = int.from_bytes(f[at:at + 4].tobytes(), "little")
        if w == 0:
            return hdr, blocks
        blocks.append(4 + (w & 0x7FFFFFFF))
        at += blocks[-1]


def zstd_blocks(frame):
    """-> (header bytes, [bytes of every block, its 3-byte header included]) of one Zstandard frame; the last block says so itself"""
    f = np.frombuffer(frame, dtype=np.uint8)
    fhd = int(f[4])
    fcs_flag, single, did = fhd >> 6, (fhd >> 5) & 1, fhd & 3
    hdr = 5 + (0 if single else 1) + (4 if did == 3 else did) + (single if fcs_flag == 0 else (2, 4, 8)[fcs_flag - 1])
    at, blocks = hdr, []
    while True:
        w = int.from_bytes(f[at:at + 3].tobytes(), "little")
        blocks.append(3 + (1 if (w >> 1) & 3 == 1 else w >> 3))
        at += blocks[-1]
        if w & 1:
            return hdr, blocks


def expected_steps(method, frame, window):
    """The go rule over the calls of a reader that feeds `window` bytes per call and takes a step's output in the call that made it:
    -> [(index of the call that takes the step, blocks of the step)]"""
    hdr, blocks = (lz4_blocks if method == dg.LZ4 else zstd_blocks)(frame)
    table, first_min = 64, (4 if method == dg.LZ4 else 2)
    fed, at, nxt, steps, call = 0, hdr, 0, [], -1 # bytes fed; offset of the first pending byte; index of the first pending block
    while True:
        all_in = fed == len(frame)                # (a call without input still steps over what is pending)
        fed = min(fed + window, len(frame))
        call += 1
        if fed < 18:                              # (the header parse may still wait: never with these windows)
            continue
        nb, q, end = 0, at, False
        if method == dg.LZ4:
            while nb < table:
                if nxt + nb == len(blocks):
                    if fed - q >= 4:
                        end, q = True, q + 4
                    break
                if fed - q < blocks[nxt + nb]:
                    break
                q += blocks[nxt + nb]; nb += 1
        else:
            while nb < table and not end and fed - q >= blocks[nxt + nb]:
                q += blocks[nxt + nb]; nb += 1
                end = nxt + nb == len(blocks)
        if end or nb == table or (not steps and nb >= first_min):
            steps.append((call, nb))
            at, nxt = q, nxt + nb
            if end:
                return steps
        else:
            assert not all_in, "the frame does not end"


def _tile(seed, size, front=0):
    """TEXT and RECORDS by turns, 1 MiB each, as in the large-entry tests of test_gpu_codec.py, behind `front` bytes that do not
    compress: they make the first blocks so large that the first step finds exactly as many blocks as it needs"""
    tile = np.concatenate([dg.fill(k % 2, seed, k, M) for k in range(8)])
    return np.ascontiguousarray(np.concatenate([dg.fill(dg.RANDOM, seed, 99, front), np.resize(tile, size - front)]))


def _one_call_entry(seed, size):
    """1 MiB that does not compress in front of a tile that does: 1-2 MiB compressed in fewer than 64 blocks"""
    return np.ascontiguousarray(np.concatenate([dg.fill(dg.RANDOM, seed, 0, M), _tile(seed, size - M)]))


CASES = [("lz4 137 blocks", dg.LZ4, 0, lambda: _tile(1901, (4 + 64 + 64 + 5) * 64 * K + 777, 192 * K), WINDOW),
         ("zstd-3 69 blocks", dg.ZSTD, 3, lambda: _tile(1902, (2 + 64 + 3) * 128 * K + 777, 224 * K), WINDOW),
         ("zstd-9 69 blocks", dg.ZSTD, 9, lambda: _tile(1903, (2 + 64 + 3) * 128 * K + 777, 224 * K), WINDOW),
         ("lz4 71 blocks, short last group", dg.LZ4, 0, lambda: _tile(1906, (4 + 64 + 3) * 64 * K + 40000, 192 * K), WINDOW),
         ("zstd-3 67 blocks, short last group", dg.ZSTD, 3, lambda: _tile(1907, (2 + 64 + 1) * 128 * K + 40000, 224 * K), WINDOW),
         ("lz4 one call", dg.LZ4, 0, lambda: _one_call_entry(1904, 5 * M // 2 + 777), None),
         ("zstd-3 one call", dg.ZSTD, 3, lambda: _one_call_entry(1905, 3 * M + 777), None)]


@pytest.mark.parametrize("label,method,level,make,window", CASES, ids=[c[0].replace(",", "").replace(" ", "-") for c in CASES])
def test_stream_steps_counted_exactly(codec, label, method, level, make, window):
    plain = make()
    frame = dg.compress(method, level, plain)
    size, h, want = len(plain), dg.xxh3(plain), plain.tobytes()
    assert len(frame) >= 1 * M, (label, len(frame))                                      # (the bounded steps start at 1 MiB compressed)
    if window is None:                                                                   # the whole entry in one call; it ends in its first step
        assert len(frame) <= 2 * M, (label, len(frame))
        window = len(frame)
        assert len(expected_steps(method, frame, window)) == 1
    steps = expected_steps(method, frame, window)
    if len(steps) > 1:                                                                   # the first step by the 4-block / 2-block rule, then full tables, then the end
        assert steps[0][1] == (4 if method == dg.LZ4 else 2) and steps[1][1] == 64 and steps[-1][1] < 64, (label, steps)
    for hh, verdict in ((h, 0), (h ^ 4, 15)):                                            # a wrong hash: the verdict with the last byte, the bytes stay
        launches = []
        st, out, _ = _stream_decode(codec, frame, method, size, hh, window, OUT_WINDOW, trace=lambda *a: launches.append(a[5]))
        stats = dict(_stream_decode.stats)
        took = [k for k in range(len(launches)) if launches[k] != (launches[k - 1] if k else 0)]
        print(label, "status", st, "steps", stats["steps"], "in calls", took, "expected", steps, "device", stats["device_peak"], "restarts", stats["restarts"])
        assert st == verdict and out == want, (label, st, stats)
        assert stats["restarts"] == 0 and stats["steps"] == len(steps), (label, stats, steps)
        assert took == [c for c, _ in steps], (label, took, steps)                      # ... each in the call the go rule says
        assert stats["device_peak"] < (64 << 20), (label, stats)
    # windows that fit nothing: bytes and verdict
    for hh, verdict in ((h, 0), (h ^ 4, 15)):
        st, out, _ = _stream_decode(codec, frame, method, size, hh, 100000, 300000)
        assert st == verdict and out == want and _stream_decode.stats["restarts"] == 0, (label, st, _stream_decode.stats)
        assert _stream_decode.stats["device_peak"] < (64 << 20), (label, _stream_decode.stats)
