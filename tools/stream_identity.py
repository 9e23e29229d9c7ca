#!/usr/bin/env python3
"""Developer: what the stream reader answers call by call, as text that two builds can be compared by (a refactor of zpk_stream.inc
prints the same bytes before and after).

The entries are those of tests/test_gpu_stream_steps.py (counted windows and the windows that fit nothing), the damaged variants of the
two large-entry tests of tests/test_gpu_codec.py cut down to 3 MiB (bytes behind the end, two frames, truncated, claims less, claims
more, flipped bits), Zstandard levels 1 and 15, and the classes TEXT, RUNS and RANDOM, all through zpk_dstream_step /
zpk_dstream_replay.  Per call one line: rc, consumed, produced, done, wants_input (-1: the call is a replay), launches, device bytes;
per entry the final status and a SHA-256 over the bytes handed out.  --digest: one line per entry, the call lines as their count
and a SHA-256 over them (what profiles/ keeps).

  python tools/stream_identity.py [--digest] > stream.txt          (ZPACK_AMD_CODEC_SO selects the build)"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zpack_amd                                                       # noqa: E402
from benchdata import datagen as dg                                    # noqa: E402
from tests.test_gpu_codec import _stream_decode                         # noqa: E402
import tests.test_gpu_stream_steps as T                                # noqa: E402

K, M = 1 << 10, 1 << 20


def entries():
    for label, method, level, make, window in T.CASES:
        plain = make()
        frame = dg.compress(method, level, plain)
        h = dg.xxh3(plain)
        for hh in (h, h ^ 4):
            yield "%s hash^%d" % (label, h ^ hh), method, frame, len(plain), hh, window or len(frame), T.OUT_WINDOW
            yield "%s hash^%d tight" % (label, h ^ hh), method, frame, len(plain), hh, 100000, 300000
    for level in (1, 15):
        plain = T._tile(1911, 20 * 128 * K + 777)
        yield "zstd-%d 20 blocks" % level, dg.ZSTD, dg.compress(dg.ZSTD, level, plain), len(plain), dg.xxh3(plain), T.WINDOW, M
    for method, level in ((dg.LZ4, 0), (dg.ZSTD, 3), (dg.ZSTD, 9)):
        for cls in (dg.TEXT, dg.RUNS, dg.RANDOM):
            plain = dg.fill(cls, 1912, 0, 6 * M)
            yield "m%d-%d class %d" % (method, level, cls), method, dg.compress(method, level, plain), len(plain), dg.xxh3(plain), 100000, 300000
    small = 3 * M
    for method, level, seed in ((dg.LZ4, 0, 9), (dg.ZSTD, 3, 10)):
        p2 = T._one_call_entry(1913, small)
        f2 = bytearray(dg.compress(method, level, p2))
        h2 = dg.xxh3(p2)
        rng = np.random.default_rng(seed)
        variants = [("bytes behind the end", bytes(f2) + b"\0\0\0", small, h2),
                    ("two frames", bytes(f2) + bytes(f2), 2 * small, dg.xxh3(np.concatenate([p2, p2]))),
                    ("truncated", bytes(f2[:-9]), small, h2),
                    ("claims less", bytes(f2), small - 1000, h2),
                    ("claims more", bytes(f2), small + 1000, h2)]
        for k in range(6):
            b = bytearray(f2); at = int(rng.integers(len(b) // 3, len(b))); b[at] ^= 0x55 if method == dg.LZ4 else 1 << int(rng.integers(0, 8))
            variants.append(("flip@%d" % at, bytes(b), small, h2))
        for label, payload, usize, hh in variants:
            yield "m%d %s" % (method, label), method, payload, usize, hh, T.WINDOW, M


def main():
    digest = "--digest" in sys.argv
    codec = zpack_amd.Codec(0)
    for label, method, frame, usize, hh, window, out_window in entries():
        calls = []
        st, out, first = _stream_decode(codec, frame, method, usize, hh, window, out_window,
                                        trace=lambda *a: calls.append("  rc %d consumed %d produced %d done %d wants %d launches %d device %d" % a))
        head = "== %s: comp %d uncomp %d window %d / %d" % (label, len(frame), usize, window, out_window)
        tail = "-> status %d bytes %d first %s restarts %d sha256 %s" % (st, len(out), first, _stream_decode.stats["restarts"], hashlib.sha256(out).hexdigest())
        if digest:
            print("%s: %d calls %s %s" % (head, len(calls), hashlib.sha256("\n".join(calls).encode()).hexdigest()[:16], tail), flush=True)
        else:
            print("\n".join([head] + calls + [tail]), flush=True)
    codec.close()


if __name__ == "__main__":
    main()
