#!/usr/bin/env python3
"""Developer: which route every entry takes through the three read calls that know large entries, and what comes out, as text that two
builds can be compared by (a refactor of the read side prints the same bytes before and after).

The inputs are those of tests/test_gpu_big_batch_device.py (the mixed batch, the 41 damaged copies) and the mixed batch of
tests/test_gpu_stored_span.py, built from benchdata alone.  Each goes through zpk_codec_decode_batch_host (one call), through
zpk_codec_decode_big_batch_device (one call) and through zpk_codec_decode_big_device (one call per entry).  Per call one line: the 16
words of zpk_codec_decode_stats2 and a SHA-256 over (status, detail, produced, hash, output bytes) of its entries — the bytes of an
entry that finished (status 0 or 15) — and, for the device calls, over everything outside the slots (the guard bytes).

  python tools/route_identity.py > route.txt"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zpack_amd                                                       # noqa: E402
from benchdata import datagen as dg                                    # noqa: E402
from zpack_amd import METHOD_NONE, METHOD_ZSTD, METHOD_LZ4, OPT_ENC_SPLIT_MIN  # noqa: E402

K, M, GUARD = 1 << 10, 1 << 20, 0xEE


def mixed_batch(codec):
    import tests.test_gpu_big_batch_device as T
    items = []
    for i, (label, m, lv, cls, n) in enumerate(T.BIG):
        plain = dg.fill(cls, 501, i, n)
        pay = T._written_in_pieces(codec, plain) if lv < 0 else np.frombuffer(dg.compress(m, lv, plain), dtype=np.uint8)
        items.append((m, np.array(pay, dtype=np.uint8), len(pay), n, dg.xxh3(plain), n, 0))
    for i, (m, lv, n) in enumerate(T.SMALL):
        plain = dg.fill(i % 2, 502, i, n)
        pay = plain if m == METHOD_NONE else np.frombuffer(dg.compress(m, lv, plain), dtype=np.uint8)
        items.append((m, np.array(pay, dtype=np.uint8), len(pay), n, dg.xxh3(plain), n, 0))
    return items, 64


def damaged_copies(codec):
    import tests.test_gpu_big_batch_device as T
    items = []
    for m, lv in ((METHOD_LZ4, 0), (METHOD_ZSTD, 3)):
        plain = dg.fill(dg.TEXT, 503, m, 512 * K)
        good = np.array(np.frombuffer(dg.compress(m, lv, plain), dtype=np.uint8))
        h, n, cs = dg.xxh3(plain), len(plain), len(good)
        hdrs = T._block_header_offsets(good, m)
        body = hdrs[len(hdrs) // 2] + 40

        def flip(at, bit=0x10):
            b = good.copy(); b[at] ^= bit
            return b
        for pay, c, u, hh, cap in [(good, cs, n, h, n), (flip(4, 0x20), cs, n, h, n), (flip(5, 0x01), cs, n, h, n), (flip(hdrs[0]), cs, n, h, n),
                                   (flip(hdrs[0] + 1, 0x01), cs, n, h, n), (flip(hdrs[len(hdrs) // 2]), cs, n, h, n),
                                   (flip(hdrs[len(hdrs) // 2] + 2, 0x40), cs, n, h, n), (flip(hdrs[-1]), cs, n, h, n), (flip(hdrs[-1], 0x01), cs, n, h, n),
                                   (flip(body), cs, n, h, n), (flip(hdrs[1] + 9, 0x04), cs, n, h, n), (flip(hdrs[-1] + 30, 0x80), cs, n, h, n),
                                   (flip(cs - 1, 0x02), cs, n, h, n), (good, cs - 1, n, h, n), (good, cs + 1, n, h, n), (good, cs, n + 1, h, n + 1),
                                   (good, cs, n - 1, h, n), (good, cs, n + 1, h, n), (good, cs, n, h ^ 1, n), (good, cs, n, h, n - 1)]:
            items.append((m, pay, c, u, hh, cap, 0))
    plain = dg.fill(dg.TEXT, 503, METHOD_LZ4, 512 * K)
    good = np.array(np.frombuffer(dg.compress(METHOD_LZ4, 0, plain), dtype=np.uint8))
    items.append((METHOD_LZ4, good, len(good), len(plain), dg.xxh3(plain), len(plain), 0))          # ends where the archive ends
    return items, 0


def stored_mixed(codec):
    plain = dg.fill(dg.RANDOM, 1701, 0, 8 * M + 3)
    items = []
    for m, lv, n in ((METHOD_LZ4, 0, 1 * M), (METHOD_ZSTD, 3, 512 * K)):
        t = dg.fill(dg.TEXT, 1702, m, n)
        pay = np.frombuffer(dg.compress(m, lv, t), dtype=np.uint8)
        items.append((m, pay, len(pay), n, dg.xxh3(t), n, 0))
    for i, (m, n) in enumerate([(m, n) for m in (METHOD_NONE, METHOD_LZ4, METHOD_ZSTD) for n in (4 * K, 64 * K + 5)]):
        t = dg.fill(i % 2, 1703, i, n)
        pay = t if m == METHOD_NONE else np.frombuffer(dg.compress(m, 1 if m == METHOD_ZSTD else 0, t), dtype=np.uint8)
        items.append((m, pay, len(pay), n, dg.xxh3(t), n, 0))
    for n in (300 * K, 1 * M + 5, 8 * M + 3):
        items.append((METHOD_NONE, plain[:n], n, n, dg.xxh3(plain[:n]), n, 0))
    return items, 64


def stats2(codec):
    b = (C.c_uint32 * 16)()
    codec.L.zpk_codec_decode_stats2.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    assert codec.L.zpk_codec_decode_stats2(codec.h, b) == 0
    return " ".join("%u" % x for x in b)


def digest(res, d, slot_bytes, outside=None):
    h = hashlib.sha256()
    for i in range(len(d)):
        st, produced = int(res["status"][i]), int(res["produced"][i])
        h.update(np.array([st, int(res["detail"][i]), produced, int(res["hash"][i])], dtype=np.uint64).tobytes())
        if st in (0, 15):
            h.update(slot_bytes(i)[:min(produced, int(d["dst_capacity"][i]))].tobytes())
    if outside is not None:
        h.update(outside.tobytes())
    return h.hexdigest()


def main():
    import torch
    from tests.test_gpu_stored_span import _batch
    dev = torch.device("cuda:0")
    codec = zpack_amd.Codec(0)
    codec.set_option(OPT_ENC_SPLIT_MIN, 2 * M)
    for name, make in (("mixed", mixed_batch), ("damaged", damaged_copies), ("stored-mixed", stored_mixed)):
        items, tail = make(codec)
        arc, d, total = _batch(items, tail=tail)
        res, outs = codec.decode_batch_host(arc, d)
        print("%s host n=%d | %s | %s" % (name, len(d), stats2(codec), digest(res, d, lambda i: outs[i])))
        src = torch.from_numpy(arc).to(dev)

        def device_call(fn, sub):
            dst = torch.full((total,), GUARD, dtype=torch.uint8, device=dev)
            r = fn(src, sub, dst)
            s2 = stats2(codec)
            out = dst.cpu().numpy()
            inside = np.zeros(len(out), dtype=bool)
            for x in sub:
                inside[int(x["dst_offset"]):int(x["dst_offset"]) + int(x["dst_capacity"])] = True
            r = np.atleast_1d(np.asarray(r, dtype=zpack_amd.DECODE_RESULT))
            return s2, digest(r, sub, lambda i: out[int(sub["dst_offset"][i]):], out[~inside])
        print("%s big_batch_device n=%d | %s | %s" % ((name, len(d)) + device_call(codec.decode_big_batch_device, d)))
        for i in range(len(d)):
            print("%s big_device entry %d | %s | %s" % ((name, i) + device_call(codec.decode_big_device, d[i:i + 1])))
    codec.close()


if __name__ == "__main__":
    main()
