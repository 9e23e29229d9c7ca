#!/usr/bin/env python3
"""What a placed read saves, and what k_place_copy costs beside k_window_copy.

  python tools/place_read_rate.py [--entries 2000] [--pairs 7]

--entries bf16 tensors of 1 MiB, each a (512, 1024) matrix, written as 8 COLUMN SHARDS of (512, 128) — 8 x --entries byte-plane entries
(element size 2) of 128 KiB at LZ4 level 0 in a sink in device memory — and read out of that image into the merged tensors.  After a
warm-up round --pairs rounds alternate the legs; medians and ranges.

(a) the call: zpk_codec_decode_batch_dimage_placed, every shard a sub-block of 512 rows of 256 bytes at pitch 2048 of its tensor,
    against what a caller does today — the whole read of every shard into scratch, then the concatenation along the columns (as ONE
    permuted copy of all tensors, the cheapest form of --entries torch.cat calls; its allocation is inside the clock: the caller pays it).
(b) the kernels alone on the same stored bytes: k_place_copy into the merged tensors against k_plane_copy joining the shards whole
    plus that concatenation; and k_place_copy at pitch == cols against k_window_copy on the same rows."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS, COLS, K, TP = 512, 1024, 2, 8              # the tensor: 512 x 1024 bf16, 8 column shards
SIZE = ROWS * COLS * K
SHARD = SIZE // TP
CB = COLS * K // TP                              # a shard's row: 256 bytes
PITCH = COLS * K


def stat(xs):
    return "median %8.3f ms  (%8.3f .. %8.3f)" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=7)
    a = ap.parse_args()
    import torch
    import zpack_amd as Z
    nt = a.entries
    n = nt * TP
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(38)
    merged = torch.empty(nt * SIZE, dtype=torch.uint8, device=dev)                      # the tensors as the loader wants them
    for i in range(0, nt, 100):
        m = min(100, nt - i)
        merged[i * SIZE:(i + m) * SIZE] = (torch.randn(m * SIZE // K, generator=g, device=dev) * 0.02).to(torch.bfloat16).view(torch.uint8)

    def cat(scratch):
        """shard-major scratch (entry t * 8 + r is shard r of tensor t) -> the merged tensors: torch.cat along the columns, all at once"""
        return scratch.view(nt, TP, ROWS, CB).permute(0, 2, 1, 3).contiguous().view(-1)

    src = merged.view(nt, ROWS, TP, CB).permute(0, 2, 1, 3).contiguous().view(-1)      # what the 8 ranks wrote
    assert torch.equal(cat(src), merged)
    codec = Z.Codec(0)
    L = Z.lib()
    vp, u64 = C.c_void_p, C.c_uint64
    L.zpk_codec_encode_batch_dsink_delta.argtypes = [vp, vp, C.c_int, vp, u64, vp, u64, vp, C.POINTER(u64), C.POINTER(u64), vp, vp]
    L.zpk_codec_decode_batch_dimage_windows.argtypes = [vp, vp, u64, vp, u64, vp, C.c_int, vp, vp, vp, vp, vp]
    L.zpk_codec_decode_batch_dimage_placed.argtypes = [vp, vp, u64, vp, u64, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    bound = codec.compress_bound(Z.METHOD_LZ4, SHARD)
    sink = torch.empty(n * bound + 64, dtype=torch.uint8, device=dev)
    ed = np.zeros(n, dtype=Z.ENCODE_DESC)
    ed["size"], ed["method"], ed["level"], ed["dst_capacity"] = SHARD, Z.METHOD_LZ4, 0, bound
    dense = lambda t: (vp * n)(*[t.data_ptr() + i * SHARD for i in range(n)])
    out = torch.empty(nt * SIZE, dtype=torch.uint8, device=dev)
    scratch = torch.empty(nt * SIZE, dtype=torch.uint8, device=dev)
    place_addr = lambda t: [t.data_ptr() + (i // TP) * SIZE + (i % TP) * CB for i in range(n)]
    elem = (C.c_uint8 * n)(*([K] * n))
    torch.cuda.synchronize()

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    res = np.zeros(n, dtype=Z.ENCODE_RESULT)
    placed, nbytes = u64(0), u64(0)
    rc = L.zpk_codec_encode_batch_dsink_delta(codec.h, dense(src), 1, ed.ctypes.data, n, sink.data_ptr(), sink.numel(), res.ctypes.data, C.byref(placed), C.byref(nbytes), elem, None)
    assert rc == 0 and placed.value == n and (res["status"] == 0).all()
    dd = np.zeros(n, dtype=Z.DECODE_DESC)
    dd["comp_size"] = res["comp_size"]
    dd["src_offset"] = np.concatenate([[0], np.cumsum(dd["comp_size"])[:-1]])
    dd["uncomp_size"] = dd["dst_capacity"] = SHARD
    dd["expect_hash"] = res["hash"]
    dd["method"] = Z.METHOD_LZ4
    image = sink[:nbytes.value + 1]                                                    # (a pad byte behind the payloads keeps the last entry inside)
    print("%d x 1 MiB bf16 as (512, 1024), each written as 8 column shards of (512, 128): %d byte-plane entries (element size 2) of 128 KiB, LZ4 level 0, "
          "compressed/plain %.3f; %d alternating rounds behind one warm-up round" % (nt, n, nbytes.value / (nt * SIZE), a.pairs))

    whole = (CB, 0, ROWS, 0, CB)                                                        # a shard whole, as 512 rows of 256 bytes
    wins = np.array([whole] * n, dtype=Z.WINDOW)
    pitches = np.full(n, PITCH, dtype=np.uint64)
    pdd = dd.copy()
    pdd["dst_capacity"] = (ROWS - 1) * PITCH + CB                                       # the extent
    p_dst = (vp * n)(*place_addr(out))
    s_dst = dense(scratch)

    def read_placed():
        r = np.zeros(n, dtype=Z.DECODE_RESULT)
        rc = L.zpk_codec_decode_batch_dimage_placed(codec.h, image.data_ptr(), image.numel(), pdd.ctypes.data, n, p_dst, 1, r.ctypes.data, elem, None, None, wins.ctypes.data,
                                                    pitches.ctypes.data)
        assert rc == 0 and (r["status"] == 0).all()
        return out

    def read_scratch_then_cat():
        r = np.zeros(n, dtype=Z.DECODE_RESULT)
        rc = L.zpk_codec_decode_batch_dimage_windows(codec.h, image.data_ptr(), image.numel(), dd.ctypes.data, n, s_dst, 1, r.ctypes.data, elem, None, None, None)
        assert rc == 0 and (r["status"] == 0).all()
        return cat(scratch)

    legs = {"placed call": read_placed, "read to scratch + cat": read_scratch_then_cat}
    times = {leg: [] for leg in legs}
    for rep in range(a.pairs + 1):
        for leg, fn in legs.items():
            if rep == 0:
                out.zero_()
            ms, got = clock(fn)
            if rep:
                times[leg].append(ms)
            else:
                assert torch.equal(got, merged), "%s: not the merged tensors" % leg
            del got
    print("(a) out of a device image, 8 shards merged into every tensor (both legs returned the merged tensors bit-exact):")
    for leg in legs:
        print("    %-22s: %s" % (leg, stat(times[leg])))
    p, s = statistics.median(times["placed call"]), statistics.median(times["read to scratch + cat"])
    print("    the placed call takes %.3f of read to scratch + cat (%.3f ms less); HBM for the destinations: %d MiB against %d + %d MiB" %
          (p / s, s - p, nt * SIZE >> 20, nt * SIZE >> 20, nt * SIZE >> 20))

    # ---- (b) the kernels alone, on the stored bytes of the same entries ----
    stored = torch.empty(nt * SIZE, dtype=torch.uint8, device=dev)
    srow = np.zeros(n, dtype=Z.PLANE_COPY)
    srow["src"], srow["dst"], srow["len"], srow["elem"], srow["join"] = list(dense(src)), list(dense(stored)), SHARD, K, 0
    codec.plane_copy_device(srow)                                                      # stored = split(shard)
    torch.cuda.synchronize()
    stptr = list(dense(stored))
    prow = np.zeros(n, dtype=Z.PLANE_COPY)
    prow["src"], prow["dst"], prow["len"], prow["elem"], prow["join"] = stptr, list(s_dst), SHARD, K, 1

    def place_rows(dst, pitch):
        t = np.zeros(n, dtype=Z.PLACE_COPY)
        t["src"], t["dst"], t["n"], t["elem"], t["pitch"] = stptr, dst, SHARD, K, pitch
        t["win"] = wins
        return t

    wrow = np.zeros(n, dtype=Z.WINDOW_COPY)
    wrow["src"], wrow["dst"], wrow["n"], wrow["elem"] = stptr, list(s_dst), SHARD, K
    wrow["win"] = wins
    merged_rows, dense_rows = place_rows(place_addr(out), PITCH), place_rows(list(s_dst), CB)
    kt = {"k_place_copy, pitch 2048 (merged)": [], "k_plane_copy join whole + cat": [], "k_plane_copy join whole": [], "k_window_copy, dense": [], "k_place_copy, pitch == cols": []}
    for rep in range(a.pairs + 1):
        for name in kt:
            if rep == 0:
                out.zero_(); scratch.zero_()
            if name.startswith("k_place_copy, pitch 2048"):
                ms, got = clock(lambda: (codec.place_copy_device(merged_rows), out)[1])
            elif name.endswith("+ cat"):
                ms, got = clock(lambda: (codec.plane_copy_device(prow), cat(scratch))[1])
            elif name.startswith("k_plane"):
                ms, got = clock(lambda: (codec.plane_copy_device(prow), scratch)[1])
            elif name.startswith("k_window"):
                ms, got = clock(lambda: (codec.window_copy_device(wrow), scratch)[1])
            else:
                ms, got = clock(lambda: (codec.place_copy_device(dense_rows), scratch)[1])
            if rep == 0:
                assert torch.equal(got, src if got is scratch else merged), name
            else:
                kt[name].append(ms)
            del got
    print("(b) the kernels alone (table upload + launch + kernel, %d rows; every kernel's bytes were checked):" % n)
    for name, xs in kt.items():
        moved = (4 if name.endswith("+ cat") else 2) * nt * SIZE
        print("    %-36s: %s   %7.1f GB/s over the %.2f GB it moves" % (name, stat(xs), moved / 1e9 / (statistics.median(xs) / 1e3), moved / 1e9))
    med = {k: statistics.median(v) for k, v in kt.items()}
    print("    k_place_copy at pitch == cols / k_window_copy on the same rows: %.3f  (k_window_copy's own range: %.3f .. %.3f of its median)" %
          (med["k_place_copy, pitch == cols"] / med["k_window_copy, dense"], min(kt["k_window_copy, dense"]) / med["k_window_copy, dense"],
           max(kt["k_window_copy, dense"]) / med["k_window_copy, dense"]))
    print("    k_place_copy into the merged tensors / k_plane_copy join whole + cat: %.3f" % (med["k_place_copy, pitch 2048 (merged)"] / med["k_plane_copy join whole + cat"]))
    codec.close()


if __name__ == "__main__":
    main()
