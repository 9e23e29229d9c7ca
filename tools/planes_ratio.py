#!/usr/bin/env python3
"""What byte planes gain through THIS project's device encoders: compressed size over plain size of float tensors written as they are
and written grouped (zpack_amd/device_io.py, planes=), beside the figures of the CPU libraries.

  python tools/planes_ratio.py [--mib 64]

bf16, fp16 and fp32 tensors of torch.randn * 0.02 (seeded), --mib MiB per dtype as entries of 1 MiB, at LZ4 level 0 and Zstandard levels
1 and 3.  Every archive is read back (grouped ones with the same element sizes) and compared with the tensors: a figure is printed only
for an archive that round-trips.  The sizes are the entries' compressed bytes: the archive without header, CDR and EOCDR."""
import argparse
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# liblz4 1.9.3 and libzstd 1.4.9 on a CPU, 1 Mi values of randn * 0.02: as is -> grouped
CPU = {"bf16": {"zstd-1": (0.780, 0.684), "zstd-3": (0.780, 0.710), "lz4": (1.004, 0.846)},
       "fp16": {"zstd-1": (0.918, 0.843), "zstd-3": (0.918, 0.843), "lz4": (1.004, 1.004)},
       "fp32": {"zstd-1": (0.923, 0.842), "zstd-3": (0.923, 0.855), "lz4": (1.004, 0.926)}}


def main():
    import torch
    from zpack_amd import device_io as io
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(28)
    codecs = (("lz4", io.METHOD_LZ4, 0), ("zstd-1", io.METHOD_ZSTD, 1), ("zstd-3", io.METHOD_ZSTD, 3))
    print("compressed size / plain size, %d MiB per dtype as entries of 1 MiB, randn * 0.02; 'as is -> grouped'" % a.mib)
    print("| dtype | codec | this encoder (device) | CPU library | gain here | gain of the CPU library |")
    print("|---|---|---|---|---|---|")
    for tag, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16), ("fp32", torch.float32)):
        k = torch.empty(0, dtype=dt).element_size()
        tensors = {"%s.%03d" % (tag, i): (torch.randn((1 << 20) // k, generator=g, device=dev) * 0.02).to(dt) for i in range(a.mib)}
        plain_bytes = a.mib << 20
        fixed = 10 + 20 + sum(35 + len(n) for n in tensors) + 12
        for name, method, level in codecs:
            r = []
            for planes in (None, {n: k for n in tensors}):
                image = io.write_archive_device(tensors, method=method, level=level, planes=planes)
                outs, status = io.read_files_device(image, planes=planes)
                ok = status == [0] * len(tensors) and all(torch.equal(o.view(dt), t) for o, t in zip(outs, tensors.values()))
                if not ok:
                    raise SystemExit("%s %s planes=%s: the archive does not read back" % (tag, name, "yes" if planes else "no"))
                assert io.test_files(image) == [0] * len(tensors)
                r.append((image.numel() - fixed) / plain_bytes)
                del image, outs
            c = CPU[tag][name]
            gain = 1 - r[1] / r[0]
            print("| %s | %s | %.3f -> %.3f | %.3f -> %.3f | %+.1f %% | %+.1f %% |%s" % (tag, name, r[0], r[1], c[0], c[1], -100 * gain, -100 * (1 - c[1] / c[0]),
                                                                                     "  (grouping gains nothing here)" if r[1] >= r[0] * 0.995 else ""))
        del tensors
    print("every archive above was read back bit-exact and passes zpack_amd_test_files")


if __name__ == "__main__":
    main()
