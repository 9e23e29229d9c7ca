#!/bin/bash
# CPU, AddressSanitizer + UBSan: the block walk over ONE large frame in the form the device runs (k_big_walk: walk_lz4_single_into,
# walk_zstd_single_into of zpack_amd/csrc/host_walk.h, tables of fixed capacity) against the vector walkers of the host paths, on
# intact and mutated frames: the same verdict and a byte-identical table wherever the table holds the frame, a decline wherever it does
# not, nothing read outside the entry, nothing written behind the table.  tools/hostfuzz/run_big_walk.sh [iterations]
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_bigwalk.XXXXXX)        # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -I zpack_amd/csrc -o "$work/big_walk" tools/hostfuzz/big_walk_main.cpp
"$work/big_walk" ${1:-1000000}
