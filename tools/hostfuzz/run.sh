#!/bin/bash
# CPU, AddressSanitizer + UBSan: the HOST code that walks untrusted frame and block headers for the frame-parallel and block-parallel
# readers and the stream steps (zpack_amd/csrc/host_walk.h: the very header the codec compiles) on mutated frames: no read outside the
# entry, every accepted plan tiles its entry exactly, every block inside the bytes given.  tools/hostfuzz/run.sh [iterations]
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_hostfuzz.XXXXXX)       # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -I zpack_amd/csrc -o "$work/walk_fuzz" tools/hostfuzz/walk_fuzz_main.cpp
"$work/walk_fuzz" ${1:-3000000}
