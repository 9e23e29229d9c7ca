#!/bin/bash
# CPU, AddressSanitizer + UBSan: which device spans one wave hashes and which the whole chip, the tables, the partial-sum layout and the
# launches of k_span_hash and the chip-wide pair, every row and group walked as the kernels walk them (zpack_amd/csrc/span_hash_plan.h:
# the very header the codec compiles).  tools/hostfuzz/run_span_hash_plan.sh [--pin THRESHOLD MAX_GROUPS]
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_spanhashplan.XXXXXX)     # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -Wall -Wno-unused-function -I zpack_amd/csrc -o "$work/span_hash_plan" tools/hostfuzz/span_hash_plan_main.cpp
"$work/span_hash_plan" "$@"
