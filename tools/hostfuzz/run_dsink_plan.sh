#!/bin/bash
# CPU, AddressSanitizer + UBSan: a batch compressed into a bounded sink in device memory — the cut, the span table, room and chaining,
# the staging slots (zpack_amd/csrc/dsink_plan.h: the very header the codec and the commit kernels compile).
# tools/hostfuzz/run_dsink_plan.sh [cut ROOM STATUS:SIZE ...]
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_dsinkplan.XXXXXX)        # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -Wall -Wno-unused-function -I zpack_amd/csrc -o "$work/dsink_plan" tools/hostfuzz/dsink_plan_main.cpp
"$work/dsink_plan" "$@"
