#!/bin/bash
# CPU, AddressSanitizer + UBSan: the pitch of a placed read, its rule and extent, the row table of k_place_copy and the placed offsets, every
# item walked as the kernel walks it, in place too (zpack_amd/csrc/place_copy_plan.h over window_copy_plan.h: the very headers the codec compiles).  tools/hostfuzz/run_place_copy_plan.sh
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_placecopyplan.XXXXXX)    # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -Wall -Wno-unused-function -I zpack_amd/csrc -o "$work/place_copy_plan" tools/hostfuzz/place_copy_plan_main.cpp
"$work/place_copy_plan" "$@"
