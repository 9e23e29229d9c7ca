#!/bin/bash
# CPU, AddressSanitizer + UBSan: the layout of a byte-plane entry, the row table, work items and launches of k_plane_copy
# (zpack_amd/csrc/plane_copy_plan.h over copy_rows_plan.h: the very headers the codec compiles).  Arguments go to the program (`dump`: the stored side of every
# case, for a model to compare with).  tools/hostfuzz/run_plane_copy_plan.sh
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_planecopyplan.XXXXXX)    # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -Wall -Wno-unused-function -I zpack_amd/csrc -o "$work/plane_copy_plan" tools/hostfuzz/plane_copy_plan_main.cpp
"$work/plane_copy_plan" "$@"
