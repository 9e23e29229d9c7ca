#!/bin/bash
# CPU, AddressSanitizer + UBSan: the row table, work items and launches of k_span_copy, the staging slots of a sub-batch, the offsets of the
# packed device read and the pointer test (zpack_amd/csrc/span_copy_plan.h over copy_rows_plan.h: the very headers the codec compiles).  tools/hostfuzz/run_span_copy_plan.sh
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_spancopyplan.XXXXXX)     # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -Wall -Wno-unused-function -I zpack_amd/csrc -o "$work/span_copy_plan" tools/hostfuzz/span_copy_plan_main.cpp
"$work/span_copy_plan"
