#!/bin/bash
# CPU, AddressSanitizer + UBSan: the window of a window read, its rule and the row table of k_window_copy, every item walked as the kernel
# walks it, in place too (zpack_amd/csrc/window_copy_plan.h over copy_rows_plan.h: the very headers the codec compiles).  tools/hostfuzz/run_window_copy_plan.sh
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_windowcopyplan.XXXXXX)   # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -Wall -Wno-unused-function -I zpack_amd/csrc -o "$work/window_copy_plan" tools/hostfuzz/window_copy_plan_main.cpp
"$work/window_copy_plan" "$@"
