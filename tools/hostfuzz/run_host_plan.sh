#!/bin/bash
# CPU, AddressSanitizer + UBSan: the host-pointer read path's decisions — slot and cut, gathered image, pipeline pieces, copy shares,
# frame-parallel groups, small rules — against the loops they replaced and against properties that hold without those
# (zpack_amd/csrc/host_plan.h: the very header the codec compiles).  tools/hostfuzz/run_host_plan.sh
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_hostplan.XXXXXX)         # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -Wall -Wno-unused-function -I zpack_amd/csrc -o "$work/host_plan" tools/hostfuzz/host_plan_main.cpp
"$work/host_plan"
