#!/bin/bash
# CPU, AddressSanitizer + UBSan: the sub-batches of a batch read out of an archive image in device memory and their staging slots
# (zpack_amd/csrc/dimage_plan.h: the very header the codec compiles).  tools/hostfuzz/run_dimage_plan.sh
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_dimageplan.XXXXXX)       # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -Wall -Wno-unused-function -I zpack_amd/csrc -o "$work/dimage_plan" tools/hostfuzz/dimage_plan_main.cpp
"$work/dimage_plan"
