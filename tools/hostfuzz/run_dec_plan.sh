#!/bin/bash
# CPU, AddressSanitizer + UBSan: a large entry's route on the read side — the candidate rule, the chooser against recorded decisions, the
# staging layout of k_big_walk, the hash verdict (zpack_amd/csrc/dec_plan.h: the very header the codec compiles).  tools/hostfuzz/run_dec_plan.sh
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_decplan.XXXXXX)        # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -Wall -Wno-unused-function -I zpack_amd/csrc -o "$work/dec_plan" tools/hostfuzz/dec_plan_main.cpp
"$work/dec_plan" "$@"
