#!/bin/bash
# CPU, AddressSanitizer + UBSan: the plan of an entry written in pieces, its frame envelope and its verdict (zpack_amd/csrc/enc_plan.h: the
# very header the codec compiles; the envelope also through the header parsers of host_walk.h).  tools/hostfuzz/run_enc_plan.sh
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_encplan.XXXXXX)        # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -Wall -Wno-unused-function -I zpack_amd/csrc -o "$work/enc_plan" tools/hostfuzz/enc_plan_main.cpp
"$work/enc_plan"
