#!/bin/bash
# CPU, AddressSanitizer + UBSan: the bounded steps of the stream reader — the intake rule and the go rule as tables, whole streams simulated
# over synthetic frames (blocks, hash sections, history carry, pending bytes), the two device layouts (zpack_amd/csrc/stream_plan.h: the
# very header the codec compiles).  tools/hostfuzz/run_stream_plan.sh
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_streamplan.XXXXXX)     # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -Wall -Wno-unused-function -I zpack_amd/csrc -o "$work/stream_plan" tools/hostfuzz/stream_plan_main.cpp
"$work/stream_plan" "$@"
