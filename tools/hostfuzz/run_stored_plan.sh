#!/bin/bash
# CPU, AddressSanitizer + UBSan: which stored entries of a device-resident call are copied and hashed chip-wide, their span table and their
# verdict (zpack_amd/csrc/stored_plan.h: the very header the codec compiles).  tools/hostfuzz/run_stored_plan.sh
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_storedplan.XXXXXX)     # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -Wall -Wno-unused-function -I zpack_amd/csrc -o "$work/stored_plan" tools/hostfuzz/stored_plan_main.cpp
"$work/stored_plan"
