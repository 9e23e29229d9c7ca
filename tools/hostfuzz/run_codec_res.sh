#!/bin/bash
# CPU, AddressSanitizer + UBSan: the owning types of the codec's HIP resources (zpack_amd/csrc/codec_res.h: the very header the codec
# compiles) against a counting stand-in for the HIP runtime (tools/hostfuzz/fakehip).  tools/hostfuzz/run_codec_res.sh
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_codecres.XXXXXX)         # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 -Wall -Wno-unused-function -I tools/hostfuzz/fakehip -I zpack_amd/csrc -o "$work/codec_res" tools/hostfuzz/codec_res_main.cpp
"$work/codec_res"
