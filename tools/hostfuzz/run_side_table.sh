#!/bin/bash
# CPU: the side tables of the host library (zpack_amd/host/util.c, the very source libzpack_amd.so compiles) under a stand-alone driver,
# built and run twice: AddressSanitizer + UBSan, then ThreadSanitizer.
# tools/hostfuzz/run_side_table.sh
set -e
cd "$(dirname "$0")/../.."
work=$(mktemp -d -t zpk_sidetable.XXXXXX)        # private to this run: a directory left by another user cannot block it
trap 'rm -rf "$work"' EXIT
flags="-O1 -g -std=c11 -Wall -Wextra -D_FILE_OFFSET_BITS=64 -D_POSIX_C_SOURCE=200809L -I include -I zpack_amd/host"
for san in address,undefined thread; do
    echo "== -fsanitize=$san"
    gcc $flags -fsanitize=$san -fno-sanitize-recover=all -o "$work/side_table" tools/hostfuzz/side_table_main.c zpack_amd/host/util.c -lpthread
    "$work/side_table"
done
