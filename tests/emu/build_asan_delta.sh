#!/bin/sh
# AddressSanitizer + UBSan build of the delta filter's kernels (split with delta, tile sums, tile offsets, join-scan-store) under the host wave emulator, as a
# stand-alone PROGRAM (its own main in delta_planes_main.cpp; nothing is loaded into python, no LD_PRELOAD), in the form of build_asan_typed.sh.
#   sh tests/emu/build_asan_delta.sh && /tmp/delta_planes_asan
set -e
cd "$(dirname "$0")"
g++ -O1 -g -std=c++17 -I. -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wno-unused-function -Wno-unused-variable -o ${1:-/tmp/delta_planes_asan} zhemu.cpp delta_planes_main.cpp
