#!/bin/sh
# AddressSanitizer + UBSan build of the xor-with-base filter's kernels (split with xor, join with xor) under the host wave emulator, as a stand-alone PROGRAM
# (its own main in xor_planes_main.cpp; nothing is loaded into python), in the form of build_asan_delta.sh.
#   sh tests/emu/build_asan_xor.sh && /tmp/xor_planes_asan
set -e
cd "$(dirname "$0")"
g++ -O1 -g -std=c++17 -I. -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wno-unused-function -Wno-unused-variable -o ${1:-/tmp/xor_planes_asan} zhemu.cpp xor_planes_main.cpp
