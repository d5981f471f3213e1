#!/bin/sh
# AddressSanitizer + UBSan build of the typed seekable kernels (split, join, seal) under the host wave emulator, as a stand-alone PROGRAM (its own main in
# typed_planes_main.cpp; nothing is loaded into python, no LD_PRELOAD), in the form of build_asan.sh's other stand-alone programs.
#   sh tests/emu/build_asan_typed.sh && /tmp/typed_planes_asan
set -e
cd "$(dirname "$0")"
g++ -O1 -g -std=c++17 -I. -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wno-unused-function -Wno-unused-variable -o ${1:-/tmp/typed_planes_asan} zhemu.cpp typed_planes_main.cpp
