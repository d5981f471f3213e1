#!/bin/sh
# AddressSanitizer + UBSan build of one of the typed seekable kernels' stand-alone PROGRAMS under the host wave emulator -- typed_planes_main.cpp (split, join,
# seal), delta_planes_main.cpp, xor_planes_main.cpp, chain_planes_main.cpp: each has its own main; nothing is loaded into python, no
# LD_PRELOAD, in the form of build_asan.sh's other stand-alone programs.
#   sh tests/emu/build_asan_planes.sh typed_planes_main.cpp /tmp/typed_planes_asan && /tmp/typed_planes_asan
set -e
cd "$(dirname "$0")"
g++ -O1 -g -std=c++17 -I. -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wno-unused-function -Wno-unused-variable -o "$2" zhemu.cpp "$1"
