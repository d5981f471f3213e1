#!/bin/sh
# AddressSanitizer + UBSan build of K1 -> K2 -> K3 of the decode pipeline under the host wave emulator, as a stand-alone PROGRAM (its own main in emu_k3_units.cpp;
# nothing is loaded into python, no LD_PRELOAD), in the form of build_asan.sh's other stand-alone programs. It decodes the frames of tests/k3units.py
# (python -m tests.k3units --write-fixture): K3's long-item units, the hand-off record's fields at their largest, the scalar-base addressing.
#   sh tests/emu/build_asan_k3_units.sh && /tmp/emu_k3_units_asan tests/golden/k3_units.bin
# (-fno-sanitize=shift-base: K2's ring offset shifts a negative position left, `(pos >> 5) << 2` in zp_seqq_body -- two's-complement arithmetic on the GPU and under g++,
# undefined before C++20; K2 runs in front of K3 here, and without the exception the program stops there)
set -e
cd "$(dirname "$0")"
g++ -O1 -g -std=c++17 -I. -fsanitize=address,undefined -fno-sanitize=shift-base -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wno-unused-function -Wno-unused-variable -DEMU_K3_UNITS_MAIN -o ${1:-/tmp/emu_k3_units_asan} zhemu.cpp emu_kernels.cpp emu_encode_plan.cpp emu_decode_plan.cpp emu_k3_units.cpp
