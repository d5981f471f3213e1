#!/bin/sh
# AddressSanitizer build of the emulated kernels (debug aid): out-of-bounds reads / writes of the kernel sources show up on the host.
#   sh tests/emu/build_asan.sh && LD_PRELOAD=$(gcc -print-file-name=libasan.so) ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0 \
#       ZHIP_EMU_SO=/tmp/libzhip_emu_asan.so python tests/stress_emu_encode.py 1 p 3
set -e
cd "$(dirname "$0")"
g++ -O1 -g -fPIC -shared -std=c++17 -I. -fsanitize=address -fno-omit-frame-pointer -Wno-unused-function -Wno-unused-variable -o ${1:-/tmp/libzhip_emu_asan.so} zhemu.cpp emu_kernels.cpp emu_encode_plan.cpp emu_decode_plan.cpp
# the same for the entropy kernel driven by explicit sequences, as a stand-alone PROGRAM (its own main; nothing is loaded into python, no LD_PRELOAD):
#   /tmp/emu_entropy_sequences_asan tests/golden/entropy_sequences.bin
g++ -O1 -g -std=c++17 -I. -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wno-unused-function -Wno-unused-variable -DEMU_ENTROPY_SEQUENCES_MAIN -o ${2:-/tmp/emu_entropy_sequences_asan} zhemu.cpp emu_entropy_sequences.cpp
# and for the double-fast searches over the aimed sources (tests/dfast_sources.py, python -m tests.dfast_sources --write-fixture), again a stand-alone program:
#   /tmp/emu_dfast_asan tests/golden/dfast_sources.bin
g++ -O1 -g -std=c++17 -I. -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -fno-omit-frame-pointer -Wno-unused-function -Wno-unused-variable -DEMU_DFAST_MAIN -o ${3:-/tmp/emu_dfast_asan} zhemu.cpp emu_dfast.cpp
# and for the launch plan of device decompress (zhip_decode_plan.hpp: double -> size_t conversions, 32-bit narrowings) over the cross product of tests/test_emu_decode_plan.py's
# axes, a stand-alone program too (emu_kernels.cpp is linked for the sizes of the kernels' LDS):
#   /tmp/emu_decode_plan_asan
g++ -O1 -g -std=c++17 -I. -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wno-unused-function -Wno-unused-variable -DEMU_DECODE_PLAN_MAIN -o ${4:-/tmp/emu_decode_plan_asan} zhemu.cpp emu_kernels.cpp emu_decode_plan.cpp
