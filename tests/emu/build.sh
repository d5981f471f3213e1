#!/bin/sh
# builds tests/emu/libzhip_emu.so : product kernel sources compiled for the host wave emulator (debug aid), and the launch plan behind a flat entry (emu_encode_plan.cpp)
set -e
cd "$(dirname "$0")"
g++ -O1 -g -fPIC -shared -std=c++17 -I. -Wall -Wno-unused-function -Wno-unused-variable -o libzhip_emu.so zhemu.cpp emu_kernels.cpp emu_encode_plan.cpp emu_decode_plan.cpp emu_host_calls.cpp
# tests/emu/libzhip_emu_entropy_sequences.so : the loader, the entropy kernel and the trailer kernel driven by explicit sequences (a library of its own: the kernel headers define their functions)
g++ -O1 -g -fPIC -shared -std=c++17 -I. -Wall -Wno-unused-function -Wno-unused-variable -o libzhip_emu_entropy_sequences.so zhemu.cpp emu_entropy_sequences.cpp
