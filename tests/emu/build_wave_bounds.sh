#!/bin/sh
# AddressSanitizer + UBSan build of the wave-parallel match finder's bounds program (wave_bounds_main.cpp: its own main, nothing is loaded into python, no LD_PRELOAD):
#   sh tests/emu/build_wave_bounds.sh /tmp/wave_bounds && /tmp/wave_bounds SOURCE_FILE...
# tests/test_emu_wave_finder.py writes the sources of tests/wave_sources.py to files and runs it.
set -e
cd "$(dirname "$0")"
g++ -O1 -g -std=c++17 -I. -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -w -o ${1:-/tmp/wave_bounds} zhemu.cpp emu_wave_finder.cpp wave_bounds_main.cpp
