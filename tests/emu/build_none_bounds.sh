#!/bin/sh
# AddressSanitizer + UBSan build of the literals-only kernel's bounds program (none_bounds_main.cpp: its own main, nothing is loaded into python, no LD_PRELOAD):
#   sh tests/emu/build_none_bounds.sh /tmp/none_bounds && /tmp/none_bounds SOURCE_FILE...
# tests/test_emu_none_finder.py writes the sources of tests/none_sources.py to files and runs it.
set -e
cd "$(dirname "$0")"
g++ -O1 -g -std=c++17 -I. -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -w -o ${1:-/tmp/none_bounds} zhemu.cpp emu_none_finder.cpp none_bounds_main.cpp
