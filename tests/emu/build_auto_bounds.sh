#!/bin/sh
# AddressSanitizer + UBSan build of the per-source finder choice's bounds program (auto_bounds_main.cpp: its own main, nothing is loaded into python, no LD_PRELOAD):
#   sh tests/emu/build_auto_bounds.sh /tmp/auto_bounds && /tmp/auto_bounds SOURCE_FILE...
# tests/test_emu_auto_finder.py writes its sources to files and runs it.
set -e
cd "$(dirname "$0")"
g++ -O1 -g -std=c++17 -I. -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -w -o ${1:-/tmp/auto_bounds} zhemu.cpp emu_auto_finder.cpp auto_bounds_main.cpp
