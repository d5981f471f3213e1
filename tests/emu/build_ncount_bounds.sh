#!/bin/sh
# AddressSanitizer + UBSan build of the FSE distribution parser's bounds program (ncount_bounds_main.cpp: its own main, nothing is loaded into python, no LD_PRELOAD):
#   sh tests/emu/build_ncount_bounds.sh /tmp/ncount_bounds && /tmp/ncount_bounds tests/golden/fse_descriptions.bin
# tests/test_emu_sequence_tables.py builds and runs it over the fixture python -m tests.fsefamilies --write-fixture writes.
set -e
cd "$(dirname "$0")"
g++ -O1 -g -std=c++17 -I. -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -w -o ${1:-/tmp/ncount_bounds} zhemu.cpp ncount_bounds_main.cpp
