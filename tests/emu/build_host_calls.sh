#!/bin/sh
# AddressSanitizer + UBSan build of the host-buffer calls' plan program (host_calls_main.cpp: its own main, nothing is loaded into python, no LD_PRELOAD):
#   sh tests/emu/build_host_calls.sh /tmp/host_calls && /tmp/host_calls
# tests/test_emu_host_calls.py builds and runs it.
set -e
cd "$(dirname "$0")"
g++ -O1 -g -std=c++17 -pthread -I. -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall -o ${1:-/tmp/host_calls} host_calls_main.cpp
