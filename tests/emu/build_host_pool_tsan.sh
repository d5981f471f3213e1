#!/bin/sh
# ThreadSanitizer build of the pool and fan-out program (host_pool_tsan_main.cpp: its own main, nothing is loaded into python, no LD_PRELOAD):
#   sh tests/emu/build_host_pool_tsan.sh /tmp/host_pool_tsan && /tmp/host_pool_tsan
# tests/test_emu_host_calls.py builds and runs it.
set -e
cd "$(dirname "$0")"
g++ -O1 -g -std=c++17 -pthread -I. -fsanitize=thread -fno-omit-frame-pointer -Wall -o ${1:-/tmp/host_pool_tsan} host_pool_tsan_main.cpp
