// tests/emu/exact_buffers.hpp -- what the stand-alone sanitizer programs of the typed seekable kernels share (typed_, delta_, xor_ and chain_planes_main.cpp,
// built by tests/emu/build_asan_planes.sh): the byte generator, whose seed each program sets first thing in its main, and buffers of exactly the bytes a kernel
// may touch. Test infrastructure only.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <memory>

static uint32_t g_seed;
static uint8_t next_byte() { g_seed = g_seed * 1664525u + 1013904223u; return (uint8_t)(g_seed >> 24); }
// `n` bytes at `offset` bytes into an allocation of exactly offset + n; fill 0: 0x5A, 1: random, 2: all bits set
struct Exact {
    std::unique_ptr<uint8_t[]> p; uint8_t* at;
    Exact(size_t n, size_t offset, int fill) : p(new uint8_t[n + offset]), at(p.get() + offset) { for (size_t i = 0; i < n; i++) at[i] = fill == 0 ? 0x5A : fill == 1 ? next_byte() : 0xFF; }
};
static int fail(const char* what, uint32_t k, uint64_t m, uint32_t off) { fprintf(stderr, "%s: k = %u, m = %llu, offset %u\n", what, k, (unsigned long long)m, off); return 1; }
