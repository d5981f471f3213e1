// tests/emu/emu_fast_flat.cpp -- the flat fast-strategy search (ze_fast_flat_np) and the lane-serial one it restates (ze_fast) side by side on the host.
// Test infrastructure only (tests/test_emu_fast_flat.py); compiled with zhemu.cpp like emu_kernels.cpp. Neither search has a cross-lane operation, so no wave is run.
#define ZHIP_EMU 1
#include <stdint.h>
extern "C" { long zd_trace_pos = -1; long zd_cur_frame = -1; long zd_stat[16]; }
#include "../../python-zstandard_amd/csrc/zhip_decode_pipeline.hpp"      // (zd_clock and friends: the encoder header relies on them, as in emu_kernels.cpp)
#include "../../python-zstandard_amd/csrc/zhip_encode_kernel.hpp"
#include <string.h>
#include <vector>

// the search under test on the caller's table (cells of earlier launches stay in it: `epoch` tells them apart). Returns the sequence count; seqs has room for n / 4 + 8.
extern "C" uint32_t emu_fast_flat(const uint8_t* src, uint32_t n, int hlog, int mml, uint32_t tlen, int pairs, uint32_t epoch, uint32_t* table, uint64_t* seqs)
{
    static uint8_t idlePad[64];
    if (pairs == 2) return ze_fast_flat_np<2>(seqs, src, n, hlog, mml, tlen, table, idlePad, epoch);
    return ze_fast_flat_np<1>(seqs, src, n, hlog, mml, tlen, table, idlePad, epoch);
}
// the lane-serial search, sequences only, on a zeroed table of its own
extern "C" uint32_t emu_fast_serial(const uint8_t* src, uint32_t n, int hlog, int mml, uint32_t tlen, uint64_t* seqs)
{
    std::vector<uint32_t> table((size_t)1 << hlog, 0u);
    ZePar cp; memset(&cp, 0, sizeof cp);
    cp.wlog = 17; cp.hlog = hlog; cp.mml = mml; cp.tlen = (int)tlen; cp.strat = 1;
    uint32_t lit = 0;
    return ze_fast(seqs, nullptr, &lit, src, n, cp, table.data());
}
