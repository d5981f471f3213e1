// tests/emu/emu_decode_plan.cpp -- the launch plan of device decompress (python-zstandard_amd/csrc/zhip_decode_plan.hpp) behind a flat C entry.
// Test infrastructure only (tests/test_emu_decode_plan.py); part of libzhip_emu.so. The plan is plain host code: nothing is emulated here. The sizes of K2's and K1b's LDS, from
// which the library derives their workgroups per CU, come from emu_kernels.cpp, which compiles the pipeline header.
// With -DEMU_DECODE_PLAN_MAIN a stand-alone program (its own main; tests/emu/build_asan.sh builds it with -fsanitize=address,undefined): the cross product of the test's axes
// through both functions of the plan.
#include "../../python-zstandard_amd/csrc/zhip_decode_plan.hpp"
#include <stdio.h>
#include <string.h>

#define EMU_LDS_BYTES (160u * 1024u)      // per CU on gfx950 (ZHIP_LDS_BYTES, zhip_lib.hip)
extern "C" void emu_decode_lds_facts(uint64_t* out);      // sizeof(ZpSeqQLDS), sizeof(ZpHufKernelLDS), ZQ_FRAMES (emu_kernels.cpp)

// dict: 0 none, 1 content only, 2 with entropy tables; knob: k0Min, dchunk, nslot, k3PerCU; dev: numCU, decBlocksPerCU, k1PerCU, k3PerCU (K2's and K1b's workgroups per CU are the
// real ones, by LDS); sw: ZHIP_SIDE, ZHIP_K0, ZHIP_NSLOT.
static ZdPlanIn plan_in(uint64_t n, uint64_t sizeHint, uint64_t slotsHint, int hostPipe, int dict, int prof, const int64_t* knob, const int64_t* dev, const int64_t* sw)
{
    ZdPlanIn in;
    in.n = (size_t)n; in.hint.size = sizeHint; in.hint.slots = (size_t)slotsHint; in.hint.hostPipe = hostPipe != 0;
    in.dict.present = dict != 0; in.dict.hasEntropy = dict == 2; in.prof = prof != 0;
    in.knob.k0Min = (size_t)knob[0]; in.knob.dchunk = (size_t)knob[1]; in.knob.nslot = (int)knob[2]; in.knob.k3PerCU = (int)knob[3];
    in.dev.numCU = (int)dev[0]; in.dev.decBlocksPerCU = (int)dev[1]; in.dev.k1PerCU = (int)dev[2]; in.dev.k3PerCU = (int)dev[3];
    uint64_t lds[3]; emu_decode_lds_facts(lds);
    in.dev.k2LdsPerCU = EMU_LDS_BYTES / (size_t)lds[0]; in.dev.k1bLdsPerCU = EMU_LDS_BYTES / (size_t)lds[1]; in.dev.k2Frames = (size_t)lds[2];
    in.sideBuild = sw[0] != 0; in.k0Build = sw[1] != 0; in.nslotBuild = (int)sw[2];
    return in;
}
// out: the plan's fields in the order of tests/test_emu_decode_plan.py's FIELDS, then the first and the last chunk's. Returns the count written. Where the plan says "frame too
// large for the block arenas" the first field is 1 and the rest 0: the call fails before anything else is decided.
extern "C" int emu_decode_plan(uint64_t n, uint64_t sizeHint, uint64_t slotsHint, int hostPipe, int dict, int prof, const int64_t* knob, const int64_t* dev, const int64_t* sw, uint64_t* out)
{
    const ZdPlanIn in = plan_in(n, sizeHint, slotsHint, hostPipe, dict, prof, knob, dev, sw);
    const ZdPlan p = zd_decode_plan(in);
    uint64_t* w = out;
    const int total = 27 + 2 * 13;
    if (p.tooLarge) { memset(out, 0, total * sizeof *out); out[0] = 1; return total; }
    *w++ = 0; *w++ = p.mb; *w++ = p.side; *w++ = p.pre; *w++ = p.k1Lanes; *w++ = p.chunk; *w++ = p.slots; *w++ = p.nChunks; *w++ = (uint64_t)p.nslot; *w++ = p.arenaBudget16; *w++ = p.arenaBytes;
    *w++ = p.scratchBytes; *w++ = p.counterBytes; *w++ = p.basesBytes; *w++ = p.metaBytes; *w++ = p.litBytes; *w++ = p.countersBytes; *w++ = p.fallbackBytes; *w++ = p.fseBytes; *w++ = p.orderBytes;
    *w++ = p.hufBytes; *w++ = p.orderLitBytes; *w++ = p.preBytes; *w++ = p.itemFrameBytes; *w++ = p.itemRepsBytes; *w++ = p.frameRecsBytes; *w++ = p.genericGrid;
    const size_t cnts[2] = { in.n < p.chunk ? in.n : p.chunk, in.n - (in.n - 1) / p.chunk * p.chunk };
    for (size_t cnt : cnts) {
        const ZdChunkPlan k = zd_decode_chunk_plan(in, p, cnt);
        *w++ = k.itemCap; *w++ = k.items; *w++ = (uint64_t)k.k1; *w++ = (uint64_t)k.k2; *w++ = (uint64_t)k.k3;
        *w++ = k.gPre; *w++ = k.gLanes; *w++ = k.g1; *w++ = k.gBin; *w++ = k.gHuf; *w++ = k.g2; *w++ = k.g3; *w++ = k.gCheck;
    }
    return (int)(w - out);
}
// the host-buffer pipeline's hint for a chunk of `cnt` frames: out = size, slots, hostPipe
extern "C" void emu_decode_host_hint(const uint64_t* len, const uint32_t* nBlocks, uint64_t cnt, uint64_t* out)
{
    const ZdHints h = zd_host_hint(len, 1, nBlocks, (size_t)cnt);
    out[0] = h.size; out[1] = h.slots; out[2] = h.hostPipe;
}

#ifdef EMU_DECODE_PLAN_MAIN
// the axes of tests/test_emu_decode_plan.py (NS, HINTS, slot hints where the several-block mode reads them, KNOBS, DEVS)
int main()
{
    static const uint64_t ns[] = {1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 6143, 6144, 10922, 10923, 65535, 65536, 65537, 131073, 196608, 262145};
    static const uint64_t hints[] = {0, 1, 256, 4096, 16384, 16385, 131071, 131072, 131073, 262144, 262145, 1u << 20, 0x7FFFFFFFull, 0x80000000ull};
    static const int64_t knobs[][4] = {{6144, 65536, 2, 0}, {0, 65536, 2, 0}, {1000000000, 65536, 2, 0}, {6144, 32768, 2, 0}, {6144, 65536, 2, 24}};
    static const int64_t devs[][4] = {{256, 8, 8, 16}, {8, 8, 8, 16}};
    static const int64_t sw[3] = {ZHIP_SIDE, ZHIP_K0, ZHIP_NSLOT};
    uint64_t out[64], cases = 0, sum = 0, refused = 0;
    for (uint64_t n : ns) for (uint64_t hint : hints) {
        const bool mb = hint > ZF_BLOCK_MAX && hint <= 0x7FFFFFFFull;
        const uint64_t slotHints[] = {0, n, 2 * n + 2, 6 * n, n << 31};
        for (int s = 0; s < (mb ? 5 : 1); s++) for (int hostPipe = 0; hostPipe < 2; hostPipe++) for (int dict = 0; dict < 3; dict++) for (int prof = 0; prof < 2; prof++)
            for (const auto& knob : knobs) for (const auto& dev : devs) {
                const int cnt = emu_decode_plan(n, hint, slotHints[s], hostPipe, dict, prof, knob, dev, sw, out);
                for (int i = 0; i < cnt; i++) sum = sum * 1000003u + out[i];
                refused += out[0]; cases++;
            }
    }
    // the host pipeline's hint over a few batches: sizes around a block, block counts known and unknown
    for (uint64_t cnt = 1; cnt <= 64; cnt++) {
        uint64_t len[64]; uint32_t nb[64];
        for (uint64_t i = 0; i < cnt; i++) { len[i] = (i * 37 % 5) * 65537u + i; nb[i] = (uint32_t)(i % 17 == 0 ? 3 : i % 4); }
        emu_decode_host_hint(len, nb, cnt, out);
        sum = sum * 1000003u + out[0] + out[1];
    }
    printf("decode plan: %llu cases (%llu refused as too large), checksum %016llx\n", (unsigned long long)cases, (unsigned long long)refused, (unsigned long long)sum);
    return 0;
}
#endif
