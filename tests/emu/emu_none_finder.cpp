// tests/emu/emu_none_finder.cpp -- the literals-only kernel (ze_none_body, ZHIP_FINDER_NONE) on the 64-fiber host emulator, with the trailer kernel behind it: whole
// frames. Test infrastructure only (tests/test_emu_none_finder.py, tests/emu/none_bounds_main.cpp); compiled with zhemu.cpp like emu_wave_finder.cpp.
#define ZHIP_EMU 1
#include <stdint.h>
extern "C" { long zd_trace_pos = -1; long zd_cur_frame = -1; long zd_stat[16]; }
#include "../../python-zstandard_amd/csrc/zhip_decode_pipeline.hpp"      // (zd_clock and friends: the encoder header relies on them, as in emu_kernels.cpp)
#include "../../python-zstandard_amd/csrc/zhip_encode_kernel.hpp"
#include "../../python-zstandard_amd/csrc/zhip_encode_none.hpp"
#include "../../python-zstandard_amd/csrc/zhip_cparams.hpp"
#include "../../python-zstandard_amd/csrc/zhip_encode_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static ZeLDS g_elds;
static ZeSeqLoad g_load;
static void none_lane(void* p) { ze_none_body(*(const ZhipEncodeArgs*)p, g_elds); }
static void load_lane(void* p) { ze_load_sequences_body(*(const ZhipEncodeArgs*)p, g_load); }
static void e2_lane(void* p) { ze_entropy_body(*(const ZhipEncodeArgs*)p, g_elds); }
static void ex_lane(void* p) { ze_trailer_body(*(const ZhipEncodeArgs*)p); }

// What zhip_compress_batch_device does under ZHIP_FINDER_NONE for a batch, in chunks of ze_none_plan's size (echunk: the ZHIP_ECHUNK knob, 0 = none): the literals-only
// kernel on nBlocks workgroups, then EX for checksummed frames. ZhipEncodeArgs.arena, .workspace and the table pointers are NULL (a load or store through one ends the
// program); the workspace pointer the kernel hands to ze_frame is the 64-byte idle pad below, from which ze_compress_block forms addresses it never dereferences.
// path 1: that. path 0: what zhip_compress_sequences_device does for the same sources with count 0 everywhere -- the loader, the entropy kernel, EX -- the second oracle.
// ov: the seven explicit fields (0 = unset) laid over `level`'s rows; flags: 1 content size, 2 checksum, 4 magicless format, 8 "the context has a dictionary".
// metaOut (may be null): n x (nbSeq, litSize, mode, pad). Returns 0, or 6 (ZHIP_ERR_UNSUPPORTED) where the product refuses the whole call.
extern "C" int emu_none_frames(const uint8_t* src, const uint64_t* srcSegs, uint32_t n, uint8_t* dst, const uint64_t* dstSegs, uint64_t* outSizes, int32_t* status,
                               int level, const int32_t* ov, uint32_t flags, uint32_t nBlocks, int path, uint32_t echunk, uint32_t* metaOut)
{
    ZhipEncodeArgs a; memset(&a, 0, sizeof(a));
    zhip_compression_parameters o; memset(&o, 0, sizeof o);
    o.windowLog = (uint32_t)ov[0]; o.chainLog = (uint32_t)ov[1]; o.hashLog = (uint32_t)ov[2]; o.searchLog = (uint32_t)ov[3]; o.minMatch = (uint32_t)ov[4]; o.targetLength = (uint32_t)ov[5]; o.strategy = ov[6];
    uint32_t counters[2] = {0, 0};
    a.src = src; a.srcSegs = srcSegs; a.dst = dst; a.dstSegs = dstSegs; a.outSizes = outSizes; a.status = status;
    a.counter = counters; a.n = n; a.level = level; zh_resolve_rows(&a.rows, level, &o);
    a.contentSizeFlag = flags & 1; a.checksumFlag = (flags >> 1) & 1; a.magicless = (flags >> 2) & 1; a.dictIDFlag = 1;
    if (path == 1 && ze_none_refusal(a.rows, (flags & 8) != 0)) return 6;      // the product's own predicate (zhip_encode_plan.hpp), as compress_batch_none asks it
    static uint8_t idlePad[64]; a.idle = idlePad;
    ZePlanIn in; in.rows = a.rows; in.n = n; in.knob.echunk = echunk; in.dev.numCU = 1; in.dev.e2PerCU = (int)nBlocks;
    size_t chunk = 0;
    std::vector<uint64_t> table;
    if (path == 1) { const ZeNonePlan s = ze_none_plan(in); chunk = s.chunk; a.meta = (ZeMeta*)malloc((s.metaBytes ? s.metaBytes : 1)); }
    else {
        const ZeSlotPlan s = ze_sequences_plan(in); chunk = s.chunk;
        a.arenaStride = s.arenaStride; a.arenaLit = s.arenaLit; a.slotSrcMax = s.slotSrcMax;
        a.meta = (ZeMeta*)malloc((chunk ? chunk : 1) * sizeof(ZeMeta)); a.arena = (uint8_t*)malloc((chunk ? chunk : 1) * (size_t)a.arenaStride);
        a.workspace = (uint8_t*)malloc((size_t)nBlocks * ZE_E2_STRIDE + ZHIP_ENC_STRIDE);
        table.assign(2 * (size_t)(n ? n : 1), 0); g_load.seqs = table.data(); g_load.table = table.data(); g_load.copyLits = 0;      // every list: first 0, count 0
    }
    memset(&g_elds, 0xA5, sizeof g_elds);
    for (size_t first = 0; first < n; first += chunk) {
        const size_t cnt = n - first < chunk ? n - first : chunk;
        a.first = (uint32_t)first; a.count = (uint32_t)cnt; counters[0] = counters[1] = 0;
        a.xxLater = a.checksumFlag ? 1u : 0u;
        if (path == 1) zhemu::run_grid(nBlocks, none_lane, &a);
        else { zhemu::run_grid((uint32_t)((cnt + 63) / 64), load_lane, &a); zhemu::run_grid(nBlocks, e2_lane, &a); }
        if (a.xxLater) zhemu::run_grid(nBlocks, ex_lane, &a);
        if (metaOut) memcpy(metaOut + 4 * first, a.meta, cnt * sizeof(ZeMeta));
    }
    free(a.meta); free(a.arena); free(a.workspace);
    return 0;
}

// zhip_compress_bound as the kernels compute it (ze_compress_bound): the exact size of a destination slot
extern "C" uint64_t emu_none_bound(uint64_t n) { return ze_compress_bound(n); }

// ze_none_plan's fields for a call of n sources on a device of numCU x e2PerCU resident entropy-kernel waves: out = {chunk, grid, metaBytes}
extern "C" void emu_none_plan(uint64_t n, int numCU, int e2PerCU, uint64_t echunk, uint64_t* out)
{
    ZePlanIn in; in.n = (size_t)n; in.knob.echunk = (size_t)echunk; in.dev.numCU = numCU; in.dev.e2PerCU = e2PerCU;
    const ZeNonePlan s = ze_none_plan(in);
    out[0] = s.chunk; out[1] = s.grid; out[2] = s.metaBytes;
}
