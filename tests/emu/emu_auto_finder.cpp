// tests/emu/emu_auto_finder.cpp -- the match finder chosen per source (ZHIP_FINDER_AUTO, zhip_encode_auto.hpp) on the 64-fiber host emulator: the classify kernel, the
// partition / gather / scatter kernels of the split, and behind them the two existing paths -- the literals-only kernel (ze_none_body) and the default finder's kernels
// (here: the lane-serial match kernel, the entropy kernel, and the generic kernel for sources of several blocks; the flat searches in front of them write the same
// frames and have their own emulator tests) -- each with the trailer kernel. Test infrastructure only (tests/test_emu_auto_finder.py, tests/emu/auto_bounds_main.cpp);
// compiled with zhemu.cpp like emu_none_finder.cpp.
#define ZHIP_EMU 1
#include <stdint.h>
extern "C" { long zd_trace_pos = -1; long zd_cur_frame = -1; long zd_stat[16]; }
#include "../../python-zstandard_amd/csrc/zhip_decode_pipeline.hpp"      // (zd_clock and friends: the encoder header relies on them, as in emu_kernels.cpp)
#include "../../python-zstandard_amd/csrc/zhip_encode_kernel.hpp"
#include "zhip_device_emu_wave.hpp"
#include "../../python-zstandard_amd/csrc/zhip_encode_none.hpp"
#include "../../python-zstandard_amd/csrc/zhip_cparams.hpp"
#include "../../python-zstandard_amd/csrc/zhip_encode_plan.hpp"
#include "../../python-zstandard_amd/csrc/zhip_encode_auto.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static ZeLDS g_elds;
static ZeLDSMulti g_eldsm;
static ZaLDS g_alds;
static void classify_lane(void* p) { ze_classify_body(*(const ZhipClassifyArgs*)p, g_alds); }
static void partition_lane(void* p) { ze_auto_partition_body(*(const ZhipSplitArgs*)p); }
static void gather_lane(void* p) { ze_auto_gather_body(*(const ZhipSplitArgs*)p); }
static void scatter_lane(void* p) { ze_auto_scatter_body(*(const ZhipSplitArgs*)p); }
static void none_lane(void* p) { ze_none_body(*(const ZhipEncodeArgs*)p, g_elds); }
static void e1_lane(void* p) { ze_match_body(*(const ZhipEncodeArgs*)p); }
static void e2_lane(void* p) { ze_entropy_body(*(const ZhipEncodeArgs*)p, g_elds); }
static void ex_lane(void* p) { ze_trailer_body(*(const ZhipEncodeArgs*)p); }
static void enc_lane(void* p) { ze_kernel_body(*(const ZhipEncodeArgs*)p, g_elds, g_eldsm); }

// the classify kernel over a batch in launches of `chunk` sources on nBlocks workgroups (the LDS is poisoned before every launch: the kernel clears what it reads)
extern "C" void emu_auto_classify(const uint8_t* src, const uint64_t* srcSegs, uint32_t n, uint8_t* choice, uint32_t* stats, uint32_t nBlocks, uint32_t chunk)
{
    uint32_t counter = 0;
    ZhipClassifyArgs k; k.src = src; k.srcSegs = srcSegs; k.choice = choice; k.stats = stats; k.counter = &counter;
    if (!chunk) chunk = n ? n : 1;
    for (uint32_t first = 0; first < n; first += chunk) {
        k.first = first; k.count = n - first < chunk ? n - first : chunk; counter = 0;
        memset(&g_alds, 0xA5, sizeof g_alds);
        zhemu::run_grid(nBlocks, classify_lane, &k);
    }
}

// ZHIP_FINDER_NONE's path over a batch, as compress_batch_none runs it (emu_none_finder.cpp's path 1); returns launches of the literals-only kernel
static uint32_t run_none(ZhipEncodeArgs a, uint32_t n, uint32_t nBlocks, uint32_t echunk)
{
    uint32_t counters[2] = {0, 0}, launches = 0;
    ZePlanIn in; in.rows = a.rows; in.n = n; in.knob.echunk = echunk; in.dev.numCU = 1; in.dev.e2PerCU = (int)nBlocks;
    const ZeNonePlan s = ze_none_plan(in);
    a.counter = counters; a.n = n; a.meta = (ZeMeta*)malloc(s.metaBytes ? s.metaBytes : 1); a.workspace = nullptr;
    for (size_t first = 0; first < n; first += s.chunk) {
        a.first = (uint32_t)first; a.count = (uint32_t)(n - first < s.chunk ? n - first : s.chunk); counters[0] = counters[1] = 0;
        a.xxLater = a.checksumFlag ? 1u : 0u;
        zhemu::run_grid(nBlocks, none_lane, &a); launches++;
        if (a.xxLater) zhemu::run_grid(nBlocks, ex_lane, &a);
    }
    free(a.meta);
    return launches;
}
// the default finder's path over a batch, one chunk: the lane-serial match kernel, the entropy kernel, the trailer kernel, then the generic kernel over the list of
// sources of several blocks; returns launches of the match kernel
static uint32_t run_search(ZhipEncodeArgs a, uint32_t n, uint32_t nBlocks)
{
    uint32_t counters[2] = {0, 0}, bigCount = 0;
    a.counter = counters; a.n = n;
    a.workspace = (uint8_t*)malloc((size_t)nBlocks * ZE_E2_STRIDE + ZHIP_ENC_STRIDE);
    a.meta = (ZeMeta*)calloc(n, sizeof(ZeMeta));
    ZePlanIn in; in.rows = a.rows; in.n = n;
    const ZePlan p = ze_encode_plan(in);
    a.arenaLit = ZE_ARENA_LIT; a.arenaStride = (uint32_t)ZE_ARENA_STRIDE;              // (the lane-serial kernel's slots keep their literal area, as in emu_wave_finder.cpp)
    a.arena = (uint8_t*)malloc((size_t)n * a.arenaStride);
    a.bigList = (uint32_t*)calloc(n, 4); a.bigCount = &bigCount;
    a.tableStride = p.tableStride; a.e1Lanes = p.e1Lanes;
    a.laneTables = (uint8_t*)malloc((size_t)nBlocks * a.e1Lanes * a.tableStride); memset(a.laneTables, 0xA5, (size_t)nBlocks * a.e1Lanes * a.tableStride);
    a.first = 0; a.count = n;
    zhemu::run_grid(nBlocks, e1_lane, &a);
    a.xxLater = a.checksumFlag ? 1u : 0u;
    zhemu::run_grid(nBlocks, e2_lane, &a);
    if (a.xxLater) zhemu::run_grid(nBlocks, ex_lane, &a);
    a.xxLater = 0;
    if (bigCount) {
        ZhipEncodeArgs b = a; uint32_t bc = 0;
        b.workspace = (uint8_t*)malloc((size_t)nBlocks * ZHIP_ENC_STRIDE); b.counter = &bc; b.frameList = a.bigList; b.listCount = &bigCount;
        zhemu::run_grid(nBlocks, enc_lane, &b);
        free(b.workspace);
    }
    free(a.workspace); free(a.meta); free(a.arena); free(a.bigList); free(a.laneTables);
    return 1;
}

// What zhip_compress_batch_device does for a batch without dictionary under finder 0 (the default), 2 (ZHIP_FINDER_NONE) or 4 (ZHIP_FINDER_AUTO: classify, partition,
// gather, the two parts through the two paths above on the gathered tables, scatter). ov: the seven explicit fields (0 = unset) laid over `level`'s rows; flags: 1 content
// size, 2 checksum, 8 "the context has a dictionary". Under finder 4: choiceOut (may be null) n choice bytes, statsOut (may be null) 4 n words -- from a second run of the
// classifier, which must not change the choice --, launches[0 .. 2] = launches of the match kernel, the literals-only kernel and the classify kernel.
// Returns 0, or 6 (ZHIP_ERR_UNSUPPORTED) where the product refuses the whole call.
extern "C" int emu_auto_frames(const uint8_t* src, const uint64_t* srcSegs, uint32_t n, uint8_t* dst, const uint64_t* dstSegs, uint64_t* outSizes, int32_t* status,
                               int level, const int32_t* ov, uint32_t flags, uint32_t nBlocks, uint32_t echunk, int finder, uint8_t* choiceOut, uint32_t* statsOut, uint32_t* launches)
{
    ZhipEncodeArgs a; memset(&a, 0, sizeof(a));
    zhip_compression_parameters o; memset(&o, 0, sizeof o);
    o.windowLog = (uint32_t)ov[0]; o.chainLog = (uint32_t)ov[1]; o.hashLog = (uint32_t)ov[2]; o.searchLog = (uint32_t)ov[3]; o.minMatch = (uint32_t)ov[4]; o.targetLength = (uint32_t)ov[5]; o.strategy = ov[6];
    a.src = src; a.srcSegs = srcSegs; a.dst = dst; a.dstSegs = dstSegs; a.outSizes = outSizes; a.status = status;
    a.level = level; zh_resolve_rows(&a.rows, level, &o);
    a.contentSizeFlag = flags & 1; a.checksumFlag = (flags >> 1) & 1; a.dictIDFlag = 1;
    static uint8_t idlePad[64]; a.idle = idlePad;
    memset(&g_elds, 0xA5, sizeof g_elds);
    uint32_t l3[3] = {0, 0, 0};
    if (finder == 2) { if (ze_none_refusal(a.rows, (flags & 8) != 0)) return 6; l3[1] = run_none(a, n, nBlocks, echunk); }
    else if (finder == 0) { if (n) l3[0] = run_search(a, n, nBlocks); }
    else {
        if (ze_auto_refusal(a.rows, (flags & 8) != 0)) return 6;
        ZePlanIn in; in.rows = a.rows; in.n = n; in.knob.echunk = echunk; in.dev.numCU = 1;
        const ZeAutoPlan s = ze_auto_plan(in, (int)nBlocks);
        std::vector<uint8_t> scratch(s.bytes + 16, 0xA5);                               // the context's encAuto buffer, laid out by the plan
        uint8_t* const base = scratch.data();
        emu_auto_classify(src, srcSegs, n, base + s.offChoice, nullptr, s.grid ? s.grid : 1, (uint32_t)s.chunk);
        l3[2] = (uint32_t)((n + s.chunk - 1) / (s.chunk ? s.chunk : 1));
        ZhipSplitArgs k; memset(&k, 0, sizeof k);
        k.choice = base + s.offChoice; k.n = n; k.perm = (uint32_t*)(base + s.offPerm); k.counts = (uint32_t*)(base + 4);
        k.srcSegs = srcSegs; k.dstSegs = dstSegs; k.gSrcSegs = (uint64_t*)(base + s.offSrcSegs); k.gDstSegs = (uint64_t*)(base + s.offDstSegs);
        k.outSizes = outSizes; k.status = status; k.gOutSizes = (const uint64_t*)(base + s.offOutSizes); k.gStatus = (const int32_t*)(base + s.offStatus);
        zhemu::run_grid(1, partition_lane, &k);
        zhemu::run_grid(s.gridMove ? s.gridMove : 1, gather_lane, &k);
        const uint32_t n0 = k.counts[0], n1 = k.counts[1];
        if (n0 + n1 != n) return 1;
        ZhipEncodeArgs b = a;
        b.srcSegs = k.gSrcSegs; b.dstSegs = k.gDstSegs; b.outSizes = (uint64_t*)k.gOutSizes; b.status = (int32_t*)k.gStatus;
        if (n0) l3[0] = run_search(b, n0, nBlocks);
        b.srcSegs = k.gSrcSegs + 2 * (size_t)n0; b.dstSegs = k.gDstSegs + 2 * (size_t)n0; b.outSizes = (uint64_t*)k.gOutSizes + n0; b.status = (int32_t*)k.gStatus + n0;
        if (n1) l3[1] = run_none(b, n1, nBlocks, echunk);
        zhemu::run_grid(s.gridMove ? s.gridMove : 1, scatter_lane, &k);
        if (choiceOut) memcpy(choiceOut, base + s.offChoice, n);
        if (statsOut) { std::vector<uint8_t> again(n ? n : 1); emu_auto_classify(src, srcSegs, n, again.data(), statsOut, 2, 0); if (memcmp(again.data(), base + s.offChoice, n)) return 2; }
    }
    if (launches) memcpy(launches, l3, sizeof l3);
    return 0;
}

// zhip_compress_bound as the kernels compute it (ze_compress_bound): the exact size of a destination slot
extern "C" uint64_t emu_auto_bound(uint64_t n) { return ze_compress_bound(n); }

// ze_auto_plan's fields for a call of n sources on numCU x perCU resident classify waves: out = {chunk, grid, gridMove, bytes}
extern "C" void emu_auto_plan(uint64_t n, int numCU, int perCU, uint64_t echunk, uint64_t* out)
{
    ZePlanIn in; in.n = (size_t)n; in.knob.echunk = (size_t)echunk; in.dev.numCU = numCU;
    const ZeAutoPlan s = ze_auto_plan(in, perCU);
    out[0] = s.chunk; out[1] = s.grid; out[2] = s.gridMove; out[3] = s.bytes;
}
