// tests/emu/emu_wave_finder.cpp -- the wave-parallel match finder (ze_match_wave_body, ZHIP_FINDER_WAVE) on the 64-fiber host emulator, with the entropy kernel and the
// trailer kernel behind it: whole frames, and the sequence lists the match kernel left. Test infrastructure only (tests/test_emu_wave_finder.py, tests/emu/wave_bounds_main.cpp);
// compiled with zhemu.cpp like emu_greedy_row.cpp.
#define ZHIP_EMU 1
#include <stdint.h>
extern "C" { long zd_trace_pos = -1; long zd_cur_frame = -1; long zd_stat[16]; }
#include "../../python-zstandard_amd/csrc/zhip_decode_pipeline.hpp"      // (zd_clock and friends: the encoder header relies on them, as in emu_kernels.cpp)
#include "../../python-zstandard_amd/csrc/zhip_encode_kernel.hpp"
#include "zhip_device_emu_wave.hpp"
#include "../../python-zstandard_amd/csrc/zhip_encode_wave.hpp"
#include "../../python-zstandard_amd/csrc/zhip_cparams.hpp"
#include "../../python-zstandard_amd/csrc/zhip_encode_plan.hpp"
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static ZeLDS g_elds;
static uint32_t g_table[1u << 14];              // the match kernel's LDS table (one workgroup runs at a time)
static int g_H = 12;
static void wave_lane(void* p)
{
    const ZhipEncodeArgs& a = *(const ZhipEncodeArgs*)p;
    if (g_H == 13) ze_match_wave_body<13>(a, g_table); else if (g_H == 14) ze_match_wave_body<14>(a, g_table); else ze_match_wave_body<12>(a, g_table);
}
static void e1_lane(void* p) { ze_match_body(*(const ZhipEncodeArgs*)p); }
static void e2_lane(void* p) { ze_entropy_body(*(const ZhipEncodeArgs*)p, g_elds); }
static void ex_lane(void* p) { ze_trailer_body(*(const ZhipEncodeArgs*)p); }

// What zhip_compress_batch_device does for a batch without dictionary, one chunk: finder 1 = the wave match kernel (H: log2 of its table cells), finder 0 = the default
// dispatch's lane-serial match kernel; then E2 and EX. ov: the seven explicit fields (0 = unset) laid over `level`'s rows; flags: 1 content size, 2 checksum.
// seqOut (may be null): seqStride packed sequences per source, what the match kernel left in the arena; metaOut (may be null): n x (nbSeq, litSize, mode, pad).
// Returns 0, or 6 (ZHIP_ERR_UNSUPPORTED) where the product refuses the whole call under the wave finder.
extern "C" int emu_wave_frames(const uint8_t* src, const uint64_t* srcSegs, uint32_t n, uint8_t* dst, const uint64_t* dstSegs, uint64_t* outSizes, int32_t* status,
                               int level, const int32_t* ov, uint32_t flags, uint32_t nBlocks, int finder, int H, uint64_t* seqOut, uint32_t seqStride, uint32_t* metaOut)
{
    ZhipEncodeArgs a; memset(&a, 0, sizeof(a));
    zhip_compression_parameters o; memset(&o, 0, sizeof o);
    o.windowLog = (uint32_t)ov[0]; o.chainLog = (uint32_t)ov[1]; o.hashLog = (uint32_t)ov[2]; o.searchLog = (uint32_t)ov[3]; o.minMatch = (uint32_t)ov[4]; o.targetLength = (uint32_t)ov[5]; o.strategy = ov[6];
    uint32_t counters[2] = {0, 0}, bigCount = 0;
    a.src = src; a.srcSegs = srcSegs; a.dst = dst; a.dstSegs = dstSegs; a.outSizes = outSizes; a.status = status;
    a.counter = counters; a.n = n; a.level = level; zh_resolve_rows(&a.rows, level, &o);
    a.contentSizeFlag = flags & 1; a.checksumFlag = (flags >> 1) & 1; a.dictIDFlag = 1;
    if (finder == 1 && a.rows.r[2][6] != 1 && a.rows.r[2][6] != 2) return 6;
    if (H < 12 || H > 14) return 6;
    g_H = H;
    a.workspace = (uint8_t*)malloc((size_t)nBlocks * ZE_E2_STRIDE + ZHIP_ENC_STRIDE);
    a.meta = (ZeMeta*)calloc(n ? n : 1, sizeof(ZeMeta));
    ZePlanIn in; in.rows = a.rows; in.n = n;
    // the product's plans. (On purpose not the product's: under the default finder only the lane-serial match kernel runs here, so its slots keep the literal area the flat
    // kernel's batches do without.)
    a.arenaLit = ZE_ARENA_LIT; a.arenaStride = finder == 1 ? ze_wave_plan(in).arenaStride : (uint32_t)ZE_ARENA_STRIDE;
    a.arena = (uint8_t*)malloc((size_t)(n ? n : 1) * a.arenaStride);
    a.bigList = (uint32_t*)calloc(n ? n : 1, 4); a.bigCount = &bigCount;
    static uint8_t idlePad[64]; a.idle = idlePad;
    a.first = 0; a.count = n;
    memset(&g_elds, 0xA5, sizeof g_elds);
    if (finder == 1) {
        memset(g_table, 0xA5, sizeof g_table);
        zhemu::run_grid(nBlocks, wave_lane, &a);
        for (uint32_t i = 0; i < n; i++) {
            // every sequence covers minMatch >= 4 bytes of a source of one block: the count cannot reach the slot's capacity
            if (a.meta[i].mode == 4) assert(a.meta[i].nbSeq <= ZE_SEQ_CAP && (uint64_t)a.meta[i].nbSeq * 4 <= srcSegs[2 * (size_t)i + 1]);
        }
    } else {
        const ZePlan p = ze_encode_plan(in);
        a.tableStride = p.tableStride; a.e1Lanes = p.e1Lanes;
        a.laneTables = (uint8_t*)malloc((size_t)nBlocks * a.e1Lanes * a.tableStride); memset(a.laneTables, 0xA5, (size_t)nBlocks * a.e1Lanes * a.tableStride);
        zhemu::run_grid(nBlocks, e1_lane, &a);
    }
    for (uint32_t i = 0; i < n; i++) {
        if (metaOut) memcpy(metaOut + 4 * (size_t)i, &a.meta[i], 16);
        if (seqOut && (a.meta[i].mode == 4 || a.meta[i].mode == 0)) {
            const uint32_t k = a.meta[i].nbSeq < seqStride ? a.meta[i].nbSeq : seqStride;
            memcpy(seqOut + (size_t)i * seqStride, a.arena + (size_t)i * a.arenaStride + ZE_ARENA_SEQ, 8 * (size_t)k);
        }
    }
    a.xxLater = a.checksumFlag ? 1u : 0u;
    zhemu::run_grid(nBlocks, e2_lane, &a);
    if (a.xxLater) zhemu::run_grid(nBlocks, ex_lane, &a);
    for (uint32_t k = 0; k < bigCount; k++) { status[a.bigList[k]] = ZE_PARAM_UNSUPPORTED; outSizes[a.bigList[k]] = 0; }      // (default finder: the generic kernel's sources; not emulated here)
    free(a.workspace); free(a.laneTables); free(a.meta); free(a.arena); free(a.bigList);
    return 0;
}
