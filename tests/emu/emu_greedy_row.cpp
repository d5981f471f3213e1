// tests/emu/emu_greedy_row.cpp -- the greedy search with libzstd's row match finder (ze_greedy_row) on the host.
// Test infrastructure only (tests/test_emu_greedy_row.py); compiled with zhemu.cpp like emu_fast_flat.cpp. The search has no cross-lane operation, so no wave is run.
#define ZHIP_EMU 1
#include <stdint.h>
extern "C" { long zd_trace_pos = -1; long zd_cur_frame = -1; long zd_stat[16]; }
#include "../../python-zstandard_amd/csrc/zhip_decode_pipeline.hpp"      // (zd_clock and friends: the encoder header relies on them, as in emu_kernels.cpp)
#include "../../python-zstandard_amd/csrc/zhip_encode_kernel.hpp"
#include <string.h>
#include <vector>

// the search on zeroed tables of its own, with the parameters the device derives for a source of n bytes from one resolved row (ze_get_cparams).
// Returns the sequence count (seqs has room for n / 4 + 8), or -status when the row is refused for this source.
extern "C" int64_t emu_greedy_row(const uint8_t* src, uint32_t n, int wlog, int clog, int hlog, int slog, int mml, int tlen, int strat, uint64_t* seqs)
{
    ZeRows rows;
    for (int t = 0; t < 4; t++) { int32_t* r = rows.r[t]; r[0] = wlog; r[1] = clog; r[2] = hlog; r[3] = slog; r[4] = mml; r[5] = tlen; r[6] = strat; }
    ZePar cp; memset(&cp, 0, sizeof cp);
    const int e = ze_get_cparams<true>(cp, rows, n);
    if (e) return -(int64_t)e;
    if (cp.strat != 3) return -1000;
    std::vector<uint8_t> tables((size_t)5u << cp.hlog, 0);
    return ze_greedy_row(seqs, src, n, cp, (uint32_t*)tables.data(), tables.data() + ((size_t)4u << cp.hlog));
}

// ---- the greedy match kernel and the entropy kernel under emulation: whole frames (zhip_compress_batch_device's lane-serial form for a batch whose one-block row is greedy)
#include "../../python-zstandard_amd/csrc/zhip_cparams.hpp"
#include "../../python-zstandard_amd/csrc/zhip_encode_plan.hpp"
#include <stdlib.h>
static ZeLDS g_elds;
static void e1g_lane(void* p) { ze_match_body<true>(*(const ZhipEncodeArgs*)p); }
static void e2_lane(void* p) { ze_entropy_body(*(const ZhipEncodeArgs*)p, g_elds); }
static void ex_lane(void* p) { ze_trailer_body(*(const ZhipEncodeArgs*)p); }
// ov: the seven explicit fields (0 = unset) laid over `level`'s rows; flags: 1 content size, 2 checksum. Sources above one block are refused here (status 40) as the generic kernel does.
extern "C" int emu_greedy_frames(const uint8_t* src, const uint64_t* srcSegs, uint32_t n, uint8_t* dst, const uint64_t* dstSegs, uint64_t* outSizes, int32_t* status,
                                 int level, const int32_t* ov, uint32_t flags, uint32_t nBlocks)
{
    ZhipEncodeArgs a; memset(&a, 0, sizeof(a));
    zhip_compression_parameters o; memset(&o, 0, sizeof o);
    o.windowLog = (uint32_t)ov[0]; o.chainLog = (uint32_t)ov[1]; o.hashLog = (uint32_t)ov[2]; o.searchLog = (uint32_t)ov[3]; o.minMatch = (uint32_t)ov[4]; o.targetLength = (uint32_t)ov[5]; o.strategy = ov[6];
    uint32_t counters[2] = {0, 0}, bigCount = 0;
    a.src = src; a.srcSegs = srcSegs; a.dst = dst; a.dstSegs = dstSegs; a.outSizes = outSizes; a.status = status;
    a.counter = counters; a.n = n; a.level = level; zh_resolve_rows(&a.rows, level, &o);
    a.contentSizeFlag = flags & 1; a.checksumFlag = (flags >> 1) & 1; a.dictIDFlag = 1;
    a.workspace = (uint8_t*)malloc((size_t)nBlocks * ZE_E2_STRIDE + ZHIP_ENC_STRIDE);
    {   ZePlanIn in; in.rows = a.rows; in.n = n; const ZePlan p = ze_encode_plan(in); a.tableStride = p.tableStride; a.e1Lanes = p.e1Lanes; }      // the product's plan: the row tables' bytes per lane
    a.laneTables = (uint8_t*)malloc((size_t)nBlocks * a.e1Lanes * a.tableStride); memset(a.laneTables, 0xA5, (size_t)nBlocks * a.e1Lanes * a.tableStride);
    a.meta = (ZeMeta*)calloc(n ? n : 1, sizeof(ZeMeta));
    a.arena = (uint8_t*)malloc((size_t)(n ? n : 1) * ZE_ARENA_STRIDE); a.arenaStride = (uint32_t)ZE_ARENA_STRIDE; a.arenaLit = ZE_ARENA_LIT;
    a.bigList = (uint32_t*)calloc(n ? n : 1, 4); a.bigCount = &bigCount;
    static uint8_t idlePad[64]; a.idle = idlePad;
    a.first = 0; a.count = n;
    memset(&g_elds, 0xA5, sizeof g_elds);
    zhemu::run_grid(nBlocks, e1g_lane, &a);
    a.xxLater = a.checksumFlag ? 1u : 0u;
    zhemu::run_grid(nBlocks, e2_lane, &a);
    if (a.xxLater) zhemu::run_grid(nBlocks, ex_lane, &a);
    for (uint32_t k = 0; k < bigCount; k++) { status[a.bigList[k]] = ZE_PARAM_UNSUPPORTED; outSizes[a.bigList[k]] = 0; }
    free(a.workspace); free(a.laneTables); free(a.meta); free(a.arena); free(a.bigList);
    return 0;
}
