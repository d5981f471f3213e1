// tests/emu/emu_encode_plan.cpp -- the launch plan of device compress (python-zstandard_amd/csrc/zhip_encode_plan.hpp) behind a flat C entry.
// Test infrastructure only (tests/test_emu_encode_plan.py); part of libzhip_emu.so. The plan is plain host code: nothing is emulated here.
#include "../../python-zstandard_amd/csrc/zhip_encode_plan.hpp"
#include <string.h>

// level + ov: the seven explicit fields (0 = unset) laid over the level's rows; dict: present, hlog, clog, strat, attachMax, contentSize; dev: numCU, encBlocksPerCU, e1PerCU,
// e2PerCU; knob: echunk, echunkMax, mbcMin, mbcLanes, flat4Max, flat3Max, flat3, fast2Max, fastPairs, e1LdsMax, e1LdsRounds; sw: fastWide, tableEpochs, e1LdsPerCU.
// out: the plan's fields in the order of tests/test_emu_encode_plan.py's FIELDS, then the match stage of the first and of the last chunk. Returns the count written.
extern "C" int emu_encode_plan(int level, const int32_t* ov, uint64_t n, uint64_t sizeHint, uint64_t srcMaxHint, const int64_t* dict, const int64_t* dev, const int64_t* knob,
                               const int64_t* sw, uint64_t flatMax, uint64_t* out)
{
    zhip_compression_parameters o; memset(&o, 0, sizeof o);
    o.windowLog = (uint32_t)ov[0]; o.chainLog = (uint32_t)ov[1]; o.hashLog = (uint32_t)ov[2]; o.searchLog = (uint32_t)ov[3]; o.minMatch = (uint32_t)ov[4]; o.targetLength = (uint32_t)ov[5]; o.strategy = ov[6];
    ZePlanIn in;
    zh_resolve_rows(&in.rows, level, &o);
    in.n = (size_t)n; in.sizeHint = (size_t)sizeHint; in.srcMaxHint = (size_t)srcMaxHint; in.flatMax = (size_t)flatMax;
    in.dict.present = dict[0] != 0; in.dict.hlog = (int)dict[1]; in.dict.clog = (int)dict[2]; in.dict.strat = (int)dict[3]; in.dict.attachMax = (uint32_t)dict[4]; in.dict.contentSize = (uint32_t)dict[5];
    in.dev.numCU = (int)dev[0]; in.dev.encBlocksPerCU = (int)dev[1]; in.dev.e1PerCU = (int)dev[2]; in.dev.e2PerCU = (int)dev[3];
    ZeEncodeKnobs& k = in.knob;
    k.echunk = (size_t)knob[0]; k.echunkMax = (size_t)knob[1]; k.mbcMin = (size_t)knob[2]; k.mbcLanes = (unsigned)knob[3]; k.flat4Max = (size_t)knob[4]; k.flat3Max = (size_t)knob[5];
    k.flat3 = knob[6] != 0; k.fast2Max = (size_t)knob[7]; k.fastPairs = (int)knob[8]; k.e1LdsMax = (long)knob[9]; k.e1LdsRounds = (size_t)knob[10];
    in.fastWide = sw[0] != 0; in.tableEpochs = sw[1] != 0; in.e1LdsPerCU = (size_t)sw[2];
    const ZePlan p = ze_encode_plan(in);
    uint64_t* w = out;
    *w++ = p.greedy; *w++ = p.anyDfast; *w++ = p.mbcWanted; *w++ = p.flatDict; *w++ = p.flatFast; *w++ = p.flat; *w++ = p.allDfast; *w++ = p.fastWide; *w++ = p.mbc;
    *w++ = p.tableStride; *w++ = p.arenaStride; *w++ = p.arenaLit; *w++ = p.slotSrcMax; *w++ = p.e1Lanes; *w++ = p.chunk; *w++ = p.g1; *w++ = p.g2; *w++ = p.gBig;
    *w++ = p.metaBytes; *w++ = p.arenaBytes; *w++ = p.tablesBytes; *w++ = p.workspaceBytes; *w++ = p.bigListBytes; *w++ = p.e1ListBytes; *w++ = p.flat ? p.flatTablesBytes : 0; *w++ = p.bigWsBytes;
    *w++ = p.mbBlocksBytes; *w++ = p.mbCountBytes; *w++ = p.mbSeqsBytes; *w++ = p.mbMaxBlocks; *w++ = p.mbSeqCap; *w++ = p.mbLanes;
    *w++ = p.epochShift; *w++ = p.epochShift ? p.epochKeyLayout : 0; *w++ = p.flatMaxOpen; *w++ = p.flatMaxNeed;
    // the match stage of the first and of the last chunk (nothing where the plan has no flat stage): kernel + 1, the LDS kernels' shape, the flat kernel's probes, its fast form's pairs, grid, mbProbes
    const size_t cnts[2] = { in.n < p.chunk ? in.n : p.chunk, in.n - (in.n - 1) / p.chunk * p.chunk };
    for (size_t cnt : cnts) {
        ZeChunkPlan c; c.kernel = -1; c.grid = 0;
        if (p.flat) c = ze_encode_chunk_plan(in, p, cnt);
        const bool lds = c.kernel == ZE_MATCH_LDS || c.kernel == ZE_MATCH_LDS_FAST;
        *w++ = (uint64_t)(c.kernel + 1); *w++ = lds ? (uint64_t)c.shape : 0; *w++ = c.kernel == ZE_MATCH_FLAT ? (uint64_t)c.probes : 0; *w++ = c.kernel == ZE_MATCH_FLAT_FAST ? (uint64_t)c.fastPairs : 0;
        *w++ = c.grid; *w++ = p.flat ? c.mbProbes : 0;
    }
    return (int)(w - out);
}
