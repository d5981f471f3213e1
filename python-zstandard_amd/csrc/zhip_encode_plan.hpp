// zhip_encode_plan.hpp -- HOST side, free of HIP: the launch plan of device compress. What zhip_compress_batch_device (zhip_lib.hip) launches, how much it reserves and
// how it cuts a batch into chunks is decided HERE, by pure functions of plain data: the library fills ZePlanIn from its context, the emulator harnesses (tests/emu/) fill it
// from their hooks, and both read the same ZePlan -- the emulator tests hold the kernels to libzstd under the host's decisions, not under a copy of them.
// The measurement comments are the record of why each number is what it is; each stands at the line it explains.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "zhip_cparams.hpp"
#include "zhip_format.hpp"

#ifndef ZHIP_E1LDS_PER_CU
#define ZHIP_E1LDS_PER_CU 4                // batches up to this many frames per CU take the LDS-source match kernel (ZHIP_E1LDS_MAX overrides the frame count); r02zq: 1 024 frames 147 ms against 159-163 with the flat kernel, 512: 89 against 146
#endif
#ifndef ZHIP_TABLE_EPOCHS
#define ZHIP_TABLE_EPOCHS 1      // launch numbers in the cells of the flat searches' tables; 0: the tables are zeroed every launch -- a memset, the dictionary search's own waves -- (A/B build)
#endif
#ifndef ZHIP_FAST_WIDE
#define ZHIP_FAST_WIDE 1          // fast-strategy batches above 32 768 sources: 65 536 per chunk at sixteen sources per wave; 0: chunks of 32 768 at eight (A/B build)
#endif

// the encode knobs (zhip_ctx::Knobs carries them; read from the environment once when the context is created)
struct ZeEncodeKnobs {
    size_t echunk = 0;                  // ZHIP_ECHUNK: sources per chunk, upper bound (0: none)
    size_t echunkMax = 0;               // ZHIP_ECHUNK_MAX: frames per launch of the flat match kernel (0 = 65 536, and 131 072 for larger batches where memory allows)
    long e1LdsMax = -1; size_t e1LdsRounds = 2;     // the LDS-source match kernel of small batches: most sources it takes (-1: by the CU count), rounds per CU
    size_t mbcMin = 4096;               // sources per 256 KiB of size hint from which sources of several blocks take the flat search (8 192 until r06zzi)
    unsigned mbcLanes = 32;             // sources per wave of that search (64 / 32 / 16 / 8 within 10-30 % of each other, r03z)
    // probes per trip of the flat double-fast search by launch size: up to flat4Max sources four (bound by one source's serial chain: 21-25 % less time from
    // 1 024 to 32 768 sources, r04zd), up to flat3Max three, above two (with the placement picked, at 65 536: 421 / 415 / 425 ms for two / three / four, r05w)
    size_t flat4Max = 32768, flat3Max = 65536; bool flat3 = true;
    // pairs per trip of the flat fast-strategy search (ze_fast_flat_np) by launch size: up to fast2Max sources two, above one. ZHIP_FAST_PAIRS=1 / 2 forces either (A/B, and the GPU test of both kernels)
    // (fast2Max is NOT measured yet: it is the double-fast search's four-probe band -- two pairs are four positions a trip -- taken over; tests/tools/compress_levels_rate.py under
    // ZHIP_FAST_PAIRS=1 and =2 at 16 384 and 65 536 sources is the measurement that sets it)
    size_t fast2Max = 32768; int fastPairs = 0;
};
struct ZePlanDict { bool present = false; int hlog = 0, clog = 0, strat = 2; uint32_t attachMax = ZE_DICT_ATTACH_MAX, contentSize = 0; };      // the digested dictionary's facts (ZeCDict)
struct ZePlanDevice { int numCU = 0, encBlocksPerCU = 0, e1PerCU = 0, e2PerCU = 0; };      // CUs, and resident waves per CU of the generic, lane-serial match and entropy kernels
struct ZePlanIn {
    ZeRows rows = {};                   // the context's parameters resolved per source-size class
    size_t n = 0;                       // sources of the call
    size_t sizeHint = 0;                // the largest source where the caller says so: the batch's largest (host-buffer API), else zhip_ctx_set_size_hint's, else 0
    size_t srcMaxHint = 0;              // the batch's largest source on its own (host-buffer API, else 0): the LDS shape follows it
    ZePlanDict dict; ZePlanDevice dev; ZeEncodeKnobs knob;
    bool fastWide = ZHIP_FAST_WIDE != 0, tableEpochs = ZHIP_TABLE_EPOCHS != 0; size_t e1LdsPerCU = ZHIP_E1LDS_PER_CU;      // the build's switches
    size_t flatMax = 65536;             // frames per launch of the flat match kernel for batches above 65 536 once decided: 65 536 or 131 072 (read where ZePlan::flatMaxOpen)
};

// the match-stage kernel in front of the lane-serial one, for one chunk
enum ZeMatchKernel { ZE_MATCH_LDS = 0, ZE_MATCH_LDS_FAST, ZE_MATCH_FLAT, ZE_MATCH_FLAT_FAST };
struct ZeChunkPlan {
    int kernel = ZE_MATCH_FLAT;         // ZeMatchKernel
    int shape = 3;                      // the LDS kernels: source bytes per CU slot 4 096 / 16 384 / 65 536 / one block
    int probes = 2, fastPairs = 0;      // the flat kernel: probes per trip (2, 3, 4); its fast form: pairs per trip (1, 2; 0: not the fast form)
    uint32_t grid = 0;
    uint32_t mbProbes = 0;              // probes per trip of the several-block search behind it (0: none runs)
};
struct ZePlan {
    bool greedy = false, anyDfast = false, mbcWanted = false, flatDict = false, flatFast = false, flat = false, allDfast = false, fastWide = false, mbc = false;
    bool flatMaxOpen = false; size_t flatMaxNeed = 0;       // the 131 072-per-launch regime is a question for this call (ZePlanIn::flatMax is read), and the free device bytes it needs
    uint32_t tableStride = 0, arenaStride = 0, arenaLit = 0, slotSrcMax = 0, e1Lanes = 0;
    size_t chunk = 0; uint32_t g1 = 0, g2 = 0, gBig = 0;
    size_t metaBytes = 0, arenaBytes = 0, tablesBytes = 0, workspaceBytes = 0, bigListBytes = 0, e1ListBytes = 0, flatTablesBytes = 0, bigWsBytes = 0;      // the reservations (flatTablesBytes: where `flat`)
    size_t mbBlocksBytes = 0, mbCountBytes = 0, mbSeqsBytes = 0;                                                                                        // (where `mbc`)
    uint32_t mbMaxBlocks = 0, mbSeqCap = 0, mbLanes = 0;
    uint32_t epochShift = 0;            // launch numbers in the flat tables' cells above this bit; 0: the cells carry none
    uint64_t epochKeyLayout = 0;        // the layout part of the key that tells numbered tables apart (the dictionary's fingerprint is the library's part)
    int ldsShape = 3; size_t ldsMax = 0;        // the LDS-source match kernel: its shape, and the most sources of a chunk it takes
    ZeChunkPlan pick;                   // the launch the table-placement pick times on a candidate allocation
};

// dictionary batches: every source is below the attach cutoff, so the per-lane tables are the dictionary row's shrunk to that
// size (ze_dict_cparams) and a frame's sequences + literals fit a slot of the cutoff's size -- a tenth of the 128 KiB shapes,
// which is what lets a whole 262 144-document batch be one chunk
// (round 4: where the caller says how large its sources are -- the host API knows, a device-API caller can tell with
// zhip_ctx_set_size_hint -- the slots are sized for THAT: 4 KiB documents need 48 KiB of tables, not the cutoff's 192, and 262 144 of
// them are one launch instead of two. A source above the hint is the generic kernel's: correct, slower)
// Sets *slotSrcMax (left alone where the slots are the cutoff's), *arenaLit and *arenaStride; returns the table bytes per source.
static inline uint32_t ze_dict_slots(const ZePlanDict& d, size_t sizeHint, uint32_t* slotSrcMax, uint32_t* arenaLit, uint32_t* arenaStride)
{
    size_t lim = d.attachMax;
    if (sizeHint && sizeHint < lim) { lim = 1024; while (lim < sizeHint) lim <<= 1; }
    if (lim < d.attachMax) *slotSrcMax = (uint32_t)lim; else lim = d.attachMax;
    int w = 10; while (((size_t)1 << w) < lim) w++;
    const int h = d.hlog > w + 1 ? w + 1 : d.hlog, cl = d.clog > w ? w : d.clog;
    uint32_t stride = (4u << h) + (d.strat == 2 ? (4u << cl) : 0u);
    if (stride < (4u << 10)) stride = 4u << 10;
    ze_dict_slot_shape((uint32_t)lim, arenaLit, arenaStride);
    return stride;
}
// waves of the entropy kernel over a chunk
static inline uint32_t ze_entropy_grid(const ZePlanDevice& dev, size_t chunk)
{
    const size_t g2max = (size_t)dev.numCU * (size_t)dev.e2PerCU;
    return (uint32_t)(chunk < g2max ? chunk : g2max);
}
// the slots and the chunk of the calls that run no match search of the library's: sequences from the caller (zhip_compress_sequences_device: full one-block slots whatever the
// level's strategy; dictionary batches the dictionary shape) and the wave match finder (ZHIP_FINDER_WAVE; no dictionary). Either call halves the chunk where its arena does not fit.
// (ZHIP_FINDER_NONE has no slots at all: ze_none_plan below.)
struct ZeSlotPlan { uint32_t arenaStride = 0, arenaLit = 0, slotSrcMax = 0; size_t chunk = 0; };
static inline ZeSlotPlan ze_sequences_plan(const ZePlanIn& in)
{
    ZeSlotPlan s;
    s.arenaStride = (uint32_t)ZE_ARENA_STRIDE; s.arenaLit = ZE_ARENA_LIT;
    if (in.dict.present) (void)ze_dict_slots(in.dict, in.sizeHint, &s.slotSrcMax, &s.arenaLit, &s.arenaStride);
    const size_t chunkMax = in.dict.present ? 262144 : 16384;                    // (7.4 GiB of one-block slots)
    s.chunk = in.n < chunkMax ? in.n : chunkMax;
    return s;
}
static inline ZeSlotPlan ze_wave_plan(const ZePlanIn& in)
{
    ZeSlotPlan s;
    s.arenaStride = (uint32_t)(ZE_ARENA_LIT + 512); s.arenaLit = ZE_ARENA_LIT;      // sequences only (mode 4): the slot needs no literal area
    s.chunk = in.n < 65536 ? in.n : 65536;
    if (in.knob.echunk && in.knob.echunk < s.chunk) s.chunk = in.knob.echunk;
    return s;
}
// no match search (ZHIP_FINDER_NONE, zhip_encode_none.hpp): the one kernel reads the sources and writes frames and a ZeMeta each -- no arena, so no arena stride and nothing
// to halve. What bounds a chunk is the context's meta buffer (16 bytes a source) and the 32-bit work counter: 65 536 sources, the chunk the default finder and the wave
// finder already size that buffer for (1 MiB), so a context that alternates finders never grows it for this one; a launch more per 65 536 sources costs microseconds against
// the milliseconds each takes.
struct ZeNonePlan { size_t chunk = 0; uint32_t grid = 0; size_t metaBytes = 0; };
// what makes the compress call as a whole refuse under ZHIP_FINDER_NONE (the zhip_last_error text, null: served), as under the wave finder: a dictionary, or a one-block row
// (sources of 16 385 ... 131 072 bytes) that is not fast or double-fast. Where only the row of smaller sources is something else (level 4), those sources are refused one by one.
static inline const char* ze_none_refusal(const ZeRows& rows, bool hasDict)
{
    if (hasDict) return "no match search (ZHIP_FINDER_NONE, match finder \"none\") does not take a dictionary";
    if (rows.r[2][6] != 1 && rows.r[2][6] != 2)
        return "no match search (ZHIP_FINDER_NONE, match finder \"none\") serves the levels whose one-block row is fast or double-fast (levels <= 4, negative levels, explicit strategy 1 / 2)";
    return nullptr;
}
static inline ZeNonePlan ze_none_plan(const ZePlanIn& in)
{
    ZeNonePlan s;
    s.chunk = in.n < 65536 ? in.n : 65536;
    if (in.knob.echunk && in.knob.echunk < s.chunk) s.chunk = in.knob.echunk;
    s.grid = ze_entropy_grid(in.dev, s.chunk);                                      // one wave per source, sources claimed from the chunk's counter: the entropy kernel's grid
    s.metaBytes = s.chunk * sizeof(ZeMeta);
    return s;
}

// The plan of zhip_compress_batch_device's default match finder:
// two kernels: E1 searches with one LANE per frame (frames in flight hide the probe latency), E2 entropy-codes with one
// wave per frame. Frames are processed in chunks so that the per-frame sequence/literal arena stays bounded.
static inline ZePlan ze_encode_plan(const ZePlanIn& in)
{
    ZePlan p;
    const ZeRows& rows = in.rows; const ZeEncodeKnobs& knob = in.knob; const ZePlanDevice& dev = in.dev;
    const bool hasCDict = in.dict.present; const size_t n = in.n;
    // table bytes of the largest one-block source of the two size classes these kernels serve (<= 128 KiB, <= 16 KiB), after the
    // per-source adjustment ze_get_cparams makes (windowLog <= 17 / 14, hashLog <= windowLog + 1, chainLog <= windowLog)
    // (greedy: the row match finder's positions and tags, 5 << hashLog bytes -- 640 KiB at level 5; only the row of 16 385 ... 131 072-byte sources can be served, ze_get_cparams)
    p.greedy = !hasCDict && rows.r[2][6] == 3 && rows.r[2][0] >= 15 && rows.r[2][3] <= 4;
    uint32_t stride = 0;
    for (int t = 2; t < 4; t++) {
        const int32_t* r = rows.r[t];
        if (r[6] != 1 && r[6] != 2 && !(p.greedy && t == 2)) continue;
        const int w = r[0] < (t == 2 ? 17 : 14) ? r[0] : (t == 2 ? 17 : 14);
        const int h = r[2] > w + 1 ? w + 1 : r[2], cl = r[1] > w ? w : r[1];
        const uint32_t bytes = r[6] == 3 ? (5u << h) : (4u << h) + (r[6] == 2 ? (4u << cl) : 0u);
        if (bytes > stride) stride = bytes;
        p.anyDfast |= r[6] == 2;
    }
    // (sources of several blocks in the flat kernel -- `mbc` below: the rows of the larger size classes count too, at the hint's size)
    const size_t sizeHint = in.sizeHint;
    // (worth it from ~8 000 sources on. Either kernel's time is a source's serial chain of probes -- ~0.2 s per 128 KiB of source at these
    // batch sizes -- times the ROUNDS it needs: the generic kernel holds ~4 096 searches at a time (one per wave), the flat one a whole chunk
    // (64 per wave, whose every trip waits for the slowest of 64 requests and runs every lane's branch: ~10 % slower per round at 256 KiB,
    // 50 % at 512 KiB+). r03u / r03v, flat against generic: 2 048 x 1 MiB 2.5 s / 1.04 s, 4 096 x 512 KiB 1.31 / 0.85, 4 096 x 256 KiB
    // 0.44 / 0.42, 8 192 x 256 KiB 0.47 / 0.68, 16 384 x 256 KiB 0.51 / 1.24, 8 192 x 1 MiB 3.3 / ~2.1: the longer the sources the more
    // rounds of the generic kernel it takes to lose, hence the threshold grows with the size hint -- ZHIP_MBC_MIN sources per 256 KiB of it.
    // Round 6's kernels, flat / generic (r06zzi): 3 072 x 256 KiB 340 / 325 ms, 4 096 x 256 KiB 351 / 420, 6 144 x 384 KiB 810 / 846, 4 096 x 512 KiB 1 075 / 860,
    // 8 192 x 512 KiB 1 191 / 1 417, 12 288 x 512 KiB 1 639 / 1 965, 2 048 x 1 MiB 1 950 / 1 034: the flat search wins from 4 096 per 256 KiB on, was 8 192)
    p.mbcWanted = p.anyDfast && !hasCDict && n >= knob.mbcMin * ((sizeHint + (256u << 10) - 1) / (256u << 10)) && sizeHint > ZF_BLOCK_MAX && sizeHint < ((size_t)1 << ZE_MB_POS_BITS) - 8;
    if (p.mbcWanted) for (int t = 0; t < 2; t++) {
        const int32_t* r = rows.r[t];
        if (r[6] != 2) continue;
        int w = 17; while (((size_t)1 << w) < sizeHint) w++;
        if (w > r[0]) w = r[0];
        const int h = r[2] > w + 1 ? w + 1 : r[2], cl = r[1] > w ? w : r[1];
        const uint32_t bytes = (4u << h) + (4u << cl);
        if (bytes > stride && bytes <= (12u << 17)) stride = bytes;
    }
    if (stride < (4u << 10)) stride = 4u << 10;
    if (stride > (12u << 17)) stride = 12u << 17;                  // larger tables: the frame is refused loudly by the match kernels
    p.arenaStride = (uint32_t)ZE_ARENA_STRIDE; p.arenaLit = ZE_ARENA_LIT;
    if (hasCDict) stride = ze_dict_slots(in.dict, sizeHint, &p.slotSrcMax, &p.arenaLit, &p.arenaStride);
    p.tableStride = stride;
    // double-fast without a dictionary: the flat match kernel (one lane per frame, the whole chunk in flight, tables zeroed by a
    // memset) takes every double-fast frame; what it declines goes to the lane-serial kernel through a list. Dictionary batches of the
    // fast strategy, and fast batches of several-block sources, use the lane-serial kernel for the whole chunk.
    // (r03: dictionary batches whose dictionary row is double-fast take the flat kernel too -- ze_dfast_dict_flat; its waves zero the tables)
    p.flatDict = hasCDict && in.dict.strat == 2;
    // (round 7) the fast strategy without a dictionary has a flat search too (ze_fast_flat_np): when BOTH one-block rows are fast the fast form of the kernel is
    // launched, which takes the fast sources and leaves nothing but errors and tiny sources to the lane-serial kernel. A batch whose two one-block rows differ
    // (explicit parameters cannot do that, the level tables do not) keeps the double-fast kernel, which hands its fast sources to the lane-serial search.
    // Batches whose size hint says "sources of several blocks" stay where they were: the lane-serial kernel's chunk shapes (fastWide below), which only list such sources.
    p.flatFast = !hasCDict && rows.r[2][6] == 1 && rows.r[3][6] == 1 && sizeHint <= ZF_BLOCK_MAX;
    p.flat = (p.anyDfast && !hasCDict) || p.flatDict || p.flatFast;
    // (round 5) every row double-fast, no dictionary: the flat kernel takes every one-block source of 64 bytes and more and writes sequences only, and what
    // it declines -- sources below 64 bytes, parameter errors -- needs a literal area of its own size at most: the slot is the sequence area + 512 bytes
    // instead of + 128 KiB (21.4 GiB of arena per 65 536 sources instead of 30; it is what lets 262 144 sources be one launch, 88 + 96 GiB)
    // (round 7: every row fast OR double-fast. Whichever form of the flat kernel runs, the one-block sources it declines for their strategy are fast ones,
    // and the lane-serial fast search writes sequences only as well)
    p.allDfast = (p.anyDfast || p.flatFast) && !hasCDict; for (int t = 0; t < 4; t++) p.allDfast = p.allDfast && (rows.r[t][6] == 2 || rows.r[t][6] == 1);
    if (p.flat && p.allDfast) p.arenaStride = (uint32_t)(ZE_ARENA_LIT + 512);
    // frames per launch of the flat match kernel: the search is a latency chain per frame, so its rate grows with the frames in flight -- 16 384: 204 ms,
    // 32 768: 270, 65 536: 417, 131 072: 760 (r04za: 9 % less per frame than two launches of 65 536, a second wave per SIMD) -- and what it costs
    // is memory, 384 KiB of tables + 196 KiB of arena per frame. Batches above 65 536 take 131 072 per launch where the device has that free.
    // (the decision is taken once per context -- hipMemGetInfo is not a launch-path call -- and a reservation that fails at 131 072
    // after all, because another context took the memory in between, falls back to 65 536 instead of failing the call: the library's side, flat_max_decided)
    size_t flatMax = knob.echunkMax;
    if (!flatMax) {
        flatMax = 65536;
        if (p.flat && !hasCDict && n > 65536) {
            p.flatMaxOpen = true;
            p.flatMaxNeed = (size_t)131072 * ((size_t)p.tableStride + (size_t)p.arenaStride) / 8 * 9 + ((size_t)4 << 30);
            flatMax = in.flatMax;
        }
    }
    // (the fast strategy -- levels 1, 2, negative -- where it still runs in the lane-serial match kernel, i.e. under a size hint above one block: its time is ONE source's chain of dependent round trips: every source in flight at once
    // is one chain's time, two chunks of 32 768 are two. ZHIP_FAST_WIDE: 65 536 per chunk, sixteen sources per wave -- the kernel's 111 VGPRs hold 4 096 waves)
    p.fastWide = in.fastWide && !p.flat && !hasCDict && n > 32768;
    size_t chunkMax = hasCDict ? 262144 : p.flat ? flatMax : p.fastWide ? 65536 : 32768;
    if (p.flat) { const size_t byMem = ((size_t)(flatMax > 65536 ? 96 : 32) << 30) / p.tableStride; if (chunkMax > byMem) chunkMax = byMem; }
    if (knob.echunk && knob.echunk < chunkMax) chunkMax = knob.echunk;
    // Sources of several blocks (the caller's size hint says so) in a double-fast batch without dictionary: the flat kernel searches them
    // too, a lane per frame over all its blocks (ZeMbBlock, zhip_format.hpp); the generic kernel then only does their entropy coding and
    // runs once per chunk. Per frame: block records and room for its sequences (a sequence covers four bytes or more).
    p.mbc = p.flat && !p.flatDict && p.mbcWanted;
    const size_t mbMaxBlocks = p.mbc ? 2 * ((sizeHint + ZF_BLOCK_MAX - 1) / ZF_BLOCK_MAX) + 2 : 0;
    const size_t mbSeqCap = p.mbc ? sizeHint / 4 + mbMaxBlocks + 64 : 0;          // (double-fast matches are four bytes or more: zstd.c:31167 / :31150)
    if (p.mbc) { const size_t byMem = ((size_t)32 << 30) / (mbSeqCap * 8); if (chunkMax > byMem) chunkMax = byMem ? byMem : 1; }
    const size_t chunk = n < chunkMax ? n : chunkMax;                        // items the arenas are sized for
    p.chunk = chunk;
    const size_t laneCap = hasCDict ? 262144 : p.fastWide ? 65536 : 32768;          // lanes of the lane-serial match kernel in flight (each owns tableStride bytes of tables)
    const size_t e1Lanes = hasCDict ? ZE_E1_LANES_DICT : p.fastWide ? 16 : ZE_E1_LANES;
    p.e1Lanes = (uint32_t)e1Lanes;
    size_t g1max = (size_t)dev.numCU * (size_t)dev.e1PerCU; if (g1max * e1Lanes > laneCap) g1max = laneCap / e1Lanes;
    if (p.flat && g1max > 256) g1max = 256;                                      // only the frames the flat kernel declines
    if (p.greedy) { const size_t byMem = ((size_t)8 << 30) / (e1Lanes * (size_t)p.tableStride); if (g1max > byMem) g1max = byMem ? byMem : 1; }      // (row tables: 8 GiB of them at most, 1 638 waves at level 5)
    const size_t w1 = (chunk + e1Lanes - 1) / e1Lanes;
    p.g1 = (uint32_t)(w1 < g1max ? w1 : g1max);
    p.g2 = ze_entropy_grid(dev, chunk);
    // waves for what the generic kernel takes: inputs above one block, and -- with a dictionary -- inputs above the attach cutoff
    // (with a dictionary: inputs above the attach cutoff too. Every wave of this kernel carries 544 bytes of scratch per lane: a full-chip
    // grid that finds an empty list still took 2.3 ms of every dictionary batch -- r02zi kernel trace; half a wave per CU is 0.4)
    // (r03: when the caller says its sources exceed one block -- the host API knows, a device-API caller can tell with zhip_ctx_set_size_hint --
    // the list is the whole batch and gets the whole chip: 2 048 x 1 MiB took 10.6 s on 64 waves, profiles/r03_multiblock_rate.txt)
    const size_t gBigMax = sizeHint > ZF_BLOCK_MAX ? (size_t)dev.numCU * (size_t)dev.encBlocksPerCU : hasCDict ? (size_t)dev.numCU / 2 : 64;
    p.gBig = (uint32_t)(n < gBigMax ? n : gBigMax);
    p.metaBytes = chunk * sizeof(ZeMeta); p.arenaBytes = chunk * (size_t)p.arenaStride;
    p.tablesBytes = (size_t)p.g1 * e1Lanes * p.tableStride; p.workspaceBytes = (size_t)p.g2 * ZE_E2_STRIDE + ZHIP_ENC_STRIDE;
    p.bigListBytes = n * sizeof(uint32_t) + 16; p.e1ListBytes = chunk * sizeof(uint32_t) + 16; p.bigWsBytes = (size_t)p.gBig * ZHIP_ENC_STRIDE;
    p.flatTablesBytes = chunk * (size_t)p.tableStride;
    if (p.mbc) {
        p.mbBlocksBytes = chunk * mbMaxBlocks * sizeof(ZeMbBlock); p.mbCountBytes = chunk * sizeof(uint32_t) + 16; p.mbSeqsBytes = chunk * mbSeqCap * 8;
        p.mbMaxBlocks = (uint32_t)mbMaxBlocks; p.mbSeqCap = (uint32_t)mbSeqCap; p.mbLanes = knob.mbcLanes;
    }
    // The dictionary search's tables are not zeroed per launch: a cell carries its launch's number above the index and reads as empty under any other number.
    // The index space is 2 + the dictionary's content + a source (+ slack): what is left of 32 bits counts launches, at least 6 bits or the kernel zeroes as before.
    // (the dictionary-less flat search of one-block sources does the same with six fixed bits: its cells are position 18 | tag 8 | launch number 6, ze_dfast_flat_np. No
    // launch numbers in the tables of the several-block search, or where the index space is too wide: the caller zeroes them as before.)
    if (in.tableEpochs && p.flat && !p.mbc) {
        uint32_t es = 26;
        if (p.flatDict) {
            const uint64_t span = 2ull + in.dict.contentSize + (p.slotSrcMax ? p.slotSrcMax : in.dict.attachMax) + 64;
            es = 1; while ((1ull << es) < span) es++;
        }
        if (es <= 26) p.epochShift = es;
    }
    // (the key tells table LAYOUTS apart: the dictionary, the slot size, and -- round 7 -- one table per slot (fast) or two (double-fast). The cells of both carry
    // the launch number in the same six bits, so neither would read the other's as live inside one run of numbers; a change of layout zeroes and restarts anyway)
    p.epochKeyLayout = ((uint64_t)p.tableStride << 40) ^ (p.flatFast ? 0x00000000FA570000ull : 0ull);
    // a few frames: nothing hides the search's round trips, so each frame gets a CU and its source goes to LDS (ze_match_lds_body)
    // (the LDS area follows the batch's largest source where the caller told us -- the host-buffer API does: more frames per CU)
    const size_t hint = in.srcMaxHint ? in.srcMaxHint : (size_t)ZF_BLOCK_MAX;
    p.ldsShape = hint <= 4096 ? 0 : hint <= 16384 ? 1 : hint <= 65536 ? 2 : 3;
    static const unsigned wavesPerCU[4] = { 32, 9, 2, 1 };          // by LDS (160 KiB per CU) and the 32-wave limit
    const size_t rounds = p.ldsShape == 3 ? in.e1LdsPerCU : knob.e1LdsRounds;
    p.ldsMax = knob.e1LdsMax >= 0 ? (size_t)knob.e1LdsMax : (size_t)dev.numCU * wavesPerCU[p.ldsShape] * rounds;
    // the placement pick's launch: the flat kernel whatever the chunk's size, never four probes, the fast form at one pair
    p.pick.kernel = p.flatFast ? ZE_MATCH_FLAT_FAST : ZE_MATCH_FLAT; p.pick.shape = p.ldsShape;
    p.pick.probes = !p.flatDict && knob.flat3 && chunk <= knob.flat3Max ? 3 : 2; p.pick.fastPairs = p.flatFast ? 1 : 0;
    p.pick.grid = (uint32_t)((chunk + ZE_FLAT_LANES - 1) / ZE_FLAT_LANES);
    return p;
}
// the match stage of a chunk of `cnt` sources of a plan with `flat` (without, only the lane-serial kernel runs)
static inline ZeChunkPlan ze_encode_chunk_plan(const ZePlanIn& in, const ZePlan& p, size_t cnt)
{
    ZeChunkPlan k;
    const ZeEncodeKnobs& knob = in.knob;
    k.shape = p.ldsShape;
    k.fastPairs = !p.flatFast ? 0 : knob.fastPairs ? knob.fastPairs : cnt <= knob.fast2Max ? 2 : 1;
    k.probes = !p.flatDict && !p.mbc && cnt <= knob.flat4Max ? 4 : !p.flatDict && !p.mbc && knob.flat3 && cnt <= knob.flat3Max ? 3 : 2;
    if (cnt <= p.ldsMax && p.flatFast) k.kernel = ZE_MATCH_LDS_FAST;
    else if (cnt <= p.ldsMax && !p.flatDict && !p.mbc) k.kernel = ZE_MATCH_LDS;
    else k.kernel = k.fastPairs ? ZE_MATCH_FLAT_FAST : ZE_MATCH_FLAT;
    k.grid = k.kernel <= ZE_MATCH_LDS_FAST ? (uint32_t)cnt : (uint32_t)((cnt + ZE_FLAT_LANES - 1) / ZE_FLAT_LANES);
    // (the traffic in flight is sources x blocks each: 16 384 x 256 KiB 7.9 -> 8.9 GB/s with four probes, 32 768 x 256 KiB 12.0 -> 11.8, r04zj)
    if (p.mbc) k.mbProbes = p.chunk * ((in.sizeHint + ZF_BLOCK_MAX - 1) / ZF_BLOCK_MAX) <= knob.flat4Max ? 4u : 2u;
    return k;
}
