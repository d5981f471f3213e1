// zhip_decode_plan.hpp -- HOST side, free of HIP: the launch plan of device decompress. How zhip_decompress_batch_device (zhip_lib.hip) cuts a batch into chunks and slots, how much
// it reserves, which form of K1 / K2 / K3 it launches on which grid and whether K1b runs beside K2 is decided HERE, by pure functions of plain data: the library fills ZdPlanIn from
// its context, the emulator's pipeline harness (tests/emu/emu_kernels.cpp) fills it from its hooks, and both read the same ZdPlan -- the emulator tests hold the kernels to libzstd
// under the host's decisions, not under a copy of them.
// The measurement comments are the record of why each number is what it is; each stands at the line it explains.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "zhip_format.hpp"

#ifndef ZHIP_NSLOT
#define ZHIP_NSLOT 3
#endif
#ifndef ZHIP_SIDE
#define ZHIP_SIDE 1              // K1b beside K2 on a side stream; 0: the decode kernels one after the other on one stream, two chunk slots (rounds 1-5; A/B build)
#endif
#ifndef ZHIP_K0
#define ZHIP_K0 1                // K0 (zhip_decode_pre_kernel) in front of K1; 0: K1 parses every description itself (A/B build)
#endif
#ifndef ZHIP_DCHUNK
#define ZHIP_DCHUNK 65536        // frames per chunk of the decode pipeline (r02zl: 301 GB/s in one 65 536-frame chunk against 297 in two of 32 768: longer launches amortise their tails, and the two chunk slots overlap little anyway)
#endif
#ifndef ZHIP_K3_PER_CU
#define ZHIP_K3_PER_CU 0         // K3's grid in waves per CU (knob.k3PerCU); 0: what the occupancy query says for zhip_decode_exec_kernel. A build-time value for A/B
                                 // (build_variants.sh k3cu24). Round 8's three copies of the block code leave the kernel's registers, and so the query's 24, where they were;
                                 // the one build that had 70 VGPRs (query: 28) measured the same at 24 and 28 (profiles/r14_k3_batch_loop_literal_modes.txt, section 4): left at 0
#endif

// the decode knobs (zhip_ctx::Knobs carries them; read from the environment once when the context is created)
struct ZdDecodeKnobs {
    size_t k0Min = 6144;                // ZHIP_K0_MIN: frames per chunk from which K0 runs in front of K1 (a GPU test sets 0: K0 on every batch)
    size_t dchunk = ZHIP_DCHUNK;        // frames (several-block mode: block slots) per chunk
    int nslot = 2;                      // chunk slots on their own streams (small frames get a third)
    int k3PerCU = ZHIP_K3_PER_CU;       // waves per CU of K3 (0: what the occupancy query says)
};
// what a caller knows about the frames of ONE call (an argument, never context state: nothing is left behind by a call that fails)
struct ZdHints {
    uint64_t size = 0;                  // the largest content size where the caller says so: the batch's largest (host-buffer API, seekable readers), else zhip_ctx_set_size_hint's, else 0
    size_t slots = 0;                   // host-buffer API: block slots the frames of the batch are expected to need (1 per frame of one block, 2 per 128 KiB + 2 above: zd_host_hint), else 0
    bool hostPipe = false;              // the host-buffer pipeline is the caller (decompress_batch_one): its chunks' kernels are far from its bound -- the copies over the link -- and it
                                        // already keeps three streams busy; the decode step's side stream only added a queue for those copies to share (65 536 x 128 KiB inside a process
                                        // with other streams: 46-48 -> 38-43 GB/s with it, r06zl), so K1b stays on the chunk's stream there
};
struct ZdPlanDict { bool present = false, hasEntropy = false; };
struct ZdPlanDevice {
    int numCU = 0, decBlocksPerCU = 0, k1PerCU = 0, k3PerCU = 0;      // CUs, and resident waves per CU of the generic kernel, K1 and K3 (the occupancy queries of zhip_ctx_create)
    size_t k2LdsPerCU = 0, k1bLdsPerCU = 0;                           // one-wave workgroups of K2 / K1b a CU's LDS holds (the LDS bytes of a CU over sizeof(ZpSeqQLDS) / sizeof(ZpHufKernelLDS))
    size_t k2Frames = 15;                                             // frames per wave of K2 (ZQ_FRAMES, zhip_decode_pipeline.hpp)
};
struct ZdPlanIn {
    size_t n = 0;                       // frames of the call
    ZdHints hint; ZdPlanDict dict; bool prof = false;
    ZdDecodeKnobs knob; ZdPlanDevice dev;
    bool sideBuild = ZHIP_SIDE != 0, k0Build = ZHIP_K0 != 0; int nslotBuild = ZHIP_NSLOT;      // the build's switches
};

enum ZdK1Form { ZD_K1_PLAIN = 0, ZD_K1_LANES, ZD_K1_MB };      // a wave per frame; the lane-per-frame pass first, then a wave per frame it listed; a wave per frame over its blocks
enum ZdK2Form { ZD_K2_PLAIN = 0, ZD_K2_MB };
enum ZdK3Form { ZD_K3_EXEC = 0, ZD_K3_PROF, ZD_K3_DICT, ZD_K3_MB, ZD_K3_MB_DICT };
struct ZdPlan {
    bool tooLarge = false;              // "frame too large for the block arenas": nothing else of the plan is filled in
    bool mb = false, side = false, pre = false, k1Lanes = false;
    size_t perFrame = 1, slotsHint = 0;      // several-block mode: slots a frame gets by its size, and the host API's count for the batch (0: none)
    size_t chunk = 0, slots = 0, nChunks = 0; int nslot = 0;
    size_t arenaBudget16 = 0, arenaBytes = 0;
    // the reservations (preBytes where `pre`, the last three where `mb`; scratchBytes is the generic kernel's, sized by its grid BEFORE the clamp)
    size_t scratchBytes = 0, counterBytes = 0, basesBytes = 0, metaBytes = 0, litBytes = 0, countersBytes = 0, fallbackBytes = 0, fseBytes = 0, orderBytes = 0, hufBytes = 0, orderLitBytes = 0;
    size_t preBytes = 0, itemFrameBytes = 0, itemRepsBytes = 0, frameRecsBytes = 0;
    uint32_t genericGrid = 0;
};
struct ZdChunkPlan {
    uint32_t itemCap = 0;               // ZhipPipeArgs.itemCap: item slots of the chunk in the several-block mode, else 0
    size_t items = 0;                   // K1b / K2 / KB work items (an upper bound in the several-block mode)
    int k1 = ZD_K1_PLAIN, k2 = ZD_K2_PLAIN, k3 = ZD_K3_EXEC;
    uint32_t gPre = 0, gLanes = 0;      // K0 and the lane pass (0: not launched)
    uint32_t g1 = 0, gBin = 0, gHuf = 0, g2 = 0, g3 = 0, gCheck = 0;      // K1, the bin kernel, K1b, K2, K3, KX
};

// item slots of `frames` frames of a chunk (== frames without the several-block mode)
static inline size_t zd_slots_for(const ZdPlanIn& in, const ZdPlan& p, size_t frames)
{
    if (!p.mb) return frames;
    if (p.slotsHint) { const size_t want = 2 * (size_t)((double)frames * (double)p.slotsHint / (double)in.n + 1.0) + 64; return want < frames ? frames : want; }
    const size_t chunkMax = in.knob.dchunk;
    const size_t lo = frames * p.perFrame, hi = 2 * lo < chunkMax ? 2 * lo : chunkMax; return lo > hi ? lo : hi;
}

// The plan of a call: the phase-split fast path for single-block frames and, under a size hint, frames of several blocks (zhip_decode_pipeline.hpp); everything it declines
// lands in the fallback list consumed by the generic kernel behind it.
// Chunks of frames flow through K1 -> K2 -> K3 on ZHIP_NSLOT internal streams (slot = chunk % NSLOT, each slot has its own
// arenas and counters), so that different chunks' kernels overlap on the GPU: each phase is latency-bound with idle issue
// slots, and their LDS footprints differ, which is exactly when co-residency pays.
static inline ZdPlan zd_decode_plan(const ZdPlanIn& in)
{
    ZdPlan p;
    const size_t n = in.n;
    const size_t maxBlocks = (size_t)in.dev.numCU * (size_t)in.dev.decBlocksPerCU;
    uint32_t grid = (uint32_t)(n < maxBlocks ? n : maxBlocks);
    p.scratchBytes = (size_t)grid * ZHIP_LIT_STRIDE; p.counterBytes = 64;
    const size_t chunkMax = in.knob.dchunk; int slotMax = in.knob.nslot;      // measured on MI355X (profiles/README.md, r01c / r02f / r02zl): 65 536 frames per chunk, 2 slots
    // Frames of several blocks (the caller's size hint says so: the host API sets it from the items it sees): the several-block mode --
    // the arenas' slots are per BLOCK, a chunk is as many frames as fit `chunkMax` slots at the estimate below (libzstd cuts a block of
    // 128 KiB where the data changes; frames with more blocks than their share still work while the chunk has slots left, then
    // they are the generic kernel's)
    const uint64_t sizeHint = in.hint.size;
    // (small frames -- the caller says so -- are short kernels with launch gaps between them: a third chunk slot fills them. 262 144 x 4 KiB with the
    // shared dictionary: 123 -> 134 GB/s, r05q; frames of 128 KiB: the kernels are long, two slots overlap little as it is)
    if (sizeHint && sizeHint <= 16384 && slotMax < 3) slotMax = 3;
    const bool mb = sizeHint > ZF_BLOCK_MAX && sizeHint <= 0x7FFFFFFFull;     // (larger frames are the generic kernel's anyway)
    // K1b beside K2 on a side stream (zhip_decompress_batch_device) -- not for batches of small frames: their kernels are short, the three chunk slots overlap them already, and the
    // side streams only added queues (262 144 x 4 KiB with the dictionary: 199 -> 187 GB/s, r06p)
    const bool side = in.sideBuild && !in.hint.hostPipe && !(sizeHint && sizeHint <= 16384);
    // (with the side stream a batch of several chunks runs them one after the other on ONE slot stream: two slots' kernels side by side mix K3 with the next chunk's
    // K2 -- each slows the other, section 4.1 of DESIGN.md -- and the side stream has taken the tail the second slot used to fill. 131 072 x 128 KiB: 360 GB/s on two
    // slots with or without the side stream, 365-366 on one slot with it, and half the scratch (r06s). A single 128 KiB frame: 3.6 -> 2.4 ms, its two chains run together)
    if (side) slotMax = 1;
    // (two slots per 128 KiB decide how many frames make a chunk -- the slots are a pool, a frame may take more than its share; a chunk of
    // FEW frames has no pool to lean on and gets four: 64 x 128 KiB of changing data in one frame came as 235 blocks, r03x)
    // (the host-buffer API knows every frame's size and says how many slots the batch should need in all -- a batch of mostly small frames
    // with a few large ones is then not cut into chunks sized for the large ones: chunks are made for half the pool, the pool is twice
    // what the chunk is expected to use)
    const size_t perFrame = mb ? (size_t)(2 * ((sizeHint + ZF_BLOCK_MAX - 1) / ZF_BLOCK_MAX) + 2) : 1;
    const size_t slotsHint = mb ? in.hint.slots : 0;
    const size_t chunkFrames = !mb ? chunkMax : slotsHint ? (size_t)((double)n * (double)(chunkMax / 2) / (double)slotsHint) + 1 : (chunkMax / perFrame ? chunkMax / perFrame : 1);
    const size_t chunk = n < chunkFrames ? n : chunkFrames;
    p.mb = mb; p.side = side; p.perFrame = perFrame; p.slotsHint = slotsHint; p.chunk = chunk;
    const size_t slots = zd_slots_for(in, p, chunk);                                // item slots per chunk (== frames without the mode)
    p.slots = slots;
    if (slots > 0x7FFFFFFFu) { p.tooLarge = true; return p; }
    const size_t nChunks = (n + chunk - 1) / chunk;
    const int nslot = (int)(nChunks < (size_t)slotMax ? nChunks : (size_t)slotMax);
    p.nChunks = nChunks; p.nslot = nslot;
    // ONE compact arena holds literals and sequences (a "frame" below is an ITEM -- a block -- in the several-block mode): K1 claims what a
    // frame's literals need, K2 what a group's sequences need, from a per-chunk budget (ZhipPipeArgs.bases). A block's literals and sequences
    // trade off -- every sequence costs at least three bytes of output -- so the budget is common: 160 KiB per frame on average (the ratio-3 bench
    // corpus needs 45 KiB + 76 KiB, Huffman-only data 128 KiB + nothing, 4-symbol noise 3 + 150 KiB; the worst case, a match every three bytes, 350 KiB):
    // 10 GiB per 65 536-frame chunk instead of the 8 + 22 GiB of fixed slots, with up to 1 024 frames' worth of worst case as the floor so that small
    // batches never run out. What does not fit goes to the generic kernel (correct, slower).
    const size_t floorFrames = slots < 1024 ? slots : 1024;
    // (frames the caller says are SMALL cannot need more than their own worst case -- literals of the frame's size + 256, a sequence per three bytes in
    // rooms of the group's longest + 8 --: 4 x the size + 1 KiB; 4 KiB documents get 17 KiB each instead of 160)
    const size_t smallWorst = !mb && sizeHint && sizeHint < ZF_BLOCK_MAX ? 4 * (size_t)sizeHint + 1024 : (size_t)0;
    const size_t roomPerFrame = smallWorst && smallWorst < (160u << 10) ? smallWorst : (size_t)(160u << 10);
    size_t arenaBudget16 = slots * (roomPerFrame / 16);
    const size_t worstFrame = smallWorst ? smallWorst : (size_t)(ZP_SEQ_STRIDE + ZP_LIT_STRIDE);
    if (arenaBudget16 < floorFrames * (worstFrame / 16)) arenaBudget16 = floorFrames * (worstFrame / 16);
    if (arenaBudget16 > 0xFFFFFFF0u) arenaBudget16 = 0xFFFFFFF0u;
    const size_t arenaBytes = arenaBudget16 * 16 + 512;
    p.arenaBudget16 = arenaBudget16; p.arenaBytes = arenaBytes;
    p.basesBytes = nslot * slots * 2 * sizeof(uint32_t);
    p.metaBytes = nslot * slots * sizeof(ZdMeta); p.litBytes = nslot * arenaBytes + ZP_LIT_FRONT; p.countersBytes = (8 + (size_t)in.nslotBuild * ZP_CNT_WORDS) * 4; p.fallbackBytes = n * 4 + 16;
    p.fseBytes = nslot * slots * ZP_FSE_CELLS * sizeof(uint16_t); p.orderBytes = nslot * slots * sizeof(uint32_t);
    p.hufBytes = nslot * slots * ZP_HUF_CELLS * sizeof(uint16_t); p.orderLitBytes = nslot * slots * sizeof(uint32_t);
    // K0's records (one per frame; not in the several-block mode, whose K1 walks a frame's blocks in order, nor for dictionary batches, whose lane pass finishes what has no table of its own)
    // (... nor for small batches: K0 is a lane-serial walk of ~0.1 ms whatever the batch, which pays from ~6 000 frames on -- 2 048 frames 3.53 -> 3.62 ms with it, 8 192
    // 4.66 -> 4.62, 16 384 7.17 -> 6.96, 32 768 12.5 -> 12.0, 65 536 23.4 -> 22.4; `profiles/r06z2_k0_by_batch_size.txt`)
    p.pre = in.k0Build && !mb && !in.dict.hasEntropy && chunk >= in.knob.k0Min;
    if (p.pre) p.preBytes = nslot * slots * sizeof(ZpPre);
    if (mb) { p.itemFrameBytes = nslot * slots * sizeof(uint32_t); p.itemRepsBytes = nslot * slots * 4 * sizeof(uint32_t); p.frameRecsBytes = nslot * chunk * sizeof(ZpFrameRec); }
    // dictionary batches: a lane-per-frame pass first (zhip_decode_lit_lanes_kernel: frames whose tables are all the dictionary's are nothing but header
    // arithmetic), K1 then only over the frames that pass listed
    p.k1Lanes = !mb && in.dict.hasEntropy;
    // the generic kernel only sees the (usually empty) fallback list: a small grid is enough
    // (unless the caller says its frames exceed one block: then the list is the whole batch)
    if (grid > 1024 && (mb || !(sizeHint > ZF_BLOCK_MAX))) grid = 1024;
    p.genericGrid = grid;
    return p;
}
// a chunk of `cnt` frames: which form of K1, K2 and K3 runs, and every kernel's grid
static inline ZdChunkPlan zd_decode_chunk_plan(const ZdPlanIn& in, const ZdPlan& p, size_t cnt)
{
    ZdChunkPlan k;
    const ZdPlanDevice& dev = in.dev;
    if (p.mb) k.itemCap = (uint32_t)zd_slots_for(in, p, cnt);
    const size_t items = p.mb ? (size_t)k.itemCap : cnt;                         // K1b / K2 / KB work items (an upper bound in the several-block mode)
    k.items = items;
    size_t g1m = (size_t)dev.numCU * dev.k1PerCU, g3m = (size_t)dev.numCU * dev.k3PerCU;
    if (in.knob.k3PerCU) g3m = (size_t)dev.numCU * (size_t)in.knob.k3PerCU;
    // K2 and K1b are sized by LDS: as many one-wave workgroups per CU as their table sets fit (K2: 15 frames per wave -> 4)
    const size_t w2 = (items + dev.k2Frames - 1) / dev.k2Frames, g2m = (size_t)dev.numCU * dev.k2LdsPerCU;
    k.g1 = (uint32_t)(cnt < g1m ? cnt : g1m); k.g2 = (uint32_t)(w2 < g2m ? w2 : g2m); k.g3 = (uint32_t)(cnt < g3m ? cnt : g3m);
    const size_t wh = (items + ZP_HUF_FRAMES - 1) / ZP_HUF_FRAMES, ghm = (size_t)dev.numCU * dev.k1bLdsPerCU;
    k.gHuf = (uint32_t)(wh < ghm ? wh : ghm);
    k.k1 = p.mb ? ZD_K1_MB : p.k1Lanes ? ZD_K1_LANES : ZD_K1_PLAIN;
    const size_t w = (cnt + 63) / 64;                                            // waves of the lane-per-frame kernels
    if (!p.mb && p.pre) { const size_t gm = (size_t)dev.numCU * 7; k.gPre = (uint32_t)(w < gm ? w : gm); }      // (7 waves of 21.3 KiB of LDS per CU)
    if (k.k1 == ZD_K1_LANES) k.gLanes = (uint32_t)(w < g1m ? w : g1m);
    k.gBin = 2 * (items < 4096 ? 1u : 64u);                                      // tiny; timed with K1
    k.k2 = p.mb ? ZD_K2_MB : ZD_K2_PLAIN;
    // (ZHIP_PROF with a dictionary or frames of several blocks: K3's timers read zero -- said once at context creation)
    k.k3 = p.mb ? (in.dict.present ? ZD_K3_MB_DICT : ZD_K3_MB) : in.dict.present ? ZD_K3_DICT : in.prof ? ZD_K3_PROF : ZD_K3_EXEC;
    { const size_t gm = (size_t)dev.numCU * 8; k.gCheck = (uint32_t)(w < gm ? w : gm); }      // KX (returns at once when no frame carries a checksum; timed with K3)
    return k;
}

// What the host-buffer pipeline says about a chunk of its batch (ZdHints::size and ::slots): content sizes `len[i]` and, where a frame's block headers could be walked, its
// block count `nBlocks[i]` (else 0 or 1), for the `cnt` frames of the chunk.
static inline ZdHints zd_host_hint(const uint64_t* len, size_t lenStride, const uint32_t* nBlocks, size_t cnt)
{
    uint64_t mx = 0, slotsWanted = 0; size_t several = 0;
    for (size_t i = 0; i < cnt; i++) {
        const uint64_t l = len[i * lenStride];
        if (l > mx) mx = l;
        // (a frame's block count is known where its block headers could be walked: the slots it will take; else the estimate from its size)
        slotsWanted += nBlocks[i] > 1 ? (uint64_t)nBlocks[i] + 1 : l <= ZF_BLOCK_MAX ? 1 : 2 * ((l + ZF_BLOCK_MAX - 1) / ZF_BLOCK_MAX) + 2;
        several += nBlocks[i] > 1 && l <= ZF_BLOCK_MAX;
    }
    // frames of one block's size cut into SEVERAL blocks (the block splitter of levels 16+): from one in sixteen on the chunk takes the several-block mode -- a size hint just
    // above a block says so --, below that the few go to the generic kernel as before
    if (several * 16 >= cnt && mx <= ZF_BLOCK_MAX) mx = ZF_BLOCK_MAX + 1;
    ZdHints h; h.size = mx; h.slots = (size_t)slotsWanted; h.hostPipe = true;
    return h;
}
