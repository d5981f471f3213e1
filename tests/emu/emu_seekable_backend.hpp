// tests/emu/emu_seekable_backend.hpp -- the backend the emulator harness hands the sequences of python-zstandard_amd/csrc/zhip_seekable_calls.hpp: what
// zhip_lib.hip's ZskHipBackend does on the device, on the host. Every reserved area is a fresh heap allocation of exactly the reserved bytes, filled with 0xA5,
// so a layout whose arrays overlap or end beyond what was reserved shows as a wrong byte or as a heap overrun under the sanitizer programs; a launch is
// zhemu::run_grid over the kernel's body; the batch calls and the compaction are stand-ins that refuse a segment outside its buffer. Every launch is appended
// to `trace`. Test infrastructure only.
#pragma once
#define ZHIP_EMU 1
#include <stdint.h>
#include "../../python-zstandard_amd/csrc/zhip_seekable_calls.hpp"
#include <memory>

#define ZSK_X(id, name, A) static void name##_lane(void* p) { zsk_##name##_body(*(const A*)p); }
ZSK_KERNELS(ZSK_X)
#undef ZSK_X
#define ZSK_X(id, name, A) name##_lane,
static zhemu::lane_fn const emu_lanes[ZSK_K_COUNT] = {ZSK_KERNELS(ZSK_X)};
#undef ZSK_X

// what the trace calls the three steps that are no zhip_seekable_*_kernel: (id, grid) for the compaction, (id, items) for the batch calls
enum { EMU_T_COMPACT = ZSK_K_COUNT, EMU_T_COMPRESS, EMU_T_DECOMPRESS };
// emu_calls_mode: the CU count the next backends report, and whether they only record (the open call's scans always run: the host reads their results)
static int g_emuNumCU = 1; static bool g_emuTraceOnly = false;
static std::vector<uint32_t> g_emuTrace;                    // the last backend's (kernel, grid) pairs

struct EmuBackend {
    int numCU = g_emuNumCU; std::string text; std::string& err = text;
    bool traceOnly = g_emuTraceOnly;
    std::vector<uint32_t> trace;
    struct Area { std::unique_ptr<uint8_t[]> p; size_t bytes = 0; } areas[ZSK_A_COUNT];
    // what the kernels were handed: the arguments of the last verdict / segment launches (the hooks the tests read are filled from these)
    ZskCompressArgs sawCompress; ZskRecordsArgs sawRecords; ZskRangeArgs sawRange; ZskGatherArgs sawGather; ZskEditArgs sawEdit;
    uint32_t passes = 0; bool gather = false;
    // the compress stand-in: item i "compresses" to givenSizes[i] bytes of (31 * i + j) & 0xFF with status givenStatus[i]; sizesOnly: no bytes, and no size is refused
    const uint64_t* givenSizes = nullptr; const int32_t* givenStatus = nullptr; uint64_t srcSize = 0; bool sizesOnly = false;
    uint64_t refused = 0, copied = 0;                       // 1 + the first item whose segments the stand-in refused; the frames the compaction took
    // the decode stand-in: frame f "decodes" to content[dOff[f], dOff[f + 1]); shortFrame comes out one byte short, codeFrame reports `code` and writes nothing
    const uint8_t* content = nullptr; int64_t shortFrame = -1, codeFrame = -1; int32_t code = 0;
    uint8_t* dst = nullptr; uint64_t dstBytes = 0;
    uint64_t* segsOut = nullptr; uint64_t* itemsOut = nullptr; uint64_t itemCap = 0;
    uint8_t* poisonAt = nullptr; size_t poisonBytes = 0;    // set to 0xC3 behind the device-to-device copy (the edit call's stash)

    ~EmuBackend() { g_emuTrace = trace; }
    int reserve(ZskArea a, size_t bytes, uint8_t** base)
    {
        areas[a].p.reset(new uint8_t[bytes]); areas[a].bytes = bytes;
        memset(areas[a].p.get(), 0xA5, bytes);
        *base = areas[a].p.get();
        return 0;
    }
    void launch(ZskKernel k, uint32_t grid, const void* args)
    {
        trace.push_back(k); trace.push_back(grid);
        if (k == ZSK_K_VERDICT) sawCompress = *(const ZskCompressArgs*)args;
        if (k == ZSK_K_RECORDS_VERDICT) sawRecords = *(const ZskRecordsArgs*)args;
        if (k == ZSK_K_RANGE_SEGS) { sawRange = *(const ZskRangeArgs*)args; gather = false; }
        if (k == ZSK_K_GATHER_SEGS) { sawGather = *(const ZskGatherArgs*)args; gather = true; passes++; }
        if (k == ZSK_K_EDIT_VERDICT) sawEdit = *(const ZskEditArgs*)args;
        if (!traceOnly) zhemu::run_grid(grid, emu_lanes[k], (void*)args);
    }
    int check() { return 0; }
    int compress(const uint8_t*, const uint64_t* srcSegs, size_t n, uint8_t* slots, const uint64_t* slotSegs, uint64_t* outSizes, int32_t* status, size_t)
    {
        trace.push_back(EMU_T_COMPRESS); trace.push_back((uint32_t)n);
        if (traceOnly) return 0;
        const uint64_t slotBytes = areas[ZSK_A_SK_SLOTS].bytes;
        for (size_t i = 0; i < n; i++) {
            const uint64_t so = srcSegs[2 * i], sl = srcSegs[2 * i + 1], to = slotSegs[2 * i], tl = slotSegs[2 * i + 1];
            if (so + sl < so || so + sl > srcSize || to + tl < to || to + tl > slotBytes || tl < zsk_compress_bound(sl)) { if (!refused) refused = 1 + i; status[i] = 64; continue; }
            status[i] = givenStatus[i]; outSizes[i] = givenSizes[i];
            if (sizesOnly) continue;
            if (!status[i] && outSizes[i] > tl) status[i] = ZSK_ERR_DSTSIZE;       // (no frame is larger than its slot)
            if (!status[i]) for (uint64_t j = 0; j < outSizes[i]; j++) slots[(size_t)(to + j)] = (uint8_t)(31 * i + j);
        }
        return 0;
    }
    void compact(uint32_t grid, const uint8_t* slots, const uint64_t* slotSegs, const uint64_t* sizes, const int32_t* status, const uint64_t* offs, uint32_t n, uint8_t* to)
    {
        trace.push_back(EMU_T_COMPACT); trace.push_back(grid);
        if (traceOnly) return;
        for (uint32_t i = 0; i < n; i++) {
            if (status[i]) continue;
            copied++;
            if (!sizesOnly) memcpy(to + offs[i], slots + slotSegs[2 * i], (size_t)sizes[i]);
        }
    }
    // a negative number: a segment outside its buffer (-1), items out of frame order (-5), more items than itemsOut holds (-3)
    int decompress(const ZskOpened& o, const uint64_t* srcSegs, size_t n, uint8_t* dstBase, const uint64_t* dstSegs, uint64_t* outSizes, int32_t* status)
    {
        trace.push_back(EMU_T_DECOMPRESS); trace.push_back((uint32_t)n);
        if (traceOnly) return 0;
        const std::vector<uint64_t>& D = o.dOff;
        const uint32_t* const frameOf = gather ? sawGather.frameOf + sawGather.item0 : sawRange.frameOf;
        const Area& side = areas[gather ? ZSK_A_G_SCRATCH : ZSK_A_EDGE];
        for (size_t k = 0; k < n; k++) {
            const uint32_t f = frameOf[k];
            const uint64_t len = dstSegs[2 * k + 1];
            if (f >= o.lay.n || len != D[f + 1] - D[f] || !len) return -1;
            if (!gather && (f > sawRange.f1 || f < sawRange.f0)) return -1;
            uint8_t* const home = dstBase + dstSegs[2 * k];
            const bool inDst = dstBytes && home >= dst && home + len <= dst + dstBytes, inSide = side.bytes && home >= side.p.get() && home + len <= side.p.get() + side.bytes;
            if (!(inDst || inSide) || srcSegs[2 * k] != o.cOff[f] || srcSegs[2 * k + 1] != o.cOff[f + 1] - o.cOff[f]) return -1;
            if (k && frameOf[k - 1] >= f) return -5;
            if ((int64_t)f == codeFrame) { status[k] = code; outSizes[k] = 0; }
            else {
                const uint64_t out = len - ((int64_t)f == shortFrame ? 1 : 0);
                memcpy(home, content + D[f], out);
                outSizes[k] = out; status[k] = 0;
            }
            const uint64_t at = inDst ? (uint64_t)(home - dst) : (uint64_t)(home - side.p.get());
            if (segsOut) { uint64_t* q = segsOut + 4 * k; q[0] = srcSegs[2 * k]; q[1] = srcSegs[2 * k + 1]; q[2] = inDst ? at : (1ull << 63) + at; q[3] = len; }
            if (itemsOut) {
                const size_t item = (gather ? sawGather.item0 : 0) + k;
                if (item >= itemCap) return -3;
                uint64_t* q = itemsOut + 5 * item; q[0] = f; q[1] = inDst ? 0 : 1; q[2] = at; q[3] = len; q[4] = passes - 1;
            }
        }
        return 0;
    }
    int zero(void* p, size_t bytes) { memset(p, 0, bytes); return 0; }
    int copy(void* to, const void* from, size_t bytes, ZskCopy kind)
    {
        memcpy(to, from, bytes);
        if (kind == ZSK_COPY_ON_DEVICE && poisonBytes) memset(poisonAt, 0xC3, poisonBytes);
        return 0;
    }
    int wait() { return 0; }
};

// zhip_seekable_open_device on a stream in host memory: the handle and the backend that holds its areas. Returns 0 or the zstd error code
struct Opened : ZskOpened { EmuBackend b; };
static int open_stream(const uint8_t* stream, uint64_t size, Opened* o)
{
    int zerr = 0; size_t index = 0;
    const bool traceOnly = o->b.traceOnly;
    o->b.traceOnly = false;
    const int kind = zsk_open(o->b, stream, size, o, &zerr, &index);
    o->b.traceOnly = traceOnly; o->b.trace.clear();
    return kind == ZHIP_ERR_ZSTD ? zerr : kind;
}
