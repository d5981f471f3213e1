// tests/emu/emu_seekable_typed.cpp -- typed seekable streams (python-zstandard_amd/csrc/zhip_seekable_typed.hpp) on the host wave emulator: the split, join,
// seal and status bodies, and the whole calls of zhip_seekable_typed_calls.hpp over the emulator backend extended by the typed areas and kernels. The batch
// compressor is replaced by a stand-in that hands out the frames the test gives it (libzstd's frames of the planes) after checking every segment; the decoder
// by the backend's copy from the planar content. Test infrastructure only (tests/test_emu_seekable_typed.py; tests/emu/typed_planes_main.cpp is the
// stand-alone sanitizer program over the same functions).
#include "emu_seekable_backend.hpp"
#include "../../python-zstandard_amd/csrc/zhip_seekable_typed_calls.hpp"

#define ZSKT_X(id, name, A) static void name##_lane(void* p) { zsk_##name##_body(*(const A*)p); }
ZSKT_KERNELS(ZSKT_X)
#undef ZSKT_X
#define ZSKT_X(id, name, A) name##_lane,
static zhemu::lane_fn const emu_typed_lanes[ZSKT_K_COUNT] = {ZSKT_KERNELS(ZSKT_X)};
#undef ZSKT_X

enum { EMU_T_TYPED = 100 };      // what the trace calls typed kernel k: EMU_T_TYPED + k

struct EmuTypedBackend : EmuBackend {
    Area typed[ZSKT_A_COUNT];
    const uint8_t* frames = nullptr; const uint64_t* frameOffs = nullptr;      // the compress stand-in: item i is frames[frameOffs[i], frameOffs[i + 1])
    int reserve_typed(ZskTypedArea a, size_t bytes, uint8_t** base)
    {
        typed[a].p.reset(new uint8_t[bytes]); typed[a].bytes = bytes;
        memset(typed[a].p.get(), 0xA5, bytes);
        *base = typed[a].p.get();
        if (a == ZSKT_A_PLANAR) { dst = *base; dstBytes = bytes; }             // where the decode stand-in may write
        return 0;
    }
    void launch_typed(ZskTypedKernel k, uint32_t grid, const void* args)
    {
        trace.push_back(EMU_T_TYPED + k); trace.push_back(grid);
        if (!traceOnly) zhemu::run_grid(grid, emu_typed_lanes[k], (void*)args);
    }
    int compress(const uint8_t*, const uint64_t* srcSegs, size_t n, uint8_t* slots, const uint64_t* slotSegs, uint64_t* outSizes, int32_t* status, size_t srcMax)
    {
        if (!frames) return EmuBackend::compress(nullptr, srcSegs, n, slots, slotSegs, outSizes, status, srcMax);      // no frames given: the base backend's stand-in
        trace.push_back(EMU_T_COMPRESS); trace.push_back((uint32_t)n);
        const uint64_t slotBytes = areas[ZSK_A_SK_SLOTS].bytes;
        for (size_t i = 0; i < n; i++) {
            const uint64_t so = srcSegs[2 * i], sl = srcSegs[2 * i + 1], to = slotSegs[2 * i], tl = slotSegs[2 * i + 1], size = frameOffs[i + 1] - frameOffs[i];
            if (so + sl > srcSize || sl > srcMax || to + tl > slotBytes || tl < zsk_compress_bound(sl) || size > tl) { if (!refused) refused = 1 + i; status[i] = 64; continue; }
            status[i] = 0; outSizes[i] = size;
            memcpy(slots + to, frames + frameOffs[i], (size_t)size);
        }
        return 0;
    }
};
struct TypedOpened : ZskTypedOpened { EmuTypedBackend b; };
// zhip_seekable_open_device with its typed probe. Returns 0 or the zstd error code (*index: the frame it names)
static int open_typed(const uint8_t* stream, uint64_t size, TypedOpened* o, size_t* index)
{
    int zerr = 0;
    int kind = zsk_open(o->b, stream, size, o, &zerr, index);
    if (!kind) kind = zsk_typed_probe(o->b, o, &zerr, index);
    o->b.trace.clear();
    return kind == ZHIP_ERR_ZSTD ? zerr : kind;
}

// ------------------------------------------------------------------------------------------------ the bodies alone
// the split kernel on `grid` workgroups; records (where given) [nGroups * k][2]
extern "C" void emu_planes_split(const uint8_t* src, uint64_t size, uint32_t k, uint32_t group, uint8_t* dst, uint32_t grid, uint64_t* records)
{
    ZskPlanesArgs a; memset(&a, 0, sizeof a);
    a.src = src; a.dst = dst; a.elements = size / k; a.k = k; a.group = group; a.nGroups = (uint32_t)zsk_frame_count(a.elements, group); a.records = records;
    zhemu::run_grid(grid, planes_split_lane, &a);
}
// the join kernel on `grid` workgroups: jobs [nJobs][5] = planar, m, dst, h, t -- or, with jobs NULL, the groups of a whole buffer of `size` bytes
extern "C" void emu_planes_join(const uint8_t* planar, uint8_t* dst, const uint64_t* jobs, uint32_t nJobs, uint64_t size, uint32_t k, uint32_t group, uint32_t grid)
{
    std::vector<ZskJoinJob> js(nJobs);
    ZskJoinArgs a; memset(&a, 0, sizeof a);
    a.planar = planar; a.dst = dst; a.k = k; a.group = group; a.elements = size / k;
    if (jobs) {
        for (uint32_t j = 0; j < nJobs; j++) {
            js[j].planar = jobs[5 * j]; js[j].m = jobs[5 * j + 1]; js[j].dst = jobs[5 * j + 2]; js[j].h = (uint32_t)jobs[5 * j + 3]; js[j].t = (uint32_t)jobs[5 * j + 4];
            js[j].tilePrefix = a.tiles; a.tiles += zsk_join_tiles(js[j].m);
        }
        a.jobs = js.data(); a.nJobs = nJobs;
    } else a.tiles = zsk_planes_tiles(a.elements, group);
    zhemu::run_grid(grid, planes_join_lane, &a);
}
// the two seal kernels behind a stream of n frames that the records call wrote into dst (streamSize its size, 0: it failed). Returns the new size
extern "C" uint64_t emu_typed_seal(uint8_t* dst, uint64_t dstCapacity, uint64_t streamSize, uint32_t n, uint32_t checksum, uint32_t k, uint32_t frameSize, uint32_t grid, int32_t* outStatus)
{
    std::unique_ptr<uint8_t[]> stash(new uint8_t[(size_t)zsk_seal_stash_bytes(n, (int)checksum)]);
    ZskSealArgs s; memset(&s, 0, sizeof s);
    s.dst = dst; s.dstCapacity = dstCapacity; s.streamSize = &streamSize; s.outStatus = outStatus; s.stash = stash.get(); s.n = n; s.checksum = checksum; s.elementSize = k; s.frameSize = frameSize;
    zhemu::run_grid(grid, seal_stash_lane, &s);
    zhemu::run_grid(grid, seal_lane, &s);
    return streamSize;
}
extern "C" uint64_t emu_typed_bound(uint64_t srcSize, uint32_t frameSize, uint32_t k, int checksum) { return zsk_typed_bound(srcSize, frameSize, k, checksum); }
extern "C" uint32_t emu_typed_grid(int numCU, uint64_t size, uint32_t k, uint32_t group) { return zsk_tile_grid(numCU, zsk_planes_tiles(size / k, group), 0); }

// ------------------------------------------------------------------------------------------------ the whole calls
// Typed compress. frames / frameOffs [n * k + 1]: what the batch stand-in "compresses" the planes to. dst holds exactly dstCapacity bytes. Returns the
// library's code; info[0] = the stream size, info[1] = 1 + the first item whose segments the stand-in refused, info[2] = the staging area's bytes;
// stagingOut (where given, srcSize bytes) and recordsOut ([n * k][2]) receive what the split kernel wrote
extern "C" int emu_typed_compress(const uint8_t* src, uint64_t srcSize, uint32_t frameSize, uint32_t k, uint32_t checksum, const uint8_t* frames, const uint64_t* frameOffs,
                                  uint8_t* dst, uint64_t dstCapacity, int32_t* outStatus, uint8_t* stagingOut, uint64_t* recordsOut, uint64_t* info, char* text)
{
    memset(info, 0, 4 * sizeof(uint64_t));
    EmuTypedBackend b; b.frames = frames; b.frameOffs = frameOffs; b.srcSize = srcSize;
    uint64_t streamSize = ~0ull;
    const int rc = zsk_typed_compress(b, true, src, srcSize, frameSize, k, checksum ? ZHIP_SEEKABLE_CHECKSUM : 0, dst, dstCapacity, &streamSize, outStatus);
    if (text) snprintf(text, 256, "%s", b.text.c_str());
    if (rc) return rc;
    info[0] = streamSize; info[1] = b.refused; info[2] = b.typed[ZSKT_A_STAGING].bytes;
    if (stagingOut && srcSize) memcpy(stagingOut, b.typed[ZSKT_A_STAGING].p.get(), (size_t)srcSize);
    if (recordsOut && b.typed[ZSKT_A_RECORDS].bytes) memcpy(recordsOut, b.typed[ZSKT_A_RECORDS].p.get(), b.typed[ZSKT_A_RECORDS].bytes);
    return 0;
}
// the plain call through the typed entry (elementSize 1) and on its own, with the base backend's stand-in (item i: givenSizes[i] bytes of (31 * i + j) & 0xFF)
extern "C" uint64_t emu_typed_plain(const uint8_t* src, uint64_t srcSize, uint32_t frameSize, uint32_t checksum, const uint64_t* givenSizes, const int32_t* givenStatus, int viaTyped,
                                    uint8_t* dst, uint64_t dstCapacity, int32_t* outStatus)
{
    uint64_t streamSize = ~0ull;
    const int flags = checksum ? ZHIP_SEEKABLE_CHECKSUM : 0;
    if (viaTyped) {
        EmuTypedBackend b;
        b.givenSizes = givenSizes; b.givenStatus = givenStatus; b.srcSize = srcSize;
        if (zsk_typed_compress(b, true, src, srcSize, frameSize, 1, flags, dst, dstCapacity, &streamSize, outStatus)) return ~0ull;
    } else {
        EmuBackend b; b.givenSizes = givenSizes; b.givenStatus = givenStatus; b.srcSize = srcSize;
        if (zsk_compress(b, true, src, srcSize, frameSize, flags, dst, dstCapacity, &streamSize, outStatus)) return ~0ull;
    }
    return streamSize;
}
// the open call's verdict: 0 or the zstd error code; out[0] = the frame a failure names, out[1] = element size, out[2] = group elements, out[3] = frames, out[4] = content size
extern "C" int emu_typed_open(const uint8_t* stream, uint64_t size, uint64_t* out)
{
    TypedOpened o; size_t index = 0;
    memset(out, 0, 5 * sizeof(uint64_t));
    const int e = open_typed(stream, size, &o, &index);
    out[0] = index;
    if (!e) { out[1] = o.elementSize; out[2] = o.groupElements; out[3] = o.lay.n; out[4] = o.contentSize; }
    return e;
}
// the refusals of the typed compress call and of the kernels on their own: the code and the text
extern "C" int emu_typed_check(int which, uint64_t size, uint32_t frameSize, uint32_t k, int flags, char* text)
{
    std::string msg;
    const int rc = which ? zsk_planes_check(true, size, k, frameSize, msg) : zsk_typed_compress_check(true, size, frameSize, k, flags, msg);
    snprintf(text, 256, "%s", msg.c_str());
    return rc;
}
// the read plan alone: planarOut [cap][3], jobsOut [cap][6] = pass, planar, m, dst, h, t; passOut [cap][2] = bytes, tiles; ownerOut [R][2]. counts[3] = planar ranges, jobs, passes
extern "C" int emu_typed_plan(const uint8_t* stream, uint64_t size, const uint64_t* rg, uint64_t R, uint64_t limit, uint64_t cap, uint64_t* planarOut, uint64_t* jobsOut, uint64_t* passOut,
                              uint64_t* ownerOut, uint64_t* counts)
{
    TypedOpened o; size_t index = 0;
    if (int e = open_typed(stream, size, &o, &index)) return e;
    if (o.elementSize == 1) return -2;
    ZskTypedPlan plan;
    zsk_typed_plan(o.dOff.data(), o.elementSize, o.groupElements, rg, (size_t)R, limit, &plan);
    counts[0] = plan.planar.size() / 3; counts[1] = plan.jobs.size(); counts[2] = plan.passes.size();
    if (counts[0] > cap || counts[1] > cap || counts[2] > cap) return -3;
    memcpy(planarOut, plan.planar.data(), plan.planar.size() * 8);
    for (size_t p = 0; p < plan.passes.size(); p++) {
        passOut[2 * p] = plan.passes[p].bytes; passOut[2 * p + 1] = plan.passes[p].tiles;
        for (uint32_t j = plan.passes[p].job0; j < plan.passes[p].job1; j++) {
            const ZskJoinJob& x = plan.jobs[j]; uint64_t* q = jobsOut + 6 * j;
            q[0] = p; q[1] = x.planar; q[2] = x.m; q[3] = x.dst; q[4] = x.h; q[5] = x.t;
        }
    }
    for (size_t i = 0; i < 2 * (size_t)R; i++) ownerOut[i] = plan.owner[i];
    return 0;
}
// The typed read. content: the stream's PLANAR content (frame f "decodes" to content[dOff[f], dOff[f + 1])); frame codeFrame (-1: none) reports `code` and
// writes nothing. dst has exactly dstCapacity bytes. Returns the library's code, the open's error code, or a negative number from the decode stand-in.
// stats[7] = items, inPlace, scratchBytes, copyJobs, typed passes, the planar buffer's bytes, the rejected range's index
extern "C" int emu_typed_ranges(const uint8_t* stream, uint64_t size, const uint8_t* content, const uint64_t* rg, uint64_t R, uint8_t* dst, uint64_t dstCapacity, uint64_t limit,
                                int64_t codeFrame, int32_t code, int32_t* outStatus, uint64_t* stats, char* text)
{
    TypedOpened o; size_t index = 0;
    if (int e = open_typed(stream, size, &o, &index)) return e;
    memset(stats, 0, 7 * sizeof(uint64_t));
    o.scratchLimit = limit;
    EmuTypedBackend& b = o.b; b.content = content; b.codeFrame = codeFrame; b.code = code;
    zhip_seekable_gather_stats g; memset(&g, 0, sizeof g);
    size_t bad = 0;
    const int rc = zsk_typed_ranges(b, true, &o, rg, (size_t)R, dst, dstCapacity, outStatus, &g, &bad);
    if (text) snprintf(text, 256, "%s", b.text.c_str());
    stats[0] = g.items; stats[1] = g.inPlace; stats[2] = g.scratchBytes; stats[3] = g.copyJobs; stats[4] = g.passes; stats[5] = b.typed[ZSKT_A_PLANAR].bytes; stats[6] = bad;
    return rc;
}
