// tests/emu/emu_seekable_delta.cpp -- the delta filter of typed seekable streams on the host wave emulator: the split-with-delta body, the three
// launches of the delta join, zh_scan_add64, and the whole calls of zhip_seekable_typed_calls.hpp with a filter, over the emulator backend of
// emu_seekable_typed.cpp (included as it is, the way typed_planes_main.cpp includes it; its entry points serve filtered streams as they are where the handle
// knows the filter -- emu_typed_ranges). Test infrastructure only (tests/test_emu_seekable_delta.py; tests/emu/delta_planes_main.cpp is the stand-alone
// sanitizer program over the same functions).
#include "emu_seekable_typed.cpp"

// ------------------------------------------------------------------------------------------------ the bodies alone
static void scan64_lane(void* p) { uint64_t* v = (uint64_t*)p; v[64 + zh_lane()] = zh_scan_add64(v[zh_lane()]); }
// v [128]: 64 inputs, then the 64 inclusive sums
extern "C" void emu_scan_add64(uint64_t* v) { zhemu::run_grid(1, scan64_lane, v); }

extern "C" void emu_delta_split(const uint8_t* src, uint64_t size, uint32_t k, uint32_t group, uint8_t* dst, uint32_t grid, uint64_t* records)
{
    ZskPlanesArgs a; memset(&a, 0, sizeof a);
    a.src = src; a.dst = dst; a.elements = size / k; a.k = k; a.group = group; a.nGroups = (uint32_t)zsk_frame_count(a.elements, group); a.records = records;
    zhemu::run_grid(grid, planes_split_delta_lane, &a);
}
// the three launches on `grid` workgroups each: jobs [nJobs][6] = planar, m, dst, h, t, skip -- or, with jobs NULL, the groups of a whole buffer of `size`
// bytes. tileSums: exactly one uint64 per tile; it holds the tiles' offsets afterwards. Returns the tiles
extern "C" uint64_t emu_delta_join(const uint8_t* planar, uint8_t* dst, const uint64_t* jobs, uint32_t nJobs, uint64_t size, uint32_t k, uint32_t group, uint32_t grid, uint64_t* tileSums)
{
    std::vector<ZskJoinJob> js(nJobs);
    ZskJoinArgs a; memset(&a, 0, sizeof a);
    a.planar = planar; a.dst = dst; a.k = k; a.group = group; a.elements = size / k; a.tileSums = tileSums;
    if (jobs) {
        for (uint32_t j = 0; j < nJobs; j++) {
            const uint64_t* q = jobs + 6 * j;
            js[j].planar = q[0]; js[j].m = q[1]; js[j].dst = q[2]; js[j].h = (uint32_t)q[3]; js[j].t = (uint32_t)q[4]; js[j].skip = q[5];
            js[j].tilePrefix = a.tiles; a.tiles += zsk_join_tiles(js[j].m);
        }
        a.jobs = js.data(); a.nJobs = nJobs;
    } else a.tiles = zsk_planes_tiles(a.elements, group);
    if (!tileSums) return a.tiles;                 // (the tiles alone: what the caller has to allocate)
    zhemu::run_grid(grid, delta_sums_lane, &a);
    zhemu::run_grid(grid, delta_offsets_lane, &a);
    zhemu::run_grid(grid, planes_join_delta_lane, &a);
    return a.tiles;
}

// ------------------------------------------------------------------------------------------------ the whole calls
static size_t copy_trace(const std::vector<uint32_t>& t, uint32_t* out, size_t cap) { for (size_t i = 0; i < t.size() && i < cap; i++) out[i] = t[i]; return t.size(); }
// the stand-alone calls over the backend: which 0 = split, 1 = join. viaFilter 0: the call as it was (no filter argument). trace [cap]; returns the
// library's code, *traceWords = the words of the trace, info[0] = the bytes of the tile-sums area; sumsOut (where given): that area
extern "C" int emu_delta_planes_call(int which, int viaFilter, uint32_t filter, const uint8_t* src, uint64_t size, uint32_t k, uint32_t group, uint8_t* dst, uint32_t* trace, uint64_t cap,
                                     uint64_t* traceWords, uint64_t* info, uint64_t* sumsOut, char* text)
{
    EmuTypedBackend b;
    int rc;
    if (which == 0) rc = viaFilter ? zsk_planes_split(b, true, src, size, k, group, dst, filter) : zsk_planes_split(b, true, src, size, k, group, dst);
    else rc = viaFilter ? zsk_planes_join(b, true, src, size, k, group, dst, filter) : zsk_planes_join(b, true, src, size, k, group, dst);
    *traceWords = copy_trace(b.trace, trace, (size_t)cap);
    info[0] = b.typed[ZSKT_A_TILESUMS].bytes;
    if (sumsOut && info[0]) memcpy(sumsOut, b.typed[ZSKT_A_TILESUMS].p.get(), (size_t)info[0]);
    if (text) snprintf(text, 256, "%s", b.text.c_str());
    return rc;
}
// emu_typed_compress with a filter (viaFilter 0: the call without the argument) and the kernel trace
extern "C" int emu_delta_compress(int viaFilter, uint32_t filter, const uint8_t* src, uint64_t srcSize, uint32_t frameSize, uint32_t k, uint32_t checksum, const uint8_t* frames,
                                  const uint64_t* frameOffs, uint8_t* dst, uint64_t dstCapacity, int32_t* outStatus, uint8_t* stagingOut, uint64_t* info, uint32_t* trace, uint64_t cap,
                                  uint64_t* traceWords, char* text)
{
    memset(info, 0, 4 * sizeof(uint64_t));
    EmuTypedBackend b; b.frames = frames; b.frameOffs = frameOffs; b.srcSize = srcSize;
    uint64_t streamSize = ~0ull;
    const int flags = checksum ? ZHIP_SEEKABLE_CHECKSUM : 0;
    const int rc = viaFilter ? zsk_typed_compress(b, true, src, srcSize, frameSize, k, flags, dst, dstCapacity, &streamSize, outStatus, filter)
                             : zsk_typed_compress(b, true, src, srcSize, frameSize, k, flags, dst, dstCapacity, &streamSize, outStatus);
    *traceWords = copy_trace(b.trace, trace, (size_t)cap);
    if (text) snprintf(text, 256, "%s", b.text.c_str());
    if (rc) return rc;
    info[0] = streamSize; info[1] = b.refused; info[2] = b.typed[ZSKT_A_STAGING].bytes;
    if (stagingOut && srcSize) memcpy(stagingOut, b.typed[ZSKT_A_STAGING].p.get(), (size_t)srcSize);
    return 0;
}
// emu_typed_open, and out[5] = the filter
extern "C" int emu_delta_open(const uint8_t* stream, uint64_t size, uint64_t* out)
{
    TypedOpened o; size_t index = 0;
    memset(out, 0, 6 * sizeof(uint64_t));
    const int e = open_typed(stream, size, &o, &index);
    out[0] = index;
    if (!e) { out[1] = o.elementSize; out[2] = o.groupElements; out[3] = o.lay.n; out[4] = o.contentSize; out[5] = o.filter; }
    return e;
}
// emu_typed_plan under the opened stream's filter (forceNone: under no filter, whatever the marker says); jobsOut [cap][7] = pass, planar, m, dst, h, t, skip
extern "C" int emu_delta_plan(const uint8_t* stream, uint64_t size, const uint64_t* rg, uint64_t R, uint64_t limit, int forceNone, uint64_t cap, uint64_t* planarOut, uint64_t* jobsOut,
                              uint64_t* passOut, uint64_t* ownerOut, uint64_t* counts)
{
    TypedOpened o; size_t index = 0;
    if (int e = open_typed(stream, size, &o, &index)) return e;
    if (o.elementSize == 1) return -2;
    ZskTypedPlan plan;
    zsk_typed_plan(o.dOff.data(), o.elementSize, o.groupElements, rg, (size_t)R, limit, &plan, forceNone ? ZSK_FILTER_NONE : o.filter);
    counts[0] = plan.planar.size() / 3; counts[1] = plan.jobs.size(); counts[2] = plan.passes.size();
    if (counts[0] > cap || counts[1] > cap || counts[2] > cap) return -3;
    memcpy(planarOut, plan.planar.data(), plan.planar.size() * 8);
    for (size_t p = 0; p < plan.passes.size(); p++) {
        passOut[2 * p] = plan.passes[p].bytes; passOut[2 * p + 1] = plan.passes[p].tiles;
        for (uint32_t j = plan.passes[p].job0; j < plan.passes[p].job1; j++) {
            const ZskJoinJob& x = plan.jobs[j]; uint64_t* q = jobsOut + 7 * j;
            q[0] = p; q[1] = x.planar; q[2] = x.m; q[3] = x.dst; q[4] = x.h; q[5] = x.t; q[6] = x.skip;
        }
    }
    for (size_t i = 0; i < 2 * (size_t)R; i++) ownerOut[i] = plan.owner[i];
    return 0;
}
// the REFUSALS with a filter, through the calls themselves: which 0 = typed compress, 1 = the split on its own. *traceWords: what was launched (nothing may
// be); -9 where the call wrote a byte of the destination, the stream size or the status
extern "C" int emu_delta_check(int which, uint64_t size, uint32_t frameSize, uint32_t k, uint32_t filter, uint64_t* traceWords, char* text)
{
    EmuTypedBackend b; b.srcSize = size;
    std::vector<uint8_t> src((size_t)size + 1), dst((size_t)zsk_bound(size, frameSize ? frameSize : 1, 1) + 256, 0x5A);
    uint64_t streamSize = 0x5A5A5A5A5A5A5A5Aull; int32_t status[2] = {-1, -1};
    int rc;
    if (which == 0) rc = zsk_typed_compress(b, true, src.data(), size, frameSize, k, 0, dst.data(), dst.size(), &streamSize, status, filter);
    else rc = zsk_planes_split(b, true, src.data(), size, k, frameSize, dst.data(), filter);
    *traceWords = b.trace.size();
    for (uint8_t x : dst) if (x != 0x5A) return -9;
    if (streamSize != 0x5A5A5A5A5A5A5A5Aull || status[0] != -1 || status[1] != -1) return -9;
    snprintf(text, 256, "%s", b.text.c_str());
    return rc;
}
