// tests/emu/emu_seekable_xor_base.cpp -- the xor-with-base filter of typed seekable streams on the host wave emulator: the split-with-xor and
// join-with-xor bodies, and the whole calls of zhip_seekable_typed_calls.hpp that take a base, over the emulator backend of emu_seekable_typed.cpp.
// emu_seekable_delta.cpp is included as it is (the way delta_planes_main.cpp includes it), so the entries of before -- emu_typed_plan, emu_delta_plan,
// emu_delta_open, emu_typed_ranges, ... -- are in this library too, built against the same headers: what they return is compared with what the entries here
// return. Test infrastructure only (tests/test_emu_seekable_xor_base.py; tests/emu/xor_planes_main.cpp is the stand-alone sanitizer program over the same functions).
#include "emu_seekable_delta.cpp"

// ------------------------------------------------------------------------------------------------ the bodies alone
extern "C" void emu_xor_split(const uint8_t* src, const uint8_t* base, uint64_t size, uint32_t k, uint32_t group, uint8_t* dst, uint32_t grid, uint64_t* records)
{
    ZskPlanesXorArgs x; memset(&x, 0, sizeof x);
    ZskPlanesArgs& a = x.p;
    a.src = src; a.dst = dst; a.elements = size / k; a.k = k; a.group = group; a.nGroups = (uint32_t)zsk_frame_count(a.elements, group); a.records = records;
    x.base = base;
    zhemu::run_grid(grid, planes_split_xor_lane, &x);
}
// the join on `grid` workgroups: jobs [nJobs][6] = planar, m, dst, h, t, content -- or, with jobs NULL, the groups of a whole buffer of `size` bytes.
// base: the pointer the kernel adds the content offsets to
extern "C" void emu_xor_join(const uint8_t* planar, const uint8_t* base, uint8_t* dst, const uint64_t* jobs, uint32_t nJobs, uint64_t size, uint32_t k, uint32_t group, uint32_t grid)
{
    std::vector<ZskJoinJob> js(nJobs);
    std::vector<uint64_t> content(nJobs);
    ZskJoinXorArgs x; memset(&x, 0, sizeof x);
    ZskJoinArgs& a = x.j;
    a.planar = planar; a.dst = dst; a.k = k; a.group = group; a.elements = size / k;
    x.base = base;
    if (jobs) {
        for (uint32_t j = 0; j < nJobs; j++) {
            const uint64_t* q = jobs + 6 * j;
            js[j].planar = q[0]; js[j].m = q[1]; js[j].dst = q[2]; js[j].h = (uint32_t)q[3]; js[j].t = (uint32_t)q[4]; js[j].skip = 0; content[j] = q[5];
            js[j].tilePrefix = a.tiles; a.tiles += zsk_join_tiles(js[j].m);
        }
        a.jobs = js.data(); a.nJobs = nJobs; x.content = content.data();
    } else a.tiles = zsk_planes_tiles(a.elements, group);
    zhemu::run_grid(grid, planes_join_xor_lane, &x);
}

// ------------------------------------------------------------------------------------------------ the whole calls
// the stand-alone calls with a base over the backend: which 0 = split, 1 = join. Returns the library's code; trace [cap], *traceWords = its words;
// info[0] = the bytes of the tile-sums area (none is wanted)
extern "C" int emu_xor_planes_call(int which, const uint8_t* src, uint64_t size, uint32_t k, uint32_t group, const uint8_t* base, uint8_t* dst, uint32_t* trace, uint64_t cap,
                                   uint64_t* traceWords, uint64_t* info, char* text)
{
    EmuTypedBackend b;
    const int rc = which == 0 ? zsk_planes_split_base(b, true, src, size, k, group, base, dst) : zsk_planes_join_base(b, true, src, size, k, group, base, dst);
    *traceWords = copy_trace(b.trace, trace, (size_t)cap);
    info[0] = b.typed[ZSKT_A_TILESUMS].bytes;
    if (text) snprintf(text, 256, "%s", b.text.c_str());
    return rc;
}
// emu_delta_compress with a base
extern "C" int emu_xor_compress(const uint8_t* src, const uint8_t* base, uint64_t srcSize, uint32_t frameSize, uint32_t k, uint32_t checksum, const uint8_t* frames,
                                const uint64_t* frameOffs, uint8_t* dst, uint64_t dstCapacity, int32_t* outStatus, uint8_t* stagingOut, uint64_t* info, uint32_t* trace, uint64_t cap,
                                uint64_t* traceWords, char* text)
{
    memset(info, 0, 4 * sizeof(uint64_t));
    EmuTypedBackend b; b.frames = frames; b.frameOffs = frameOffs; b.srcSize = srcSize;
    uint64_t streamSize = ~0ull;
    const int rc = zsk_typed_compress_base(b, true, src, srcSize, frameSize, k, base, checksum ? ZHIP_SEEKABLE_CHECKSUM : 0, dst, dstCapacity, &streamSize, outStatus);
    *traceWords = copy_trace(b.trace, trace, (size_t)cap);
    if (text) snprintf(text, 256, "%s", b.text.c_str());
    if (rc) return rc;
    info[0] = streamSize; info[1] = b.refused; info[2] = b.typed[ZSKT_A_STAGING].bytes;
    if (stagingOut && srcSize) memcpy(stagingOut, b.typed[ZSKT_A_STAGING].p.get(), (size_t)srcSize);
    return 0;
}
// the read plan under `filter` (-1: the opened stream's): emu_delta_plan's outputs, and contentOut [cap] = the jobs' content offsets; counts[3] = how many
// of them the plan holds (0 but under the xor-with-base filter); layout[5] = the upload's offsets and bytes (jobs, owner, pairAt, content, all)
extern "C" int emu_xor_plan(const uint8_t* stream, uint64_t size, const uint64_t* rg, uint64_t R, uint64_t limit, int64_t filter, uint64_t cap, uint64_t* planarOut, uint64_t* jobsOut,
                            uint64_t* passOut, uint64_t* ownerOut, uint64_t* contentOut, uint64_t* counts, uint64_t* layout)
{
    TypedOpened o; size_t index = 0;
    if (int e = open_typed(stream, size, &o, &index)) return e;
    if (o.elementSize == 1) return -2;
    ZskTypedPlan plan;
    zsk_typed_plan(o.dOff.data(), o.elementSize, o.groupElements, rg, (size_t)R, limit, &plan, filter < 0 ? o.filter : (uint32_t)filter);
    counts[0] = plan.planar.size() / 3; counts[1] = plan.jobs.size(); counts[2] = plan.passes.size(); counts[3] = plan.content.size();
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
    for (size_t j = 0; j < plan.content.size(); j++) contentOut[j] = plan.content[j];
    const ZskTypedReadLayout l = zsk_typed_read_layout(plan.jobs.size(), (size_t)R, plan.planar.size() / 3, plan.content.size());
    layout[0] = l.oJobs; layout[1] = l.oOwner; layout[2] = l.oPairAt; layout[3] = l.oContent; layout[4] = l.tableBytes;
    return 0;
}
// emu_typed_ranges with a base of baseSize bytes; trace [cap]: what was launched
extern "C" int emu_xor_ranges(const uint8_t* stream, uint64_t size, const uint8_t* content, const uint8_t* base, uint64_t baseSize, const uint64_t* rg, uint64_t R, uint8_t* dst,
                              uint64_t dstCapacity, uint64_t limit, int64_t codeFrame, int32_t code, int32_t* outStatus, uint64_t* stats, uint32_t* trace, uint64_t cap, uint64_t* traceWords,
                              char* text)
{
    TypedOpened o; size_t index = 0;
    if (int e = open_typed(stream, size, &o, &index)) return e;
    memset(stats, 0, 7 * sizeof(uint64_t));
    o.scratchLimit = limit;
    EmuTypedBackend& b = o.b; b.content = content; b.codeFrame = codeFrame; b.code = code;
    zhip_seekable_gather_stats g; memset(&g, 0, sizeof g);
    size_t bad = 0;
    const int rc = zsk_typed_ranges_base(b, true, &o, base, baseSize, rg, (size_t)R, dst, dstCapacity, outStatus, &g, &bad);
    *traceWords = copy_trace(b.trace, trace, (size_t)cap);
    if (text) snprintf(text, 256, "%s", b.text.c_str());
    stats[0] = g.items; stats[1] = g.inPlace; stats[2] = g.scratchBytes; stats[3] = g.copyJobs; stats[4] = g.passes; stats[5] = b.typed[ZSKT_A_PLANAR].bytes; stats[6] = bad;
    return rc;
}
// The REFUSALS, through the calls themselves. which 0 = typed compress with a base, 1 = the split with a base, 2 = the join with a base; 3, 4, 5 = the same
// three through their filter argument (filter 4, no base to take). baseMode 0: NULL, 1: a buffer of its own, 2: one that shares the destination's last byte.
// *traceWords: what was launched (nothing may be); -9 where the call wrote a byte of the destination, the stream size or the status
extern "C" int emu_xor_check(int which, uint64_t size, uint32_t frameSize, uint32_t k, int baseMode, uint64_t* traceWords, char* text)
{
    EmuTypedBackend b; b.srcSize = size;
    const size_t dstBytes = (size_t)zsk_bound(size, frameSize ? frameSize : 1, 1) + 256;
    std::vector<uint8_t> src((size_t)size + 1), own((size_t)size + 1), dst(dstBytes + (size_t)size, 0x5A);      // (the overlapping base begins at the destination's last byte)
    const uint8_t* base = baseMode == 0 ? nullptr : baseMode == 1 ? own.data() : dst.data() + dstBytes - 1;
    uint64_t streamSize = 0x5A5A5A5A5A5A5A5Aull; int32_t status[2] = {-1, -1};
    int rc;
    if (which == 0) rc = zsk_typed_compress_base(b, true, src.data(), size, frameSize, k, base, 0, dst.data(), dstBytes, &streamSize, status);
    else if (which == 1) rc = zsk_planes_split_base(b, true, src.data(), size, k, frameSize, base, dst.data() + dstBytes - size);
    else if (which == 2) rc = zsk_planes_join_base(b, true, src.data(), size, k, frameSize, base, dst.data() + dstBytes - size);
    else if (which == 3) rc = zsk_typed_compress(b, true, src.data(), size, frameSize, k, 0, dst.data(), dstBytes, &streamSize, status, ZSK_FILTER_XOR_BASE);
    else if (which == 4) rc = zsk_planes_split(b, true, src.data(), size, k, frameSize, dst.data(), ZSK_FILTER_XOR_BASE);
    else rc = zsk_planes_join(b, true, src.data(), size, k, frameSize, dst.data(), ZSK_FILTER_XOR_BASE);
    *traceWords = b.trace.size();
    for (uint8_t x : dst) if (x != 0x5A) return -9;
    if (streamSize != 0x5A5A5A5A5A5A5A5Aull || status[0] != -1 || status[1] != -1) return -9;
    snprintf(text, 256, "%s", b.text.c_str());
    return rc;
}
