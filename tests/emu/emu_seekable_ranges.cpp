// tests/emu/emu_seekable_ranges.cpp -- the many-ranges read (zhip_seekable_decompress_ranges_device) on the host wave emulator: the library's own checks and plan
// (zsk_gather_check, zsk_gather_plan) and the bodies of its three kernels, launched pass by pass as the library launches them. Test infrastructure only
// (tests/test_emu_seekable_ranges.py, built by tests/seekable_range_cases.py). The decoder is replaced by a copy from the content the test says the stream holds.
// With -DZSK_RANGES_MAIN this is a stand-alone program that runs the cases of a file (see main) -- the form the sanitizer build takes.
#include "emu_seekable.cpp"     // open_stream, the backend
#include <stdio.h>

static void put_stats(const ZskGatherPlan& plan, uint64_t* stats)
{
    stats[0] = plan.items; stats[1] = plan.inPlace; stats[2] = plan.scratchBytes; stats[3] = plan.jobs.size(); stats[4] = plan.passes.size();
    stats[5] = plan.segs.size(); stats[6] = plan.scratchMax;
}

// the checks and the plan alone. rg = [R][3]. Returns 0, the library's code for a rejected call (stats[7] = the range's index) or the open's error code.
// stats[8] = items, inPlace, scratchBytes, copyJobs, passes, segments, scratchMax, -; segsOut [segCap][6] = first, frames, item, home, inPlace, pass;
// jobsOut [jobCap][4] = pass, src, dst, bytes; passOut [passCap][4] = scratch, item0, item1, tiles; rangeOut [R][2] = f0, f1
extern "C" int emu_gather_plan(const uint8_t* stream, uint64_t size, const uint64_t* rg, uint64_t R, uint64_t dstCapacity, uint64_t limit, uint64_t* stats,
                               uint64_t* segsOut, uint64_t segCap, uint64_t* jobsOut, uint64_t jobCap, uint64_t* passOut, uint64_t passCap, uint64_t* rangeOut)
{
    Opened o;
    if (int e = open_stream(stream, size, &o)) return e;
    size_t bad = 0; bool any = false;
    memset(stats, 0, 8 * sizeof(uint64_t));
    if (const int rc = zsk_ranges_check(true, rg, (size_t)R, o.contentSize, stream, dstCapacity, &bad, &any, o.b.err)) { stats[7] = bad; return rc; }
    ZskGatherPlan plan;
    zsk_gather_plan(o.dOff.data(), o.place.data(), o.lay.n, rg, (size_t)R, limit, &plan);
    put_stats(plan, stats);
    if (plan.segs.size() > segCap || plan.jobs.size() > jobCap || plan.passes.size() > passCap) return -3;
    for (size_t s = 0; s < plan.segs.size(); s++) {
        const ZskGatherSeg& x = plan.segs[s];
        uint64_t* q = segsOut + 6 * s; q[0] = x.first; q[1] = x.frames; q[2] = x.item; q[3] = x.home; q[4] = x.inPlace; q[5] = x.pass;
    }
    for (size_t p = 0; p < plan.passes.size(); p++) {
        const ZskGatherPass& x = plan.passes[p];
        uint64_t* q = passOut + 4 * p; q[0] = x.scratch; q[1] = x.item0; q[2] = x.item1; q[3] = x.tiles;
        for (uint32_t j = x.job0; j < x.job1; j++) { uint64_t* w = jobsOut + 4 * j; w[0] = p; w[1] = plan.jobs[j].src; w[2] = plan.jobs[j].dst; w[3] = plan.jobs[j].bytes; }
    }
    for (size_t r = 0; r < (size_t)R; r++) { rangeOut[2 * r] = plan.ranges[r].f0; rangeOut[2 * r + 1] = plan.ranges[r].f1; }
    return 0;
}

// The whole call. Frame f "decodes" to content[dOff[f], dOff[f + 1]), except frame shortFrame (-1: none), which comes out one byte short, and frame codeFrame
// (-1: none), for which the decoder reports `code` and writes nothing. dst has dstCapacity bytes. Returns 0, the library's code (rejected: nothing written), the
// open's error code, or a negative number where a segment lies outside its buffer. outStatus [2 + 2R]; stats as emu_gather_plan, from what the library's call
// reports and what the backend was asked to reserve; itemsOut (where given) [itemCap][5] = frame, 0 (d_dst) / 1 (scratch), offset there, length, pass.
extern "C" int emu_gather_run(const uint8_t* stream, uint64_t size, const uint8_t* content, const uint64_t* rg, uint64_t R, uint8_t* dst, uint64_t dstCapacity, uint64_t limit,
                              int64_t shortFrame, int64_t codeFrame, int32_t code, int32_t* outStatus, uint64_t* stats, uint64_t* itemsOut, uint64_t itemCap)
{
    Opened o;
    if (int e = open_stream(stream, size, &o)) return e;
    memset(stats, 0, 8 * sizeof(uint64_t));
    o.scratchLimit = limit;
    EmuBackend& b = o.b; b.content = content; b.shortFrame = shortFrame; b.codeFrame = codeFrame; b.code = code; b.dst = dst; b.dstBytes = dstCapacity; b.itemsOut = itemsOut; b.itemCap = itemCap;
    zhip_seekable_gather_stats g; memset(&g, 0, sizeof g);
    size_t bad = 0;
    const int rc = zsk_ranges(b, true, &o, rg, (size_t)R, dst, dstCapacity, outStatus, &g, &bad);
    if (rc > 0) stats[7] = bad;
    stats[0] = g.items; stats[1] = g.inPlace; stats[2] = g.scratchBytes; stats[3] = g.copyJobs; stats[4] = g.passes;
    if (g.passes) { stats[5] = b.areas[ZSK_A_G_TABLES].bytes / 32 - R - g.copyJobs; stats[6] = b.areas[ZSK_A_G_SCRATCH].bytes; }
    return rc;
}

#ifdef ZSK_RANGES_MAIN
// emu_seekable_ranges <file>: the cases of the file, each {u64 streamSize, stream, u64 contentSize, content, u64 R, ranges [R][3], u64 dstCapacity, u64 limit}
// (little-endian, back to back), through the plan and the emulated kernels into buffers of exactly the sizes the call is given. Exit 0: every range of every
// case holds its content's bytes and every status is 0.
static bool rd(FILE* f, void* p, size_t n) { return !n || fread(p, 1, n, f) == n; }
int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s <cases>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int cases = 0;
    for (uint64_t streamSize; fread(&streamSize, 8, 1, f) == 1; cases++) {
        uint64_t contentSize = 0, R = 0, tail[2] = {0, 0};
        std::vector<uint8_t> stream((size_t)streamSize);
        if (!rd(f, stream.data(), stream.size()) || !rd(f, &contentSize, 8)) return 2;
        std::vector<uint8_t> content((size_t)contentSize);
        if (!rd(f, content.data(), content.size()) || !rd(f, &R, 8)) return 2;
        std::vector<uint64_t> rg(3 * (size_t)R);
        if (!rd(f, rg.data(), rg.size() * 8) || !rd(f, tail, 16)) return 2;
        std::vector<uint8_t> dst((size_t)tail[0], 0x5A);
        std::vector<int32_t> status(2 + 2 * (size_t)R, -1);
        uint64_t stats[8];
        const int rc = emu_gather_run(stream.data(), streamSize, content.data(), rg.data(), R, dst.data(), tail[0], tail[1], -1, -1, 0, status.data(), stats, nullptr, 0);
        if (rc) { fprintf(stderr, "case %d: the call returned %d\n", cases, rc); return 1; }
        for (int32_t s : status) if (s) { fprintf(stderr, "case %d: a status is %d\n", cases, s); return 1; }
        for (size_t r = 0; r < (size_t)R; r++)
            if (rg[3 * r + 1] && memcmp(dst.data() + rg[3 * r + 2], content.data() + rg[3 * r], (size_t)rg[3 * r + 1])) { fprintf(stderr, "case %d: range %zu differs\n", cases, r); return 1; }
    }
    fclose(f);
    printf("%d cases\n", cases);
    return cases ? 0 : 2;
}
#endif
