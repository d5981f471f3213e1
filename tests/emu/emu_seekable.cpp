// tests/emu/emu_seekable.cpp -- the seekable-stream kernels (python-zstandard_amd/csrc/zhip_seekable.hpp) on the host wave emulator.
// Test infrastructure only (tests/test_emu_seekable.py); compiled with zhemu.cpp like emu_greedy_row.cpp. Every function launches the kernels' bodies in the
// grids the library launches them in (zsk_scan_shape) and makes the library's host-side decisions with the library's own functions.
#define ZHIP_EMU 1
#include <stdint.h>
#include "../../python-zstandard_amd/csrc/zhip_seekable.hpp"
#include <string.h>
#include <algorithm>
#include <vector>

static void scan_reduce_lane(void* p) { zsk_scan_reduce_body(*(const ZskScanArgs*)p); }
static void scan_write_lane(void* p) { zsk_scan_write_body(*(const ZskScanArgs*)p); }
static void chunk_segs_lane(void* p) { zsk_chunk_segs_body(*(const ZskCompressArgs*)p); }
static void verdict_lane(void* p) { zsk_verdict_body(*(const ZskCompressArgs*)p); }
static void table_lane(void* p) { zsk_table_body(*(const ZskCompressArgs*)p); }
static void range_segs_lane(void* p) { zsk_range_segs_body(*(const ZskRangeArgs*)p); }
static void range_verify_lane(void* p) { zsk_range_verify_body(*(const ZskRangeArgs*)p); }
static void range_finish_lane(void* p) { zsk_range_finish_body(*(const ZskRangeArgs*)p); }

static uint32_t lane_grid(uint64_t lanes) { const uint64_t w = (lanes + 63) / 64; return (uint32_t)(w < 1 ? 1 : w < 8 ? w : 8); }
// both launches of the scan; returns the lowest bad item (ZSK_NONE: none)
static uint64_t run_scan(ZskScanArgs s)
{
    const uint32_t grid = zsk_scan_shape(s.n, &s.span);
    std::vector<uint64_t> sum(grid, 0xA5A5A5A5A5A5A5A5ull), bad(grid, 0xA5A5A5A5A5A5A5A5ull);
    s.partSum = sum.data(); s.partBad = bad.data();
    zhemu::run_grid(grid, scan_reduce_lane, &s);
    zhemu::run_grid(grid, scan_write_lane, &s);
    return *std::min_element(bad.begin(), bad.end());
}

// the kernel's own tile sizes: lanes per workgroup, items per workgroup, items of one full grid pass
extern "C" void emu_seekable_tiles(uint32_t* out) { out[0] = ZSK_SCAN_LANES; out[1] = ZSK_SCAN_TILE; out[2] = ZSK_SCAN_GRID * ZSK_SCAN_TILE; }

// mode 0 (what the compress call runs): offs has n + 1 cells, the last one receives the total
extern "C" uint64_t emu_seekable_scan(const uint64_t* sizes, const int32_t* status, uint32_t n, uint64_t* offs)
{
    ZskScanArgs s; memset(&s, 0, sizeof s);
    s.in = (const uint8_t*)sizes; s.status = status; s.mode = 0; s.n = n; s.offs = offs;
    return run_scan(s);
}

// the compress call behind zhip_compress_batch_device: outSizes / status are given, the frames' bytes are not written (the compaction is zhip_lib.hip's kernel).
// dst holds dstCapacity bytes; srcSegs / slotSegs [n][2] receive the chunk segments. Returns the stream size (0: failed), outStatus[2] the status.
extern "C" uint64_t emu_seekable_table(const uint8_t* src, uint64_t srcSize, uint32_t frameSize, uint32_t checksum, const uint64_t* outSizes, int32_t* status,
                                       uint8_t* dst, uint64_t dstCapacity, uint64_t* srcSegs, uint64_t* slotSegs, int32_t* outStatus)
{
    if (!zsk_args_ok(srcSize, frameSize)) return 0;
    const uint32_t n = (uint32_t)zsk_frame_count(srcSize, frameSize);
    std::vector<uint64_t> offs((size_t)n + 1, 0xA5A5A5A5A5A5A5A5ull);
    uint64_t streamSize = ~0ull; uint32_t go = 7;
    ZskCompressArgs a; memset(&a, 0, sizeof a);
    a.src = src; a.srcSize = srcSize; a.frameSize = frameSize; a.n = n; a.checksum = checksum;
    a.srcSegs = srcSegs; a.slotSegs = slotSegs; a.outSizes = outSizes; a.status = status; a.offs = offs.data();
    a.dst = dst; a.dstCapacity = dstCapacity; a.streamSize = &streamSize; a.outStatus = outStatus; a.go = &go;
    if (n) zhemu::run_grid(lane_grid(n), chunk_segs_lane, &a);
    ZskScanArgs s; memset(&s, 0, sizeof s);
    s.in = (const uint8_t*)outSizes; s.status = status; s.mode = 0; s.n = n; s.offs = offs.data();
    a.nPart = zsk_scan_shape(n, &s.span);
    std::vector<uint64_t> sum(a.nPart), bad(a.nPart);
    s.partSum = sum.data(); s.partBad = bad.data(); a.partBad = bad.data();
    zhemu::run_grid(a.nPart, scan_reduce_lane, &s);
    zhemu::run_grid(a.nPart, scan_write_lane, &s);
    zhemu::run_grid(1, verdict_lane, &a);
    zhemu::run_grid(lane_grid(n), table_lane, &a);
    return streamSize;
}

// zhip_seekable_open_device's checks on a stream in host memory. Returns 0 or the zstd error code; on success info = {n, entry size, checksum flag,
// table offset, content size} and, where given, cOff / dOff / place receive the n + 1 cells of the three scans.
struct Opened { ZskLayout lay; std::vector<uint64_t> cOff, dOff, place; };
static int open_stream(const uint8_t* stream, uint64_t size, Opened* o)
{
    if (size < ZSK_HEADER + ZSK_FOOTER) return ZSK_ERR_CORRUPT;
    uint8_t foot[ZSK_FOOTER], head[ZSK_HEADER];
    memcpy(foot, stream + size - ZSK_FOOTER, ZSK_FOOTER);
    if (int e = zsk_parse_footer(foot, size, &o->lay)) return e;
    memcpy(head, stream + o->lay.tableOffset, ZSK_HEADER);
    if (int e = zsk_check_header(head, &o->lay)) return e;
    const uint32_t n = o->lay.n;
    const uint8_t* const entries = stream + o->lay.tableOffset + ZSK_HEADER;
    o->cOff.assign((size_t)n + 1, 0); o->dOff.assign((size_t)n + 1, 0); o->place.assign((size_t)n + 1, 0);
    uint64_t lowestBad = ZSK_NONE;
    for (int k = 0; k < 3; k++) {
        ZskScanArgs s; memset(&s, 0, sizeof s);
        s.in = entries + (k ? 4 : 0); s.stride = o->lay.entry; s.mode = k == 2 ? 2u : 1u; s.limit = k == 1 ? ZSK_MAX_CONTENT : 0xFFFFFFFFu; s.n = n;
        s.offs = k == 0 ? o->cOff.data() : k == 1 ? o->dOff.data() : o->place.data();
        const uint64_t bad = run_scan(s);
        if (k == 1) lowestBad = bad;
    }
    return zsk_table_verdict(lowestBad, o->cOff[n], &o->lay);
}
extern "C" int emu_seekable_validate(const uint8_t* stream, uint64_t size, uint64_t* info, uint64_t* cOff, uint64_t* dOff, uint64_t* place)
{
    Opened o;
    const int e = open_stream(stream, size, &o);
    if (e) return e;
    const size_t n = o.lay.n;
    if (info) { info[0] = n; info[1] = o.lay.entry; info[2] = (uint64_t)o.lay.checksum; info[3] = o.lay.tableOffset; info[4] = o.dOff[n]; }
    if (cOff) memcpy(cOff, o.cOff.data(), (n + 1) * 8);
    if (dOff) memcpy(dOff, o.dOff.data(), (n + 1) * 8);
    if (place) memcpy(place, o.place.data(), (n + 1) * 8);
    return 0;
}

// zhip_seekable_decompress_device with the decoder replaced by a copy: frame f "decodes" to content[dOff[f], dOff[f + 1]) -- `content` is what the test says the
// stream holds -- except frame `shortFrame` (-1: none), which comes out one byte short. dst has `length` bytes. Returns 0, 3 (ZHIP_ERR_SIZE_MISMATCH: the range
// is outside the content) or the open's error code; outStatus[2] the range's status; segsOut (where given) [count][4] = srcSeg, dstSeg relative to dst or, for
// a frame in the edge buffer, 2^63 + its offset there.
extern "C" int emu_seekable_range(const uint8_t* stream, uint64_t size, const uint8_t* content, uint64_t offset, uint64_t length, uint8_t* dst, int64_t shortFrame,
                                  int32_t* outStatus, uint64_t* segsOut, uint32_t* countOut)
{
    Opened o;
    if (int e = open_stream(stream, size, &o)) return e;
    const std::vector<uint64_t>& D = o.dOff;
    const uint64_t end = offset + length;
    if (countOut) *countOut = 0;
    if (end < offset || end > D[o.lay.n]) return 3;
    if (!length) { outStatus[0] = outStatus[1] = 0; return 0; }
    const uint32_t f0 = (uint32_t)(std::upper_bound(D.begin(), D.end(), offset) - D.begin() - 1), f1 = (uint32_t)(std::upper_bound(D.begin(), D.end(), end - 1) - D.begin() - 1);
    const size_t count = (size_t)(o.place[f1 + 1] - o.place[f0]);
    const bool cut0 = D[f0] < offset || D[f0 + 1] > end, cut1 = f1 != f0 && D[f1 + 1] > end;
    const size_t edgeBytes = (size_t)((cut0 ? D[f0 + 1] - D[f0] : 0) + (cut1 ? D[f1 + 1] - D[f1] : 0));
    std::vector<uint8_t> edge(edgeBytes + 1, 0xEE);
    std::vector<uint64_t> srcSegs(2 * count, ~0ull), dstSegs(2 * count, ~0ull), outSizes(count, 0);
    std::vector<uint32_t> frameOf(count, ~0u); std::vector<int32_t> status(count, -1);
    uint32_t worst = 0;
    ZskRangeArgs a; memset(&a, 0, sizeof a);
    a.cOff = o.cOff.data(); a.dOff = o.dOff.data(); a.place = o.place.data();
    a.table = stream + o.lay.tableOffset + ZSK_HEADER; a.entry = o.lay.entry; a.checksum = (uint32_t)o.lay.checksum;
    a.f0 = f0; a.f1 = f1; a.count = (uint32_t)count; a.offset = offset; a.length = length;
    a.dst = dst; a.edge = edgeBytes ? edge.data() : dst; a.dstBase = a.edge < a.dst ? a.edge : a.dst;
    a.srcSegs = srcSegs.data(); a.dstSegs = dstSegs.data(); a.frameOf = frameOf.data(); a.outSizes = outSizes.data(); a.status = status.data(); a.worst = &worst; a.outStatus = outStatus;
    zhemu::run_grid(lane_grid((uint64_t)f1 - f0 + 1), range_segs_lane, &a);
    for (size_t k = 0; k < count; k++) {                                   // the stand-in for the decoder
        const uint32_t f = frameOf[k];
        uint8_t* const home = a.dstBase + dstSegs[2 * k];
        const bool inDst = home >= dst && home + dstSegs[2 * k + 1] <= dst + length, inEdge = home >= edge.data() && home + dstSegs[2 * k + 1] <= edge.data() + edgeBytes;
        if (f > f1 || f < f0 || !(inDst || inEdge) || srcSegs[2 * k] + srcSegs[2 * k + 1] > o.lay.tableOffset || dstSegs[2 * k + 1] != D[f + 1] - D[f]) return -1;      // a segment outside its buffer
        const uint64_t out = dstSegs[2 * k + 1] - ((int64_t)f == shortFrame ? 1 : 0);
        memcpy(home, content + D[f], out);
        outSizes[k] = out; status[k] = 0;
        if (segsOut) { segsOut[4 * k] = srcSegs[2 * k]; segsOut[4 * k + 1] = srcSegs[2 * k + 1]; segsOut[4 * k + 2] = inDst ? (uint64_t)(home - dst) : (1ull << 63) + (uint64_t)(home - edge.data()); segsOut[4 * k + 3] = dstSegs[2 * k + 1]; }
    }
    if (countOut) *countOut = (uint32_t)count;
    zhemu::run_grid(lane_grid(count), range_verify_lane, &a);
    zhemu::run_grid(lane_grid(edgeBytes / 16 + 1), range_finish_lane, &a);
    return edge[edgeBytes] == 0xEE ? 0 : -2;
}

extern "C" uint64_t emu_seekable_bound(uint64_t srcSize, uint32_t frameSize, int checksum) { return zsk_bound(srcSize, frameSize, checksum); }
extern "C" uint64_t emu_seekable_xxh64(const uint8_t* p, uint32_t n) { return ze_xxh64(p, n); }
