// tests/emu/emu_host_calls.cpp -- the plan of the host-buffer batch calls (python-zstandard_amd/csrc/zhip_host_calls.hpp) behind flat C entries.
// Test infrastructure only (tests/test_emu_host_calls.py); part of libzhip_emu.so. The plan is plain host code: nothing is emulated here.
// The entries up to emu_hc_merge are the ones tests/golden/host_calls.json was recorded through, from a library that held the parent commit's lines behind them.
#include "../../python-zstandard_amd/csrc/zhip_host_calls.hpp"
#include <stdio.h>

static std::vector<zhip_segment> table(const uint64_t* inLen, const uint64_t* outLen, size_t n)      // [0,n) source, [n,2n) destination, both back to back
{
    std::vector<zhip_segment> segs(2 * n + 1);
    uint64_t a = 0, b = 0;
    for (size_t i = 0; i < n; i++) { segs[i] = {a, inLen[i]}; a += inLen[i]; segs[n + i] = {b, outLen ? outLen[i] : 0}; b += outLen ? outLen[i] : 0; }
    return segs;
}
// cuts of host_chunks -> out (at most cap); returns how many
extern "C" uint64_t emu_hc_chunks(const uint64_t* inLen, const uint64_t* outLen, uint64_t n, uint64_t maxBytes, uint64_t maxItems, uint64_t firstItems, uint64_t* out, uint64_t cap)
{
    const std::vector<zhip_segment> segs = table(inLen, outLen, (size_t)n);
    const std::vector<size_t> cut = host_chunks(segs.data(), (size_t)n, maxBytes, (size_t)maxItems, (size_t)firstItems);
    for (size_t i = 0; i < cut.size() && i < cap; i++) out[i] = cut[i];
    return cut.size();
}
// the upload steps of items [lo, hi): out = (a, b, bytes) per step; returns the steps
extern "C" uint64_t emu_hc_upload_steps(const uint64_t* len, uint64_t n, uint64_t lo, uint64_t hi, uint64_t stageBytes, uint64_t* out, uint64_t cap)
{
    const std::vector<zhip_segment> segs = table(len, nullptr, (size_t)n);
    uint64_t k = 0;
    for (size_t a = (size_t)lo; a < hi; k++) {
        const HostStep st = host_upload_step(segs.data(), a, (size_t)hi, stageBytes);
        if (k < cap) { out[3 * k] = st.a; out[3 * k + 1] = st.b; out[3 * k + 2] = st.bytes; }
        a = st.b;
    }
    return k;
}
// the packing runs of items [lo, hi): out = (a, b) per run; returns the runs
extern "C" uint64_t emu_hc_pack_split(const uint64_t* len, uint64_t n, uint64_t lo, uint64_t hi, uint64_t threshold, uint32_t threads, uint64_t* out, uint64_t cap)
{
    const std::vector<zhip_segment> segs = table(len, nullptr, (size_t)n);
    const std::vector<size_t> cut = host_pack_split(segs.data(), (size_t)lo, (size_t)hi, threshold, threads);
    for (size_t t = 0; t + 1 < cut.size() && t < cap; t++) { out[2 * t] = cut[t]; out[2 * t + 1] = cut[t + 1]; }
    return cut.size() - 1;
}
// bytes reserved for a call's meta areas: out = device, pinned. dir 0 decompress, 1 compress
extern "C" void emu_hc_layout_bytes(int dir, uint64_t n, uint64_t nChunks, uint64_t* out)
{
    if (dir) { const HostCompressLayout l = host_compress_layout((size_t)n, (size_t)nChunks); out[0] = l.dBytes; out[1] = l.hBytes; }
    else { const HostDecompressLayout l = host_decompress_layout((size_t)n); out[0] = l.dBytes; out[1] = l.hBytes; }
}
extern "C" uint64_t emu_hc_slots_for(uint64_t slots, int explicitList, uint64_t minBytes, uint64_t n, uint64_t bytes) { return host_slots_for((size_t)slots, explicitList != 0, minBytes, (size_t)n, bytes); }
extern "C" int emu_hc_parse_devices(const char* list, int count, int* out, int cap)
{
    const std::vector<int> s = host_parse_devices(list, count);
    for (size_t i = 0; i < s.size() && (int)i < cap; i++) out[i] = s[i];
    return (int)s.size();
}
// the fan-out's merge over runs that begin at lo[w] and returned rc[w] with the error index errIndex[w]: out = the failing run (`used`: none), its code, the index reported
extern "C" void emu_hc_merge(const int* rc, const uint64_t* lo, const uint64_t* errIndex, uint64_t used, uint64_t* out)
{
    std::vector<HostRun> runs((size_t)used);
    for (size_t w = 0; w < used; w++) { runs[w].lo = (size_t)lo[w]; runs[w].rc = rc[w]; memset(&runs[w].err, 0, sizeof runs[w].err); runs[w].err.kind = rc[w]; runs[w].err.index = (size_t)errIndex[w]; }
    zhip_error err; memset(&err, 0, sizeof err);
    const size_t bad = host_merge_failing(runs.data(), (size_t)used, &err);
    out[0] = bad; out[1] = bad < used ? (uint64_t)runs[bad].rc : 0; out[2] = err.index;
}
extern "C" uint64_t emu_hc_partition(const uint64_t* sizes, uint64_t n, uint64_t workers, uint64_t* bounds)
{
    std::vector<size_t> b(2 * (size_t)(workers ? workers : 1));
    const size_t used = host_partition_by_bytes(sizes, (size_t)n, (size_t)workers, b.data());
    for (size_t i = 0; i < 2 * used; i++) bounds[i] = b[i];
    return used;
}

// ---- frame inspection
extern "C" uint64_t emu_hc_content_size(const uint8_t* src, uint64_t n, int format) { return host_frame_content_size(src, (size_t)n, format); }
extern "C" int64_t emu_hc_frame_size(const uint8_t* src, uint64_t n, int format) { return host_frame_compressed_size(src, (size_t)n, format); }
extern "C" uint32_t emu_hc_count_blocks(const uint8_t* src, uint64_t n, int format) { return host_count_blocks(src, (size_t)n, format); }
// the walker from `pos`: out = blocks, end, stop
extern "C" void emu_hc_walk(const uint8_t* src, uint64_t n, uint64_t pos, uint64_t* out)
{
    const HostBlockWalk w = host_walk_blocks(src, (size_t)n, (size_t)pos);
    out[0] = w.nBlocks; out[1] = w.end; out[2] = (uint64_t)w.stop;
}

// ---- pass 1. Item i: srcSize[i] bytes at blob + off[i] (blob NULL: no bytes are there to read -- the sizes alone decide), dstSize[i].
// out: kind, index, srcTotal, dstTotal; segs as (offset, length) pairs, 2n of them
static std::vector<zhip_item> items_of(const uint8_t* blob, const uint64_t* off, const uint64_t* srcSize, const uint64_t* dstSize, size_t n)
{
    std::vector<zhip_item> it(n + 1);
    for (size_t i = 0; i < n; i++) { it[i].src = blob ? blob + off[i] : nullptr; it[i].srcSize = (size_t)srcSize[i]; it[i].dstSize = dstSize ? (size_t)dstSize[i] : 0; }
    return it;
}
extern "C" void emu_hc_decompress_segments(const uint8_t* blob, const uint64_t* off, const uint64_t* srcSize, const uint64_t* dstSize, uint64_t n, int format, uint64_t* segs, uint32_t* nBlocks, uint64_t* out)
{
    const std::vector<zhip_item> it = items_of(blob, off, srcSize, dstSize, (size_t)n);
    std::vector<zhip_segment> s(2 * (size_t)n + 1);
    uint64_t st = 0, dt = 0;
    const HostRefusal r = host_decompress_segments(it.data(), (size_t)n, format, s.data(), nBlocks, &st, &dt);
    out[0] = (uint64_t)r.kind; out[1] = r.index; out[2] = st; out[3] = dt;
    for (size_t i = 0; i < 2 * n; i++) { segs[2 * i] = s[i].offset; segs[2 * i + 1] = s[i].length; }
}
extern "C" void emu_hc_compress_segments(const uint64_t* srcSize, uint64_t n, uint64_t* segs, uint64_t* out, char* text, uint64_t cap)
{
    const std::vector<zhip_item> it = items_of(nullptr, nullptr, srcSize, nullptr, (size_t)n);
    std::vector<zhip_segment> s(2 * (size_t)n + 1);
    uint64_t st = 0, dt = 0;
    const HostRefusal r = host_compress_segments(it.data(), (size_t)n, s.data(), &st, &dt);
    out[0] = (uint64_t)r.kind; out[1] = r.index; out[2] = st; out[3] = dt;
    snprintf(text, (size_t)cap, "%s", r.text ? r.text : "");
    for (size_t i = 0; i < 2 * n; i++) { segs[2 * i] = s[i].offset; segs[2 * i + 1] = s[i].length; }
}
extern "C" uint64_t emu_hc_compress_bound(uint64_t n) { return host_compress_bound((size_t)n); }

// ---- the meta layouts' offsets: decompress dSizes dStatus dBytes hSizes hStatus hBytes; compress dSizes dOffs dTotals dStatus dBytes hSizes hTotals hStatus hBytes
extern "C" int emu_hc_layout(int dir, uint64_t n, uint64_t nChunks, uint64_t* out)
{
    if (dir) {
        const HostCompressLayout l = host_compress_layout((size_t)n, (size_t)nChunks);
        const size_t v[] = {l.dSizes, l.dOffs, l.dTotals, l.dStatus, l.dBytes, l.hSizes, l.hTotals, l.hStatus, l.hBytes};
        for (int i = 0; i < 9; i++) out[i] = v[i];
        return 9;
    }
    const HostDecompressLayout l = host_decompress_layout((size_t)n);
    const size_t v[] = {l.dSizes, l.dStatus, l.dBytes, l.hSizes, l.hStatus, l.hBytes};
    for (int i = 0; i < 6; i++) out[i] = v[i];
    return 6;
}

// ---- verdicts over items [lo, hi). out: kind, index, zerr, d0, d1 (compress: then the frames' bytes); segs as (offset, length) pairs, hi - lo of them
extern "C" void emu_hc_decompress_verdict(const uint64_t* dstLen, const uint64_t* sizes, const int32_t* status, uint64_t n, uint64_t lo, uint64_t hi, int allowShort, uint64_t* segs, uint64_t* out)
{
    const std::vector<zhip_segment> t = table(dstLen, dstLen, (size_t)n);
    std::vector<zhip_segment> o((size_t)(hi - lo) + 1);
    const HostVerdict v = host_decompress_verdict(t.data() + n, sizes, status, (size_t)lo, (size_t)hi, allowShort != 0, o.data());
    out[0] = (uint64_t)v.kind; out[1] = v.index; out[2] = (uint64_t)(int64_t)v.zerr; out[3] = v.d0; out[4] = v.d1;
    for (size_t i = 0; i < hi - lo; i++) { segs[2 * i] = o[i].offset; segs[2 * i + 1] = o[i].length; }
}
extern "C" void emu_hc_compress_verdict(const uint64_t* sizes, const int32_t* status, uint64_t lo, uint64_t hi, uint64_t* segs, uint64_t* out)
{
    std::vector<zhip_segment> o((size_t)(hi - lo) + 1);
    const HostVerdict v = host_compress_verdict(status, (size_t)lo, (size_t)hi);
    out[0] = (uint64_t)v.kind; out[1] = v.index; out[2] = (uint64_t)(int64_t)v.zerr; out[3] = v.d0; out[4] = v.d1;
    out[5] = v.kind ? 0 : host_compress_out_segments(sizes, (size_t)lo, (size_t)hi, o.data());
    if (!v.kind) for (size_t i = 0; i < hi - lo; i++) { segs[2 * i] = o[i].offset; segs[2 * i + 1] = o[i].length; }
}
