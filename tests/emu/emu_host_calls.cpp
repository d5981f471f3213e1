// tests/emu/emu_host_calls.cpp -- the plan of the host-buffer batch calls (python-zstandard_amd/csrc/zhip_host_calls.hpp) behind flat C entries.
// Test infrastructure only (tests/test_emu_host_calls.py); part of libzhip_emu.so. The plan is plain host code: nothing is emulated here.
// The pool, the device slots and the fan-out (python-zstandard_amd/csrc/zhip_host_pool.hpp) run over the stubs of host_pool_stubs.hpp.
// The entries up to emu_hc_merge are the ones tests/golden/host_calls.json was recorded through, from a library that held the parent commit's lines behind them.
#include "../../python-zstandard_amd/csrc/zhip_host_calls.hpp"
#include "host_pool_stubs.hpp"
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

// ---- what a context gives back (host_trim_order): out = the indices to release, in order; returns how many
extern "C" uint64_t emu_hc_trim_order(const uint64_t* caps, const uint8_t* trimmable, uint64_t n, uint64_t keep, uint64_t* out)
{
    std::vector<size_t> c(caps, caps + n);
    std::unique_ptr<bool[]> t(new bool[n ? n : 1]);
    for (size_t i = 0; i < n; i++) t[i] = trimmable[i] != 0;
    const std::vector<size_t> order = host_trim_order(c.data(), t.get(), (size_t)n, (size_t)keep);
    for (size_t i = 0; i < order.size(); i++) out[i] = order[i];
    return order.size();
}

// ---- the payload pool over a counting allocator. ops: (kind, arg) pairs -- 0 take(arg bytes), 1 give(what op number arg took), 2 give(a malloc(arg) the pool never saw),
// 3 the allocator refuses from here on (arg 1) or serves again (0). res, four words per op: take -> which distinct pointer this is (the op number that first returned it, while it
// lived), 1 if it came from the allocator in this op, the capacity the allocator was asked for; every op -> [3] the pool's idle bytes afterwards.
// tail: allocator calls, unpin calls, unknown frees, blocks still pinned; freedCaps: the capacities unpinned, in order (at most cap of them)
extern "C" void emu_hc_pool_script(uint64_t keep, const uint64_t* ops, uint64_t nOps, uint64_t* res, uint64_t* tail, uint64_t* freedCaps, uint64_t cap)
{
    CountingPin pin;
    std::unique_ptr<PinPool> pool(pin.pool((size_t)keep));
    std::vector<void*> got((size_t)nOps, nullptr);
    std::unordered_map<void*, uint64_t> firstOp;
    for (size_t k = 0; k < nOps; k++) {
        const uint64_t kind = ops[2 * k], arg = ops[2 * k + 1];
        uint64_t* r = res + 4 * k;
        r[0] = r[1] = r[2] = 0;
        if (kind == 0) {
            const size_t before = pin.allocated.size();
            void* p = got[k] = pool->take((size_t)arg);
            if (!firstOp.count(p)) firstOp[p] = k;
            r[0] = firstOp[p]; r[1] = pin.allocated.size() - before; r[2] = r[1] ? pin.allocated.back() : 0;
        } else if (kind == 1) {
            void* p = got[(size_t)arg]; got[(size_t)arg] = nullptr;
            const bool pooled = pin.live.count(p) != 0;
            pool->give(p);
            if (!pooled || !pin.live.count(p)) firstOp.erase(p);      // freed: the address may come back as another block
        } else if (kind == 2) pool->give(malloc((size_t)arg));
        else pin.refuse = arg != 0;
        r[3] = pool->idle;
    }
    for (void* p : got) if (p) pool->give(p);      // (whatever the script left out: nothing leaks from the entry itself)
    tail[0] = pin.allocated.size(); tail[1] = pin.freed.size(); tail[2] = (uint64_t)pin.unknownFrees; tail[3] = pin.live.size();
    for (size_t i = 0; i < pin.freed.size() && i < cap; i++) freedCaps[i] = pin.freed[i];
    for (auto& kv : pin.live) free(kv.first);
}

// ---- DevPool::parse: out = explicit list, minBytes, then the slots' devices; returns the slots
extern "C" int emu_hc_pool_parse(int count, const char* devices, const char* minBytes, uint64_t* out, int cap)
{
    DevPool p([](int) {});
    p.parse(count, devices, minBytes);
    out[0] = p.explicitList; out[1] = p.minBytes;
    for (size_t i = 0; i < p.slots.size() && (int)i < cap; i++) out[2 + i] = (uint64_t)p.slots[i];
    return (int)p.slots.size();
}

// ---- host_fan_out over d of the eight stub slots, the items' modes as StubCall reads them. out: rc, err.kind, err.index, err.zstdErr, outputs, runs, runs with lo == hi,
// after() calls, buffers the fan-out freed, buffers still alive, worker threads bound so far, 1 if every worker bound its slot's device first; order: the outputs' item indices
extern "C" void emu_hc_fan_out(const uint64_t* sizes, const uint8_t* mode, uint64_t n, uint64_t d, uint64_t* out, uint64_t* order, char* text, uint64_t textCap)
{
    static StubDevices* dev = new StubDevices();      // persistent like the library's: its threads never end
    StubCall call; call.mode = mode;
    StubCall::current() = &call;
    zhip_error err; std::string t; std::vector<uint64_t> ord;
    const int rc = call.call(dev->pool, (size_t)d, sizes, (size_t)n, &err, &t, &ord);
    out[0] = (uint64_t)rc; out[1] = (uint64_t)err.kind; out[2] = err.index; out[3] = (uint64_t)(int64_t)err.zstdErr; out[4] = ord.size(); out[5] = (uint64_t)call.runs; out[6] = (uint64_t)call.emptyRuns;
    out[7] = (uint64_t)call.afters; out[8] = (uint64_t)call.freedBufs; out[9] = (uint64_t)call.liveBufs;
    {   std::lock_guard<std::mutex> g(dev->mu);
        out[10] = dev->bound.size(); out[11] = 1;
        for (size_t w = 0; w < dev->pool.workers.size(); w++) if (dev->pool.workers[w]) { bool seen = false; for (int b : dev->bound) seen |= b == 10 + (int)w; if (!seen) out[11] = 0; }
    }
    for (size_t i = 0; i < ord.size(); i++) order[i] = ord[i];
    snprintf(text, (size_t)textCap, "%s", t.c_str());
}
