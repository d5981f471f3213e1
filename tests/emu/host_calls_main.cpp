// tests/emu/host_calls_main.cpp -- a stand-alone program (its own main) over python-zstandard_amd/csrc/zhip_host_calls.hpp for AddressSanitizer + UBSan
// (tests/emu/build_host_calls.sh; nothing is loaded into python). For a few dozen item lists it runs what a host-buffer call runs between its HIP calls, with every buffer a
// heap block of EXACTLY the bytes the plan gives: pass 1 -> cuts -> upload steps -> pack_items into a block of the step's bytes (three threads: the threshold is lowered) -> the
// step copied into a "device" block of srcTotal bytes, every item's bytes then checked at segs[i].offset; both meta layouts carved out of blocks of their reserved bytes, every
// array written at its full length; the verdicts over those arrays. Then the payload pool, the trim order and the fan-out of zhip_host_pool.hpp over the stubs of
// host_pool_stubs.hpp: every block, every output and every run's state a heap object of its own, every one of them freed by the end (LeakSanitizer counts).
// Exits 0 and prints the case count; any other exit is a finding.
#include "../../python-zstandard_amd/csrc/zhip_host_calls.hpp"
#include "host_pool_stubs.hpp"
#include <stdio.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "case %d: %s failed (line %d)\n", g_case, #x, __LINE__); exit(1); } } while (0)
static int g_case = 0;

template <typename T> struct Exact {          // a heap block of exactly n elements (n 0: one byte, never touched)
    T* p; size_t n;
    explicit Exact(size_t n_) : p((T*)malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) {}
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
};
static uint8_t byte_of(size_t item, size_t j) { return (uint8_t)(item * 131 + j * 7 + 1); }

// one list of source sizes through the compress direction's plan (its slots are the larger side) and, with the same sizes as "frames", the decompress direction's verdicts
static void run_case(const std::vector<size_t>& sizes, uint64_t stageBytes, uint64_t maxBytes, size_t maxItems, size_t firstItems)
{
    g_case++;
    const size_t n = sizes.size();
    // the items: each source a block of exactly its bytes
    std::vector<Exact<uint8_t>*> src(n);
    Exact<zhip_item> items(n);
    for (size_t i = 0; i < n; i++) {
        src[i] = new Exact<uint8_t>(sizes[i]);
        for (size_t j = 0; j < sizes[i]; j++) src[i]->p[j] = byte_of(i, j);
        items.p[i].src = src[i]->p; items.p[i].srcSize = sizes[i]; items.p[i].dstSize = sizes[i] + 1;
    }
    Exact<zhip_segment> segs(2 * n);
    uint64_t srcTotal = 0, dstTotal = 0;
    const HostRefusal no = host_compress_segments(items.p, n, segs.p, &srcTotal, &dstTotal);
    CHECK(no.kind == ZHIP_ERR_NONE);
    const std::vector<size_t> cut = host_chunks(segs.p, n, maxBytes, maxItems, firstItems);
    const size_t nChunks = cut.size() - 1;
    CHECK(cut.front() == 0 && cut.back() == n);
    Exact<uint8_t> device((size_t)srcTotal);
    for (size_t k = 0; k < nChunks; k++) {
        for (size_t a = cut[k]; a < cut[k + 1];) {
            const HostStep st = host_upload_step(segs.p, a, cut[k + 1], stageBytes);
            CHECK(st.a == a && st.b > a && st.b <= cut[k + 1]);
            Exact<uint8_t> stage((size_t)st.bytes);
            pack_items(stage.p, items.p, segs.p, st.a, st.b, 64, 3);
            CHECK(segs.p[a].offset + st.bytes <= srcTotal);
            if (st.bytes) memcpy(device.p + segs.p[a].offset, stage.p, (size_t)st.bytes);
            a = st.b;
        }
    }
    for (size_t i = 0; i < n; i++) {
        CHECK(segs.p[i].length == sizes[i] && segs.p[i].offset + sizes[i] <= srcTotal);
        for (size_t j = 0; j < sizes[i]; j++) CHECK(device.p[segs.p[i].offset + j] == byte_of(i, j));
    }
    // compress: both meta areas at exactly their bytes, every array written whole, then the verdicts chunk by chunk
    {
        const HostCompressLayout l = host_compress_layout(n, nChunks);
        Exact<uint8_t> d(l.dBytes), h(l.hBytes);
        uint64_t* dSizes = (uint64_t*)(d.p + l.dSizes); uint64_t* dOffs = (uint64_t*)(d.p + l.dOffs); uint64_t* dTotals = (uint64_t*)(d.p + l.dTotals); int32_t* dStatus = (int32_t*)(d.p + l.dStatus);
        uint64_t* hSizes = (uint64_t*)(h.p + l.hSizes); uint64_t* hTotals = (uint64_t*)(h.p + l.hTotals); int32_t* hStatus = (int32_t*)(h.p + l.hStatus);
        for (size_t i = 0; i < n; i++) { dSizes[i] = sizes[i] / 2 + 9; dOffs[i] = i; dStatus[i] = 0; }
        for (size_t k = 0; k <= nChunks; k++) dTotals[k] = k;
        for (size_t i = 0; i < n; i++) { hSizes[i] = dSizes[i]; hStatus[i] = dStatus[i]; }
        for (size_t k = 0; k <= nChunks; k++) hTotals[k] = dTotals[k];
        for (size_t i = 0; i < n; i++) CHECK(dSizes[i] == sizes[i] / 2 + 9 && dOffs[i] == i && dStatus[i] == 0 && hSizes[i] == dSizes[i] && hStatus[i] == 0);      // (no array wrote into another)
        for (size_t k = 0; k <= nChunks; k++) CHECK(dTotals[k] == k && hTotals[k] == k);
        for (size_t k = 0; k < nChunks; k++) {
            const size_t lo = cut[k], hi = cut[k + 1];
            CHECK(host_compress_verdict(hStatus, lo, hi).kind == ZHIP_ERR_NONE);
            Exact<zhip_segment> out(hi - lo);
            uint64_t want = 0;
            for (size_t i = lo; i < hi; i++) want += hSizes[i];
            CHECK(host_compress_out_segments(hSizes, lo, hi, out.p) == want);
            CHECK(out.p[0].offset == 0 && out.p[hi - lo - 1].offset + out.p[hi - lo - 1].length == want);
        }
        if (n) {
            hStatus[n - 1] = 70;
            const HostVerdict v = host_compress_verdict(hStatus, cut[nChunks - 1], n);
            CHECK(v.kind == ZHIP_ERR_ZSTD && v.index == n - 1 && v.zerr == 70);
        }
    }
    // decompress: the same, over a table whose destinations are the items' dstSize
    {
        Exact<zhip_segment> dseg(2 * n);
        uint64_t t = 0;
        for (size_t i = 0; i < n; i++) { dseg.p[i] = segs.p[i]; dseg.p[n + i].offset = t; dseg.p[n + i].length = items.p[i].dstSize; t += items.p[i].dstSize; }
        const HostDecompressLayout l = host_decompress_layout(n);
        Exact<uint8_t> d(l.dBytes), h(l.hBytes);
        uint64_t* dSizes = (uint64_t*)(d.p + l.dSizes); int32_t* dStatus = (int32_t*)(d.p + l.dStatus);
        uint64_t* hSizes = (uint64_t*)(h.p + l.hSizes); int32_t* hStatus = (int32_t*)(h.p + l.hStatus);
        for (size_t i = 0; i < n; i++) { dSizes[i] = items.p[i].dstSize; dStatus[i] = 0; }
        for (size_t i = 0; i < n; i++) { hSizes[i] = dSizes[i]; hStatus[i] = dStatus[i]; }
        for (size_t i = 0; i < n; i++) CHECK(dSizes[i] == items.p[i].dstSize && dStatus[i] == 0 && hSizes[i] == dSizes[i] && hStatus[i] == 0);
        for (size_t k = 0; k < nChunks; k++) {
            const size_t lo = cut[k], hi = cut[k + 1];
            Exact<zhip_segment> out(hi - lo);
            CHECK(host_decompress_verdict(dseg.p + n, hSizes, hStatus, lo, hi, false, out.p).kind == ZHIP_ERR_NONE);
            for (size_t i = lo; i < hi; i++) CHECK(out.p[i - lo].offset == dseg.p[n + i].offset - dseg.p[n + lo].offset && out.p[i - lo].length == hSizes[i]);
        }
        if (n) {
            const size_t lo = cut[nChunks - 1];
            Exact<zhip_segment> out(n - lo);
            hSizes[n - 1]--;
            CHECK(host_decompress_verdict(dseg.p + n, hSizes, hStatus, lo, n, true, out.p).kind == ZHIP_ERR_NONE);
            const HostVerdict v = host_decompress_verdict(dseg.p + n, hSizes, hStatus, lo, n, false, out.p);
            CHECK(v.kind == ZHIP_ERR_SIZE_MISMATCH && v.index == n - 1 && v.d0 == hSizes[n - 1] && v.d1 == hSizes[n - 1] + 1);
        }
    }
    for (size_t i = 0; i < n; i++) delete src[i];
}

// the pool under keep limits from nothing to everything, a foreign pointer, a refused allocation; every block is unpinned exactly once by the end
static void run_pool(size_t keep)
{
    g_case++;
    const size_t M = (size_t)1 << 20;
    CountingPin pin; pin.exact = true;
    PinPool* pool = pin.pool(keep);
    auto touch = [](void* p, size_t n) { if (n) { ((volatile uint8_t*)p)[0] = 1; ((volatile uint8_t*)p)[n - 1] = 2; } };      // a payload of n bytes holds n bytes
    std::vector<void*> held;
    const size_t want[] = {0, 1, ZHIP_PIN_MIN - 1, ZHIP_PIN_MIN, 3 * M, 70 * M, 4 * M, 100 * M, 5 * M + 1, 64 * M};
    for (int round = 0; round < 6; round++) {
        for (size_t n : want) { void* p = pool->take(n); CHECK(p != nullptr); touch(p, n); held.push_back(p); }
        for (size_t k = round % 3; k < held.size(); k += 2) { pool->give(held[k]); held[k] = nullptr; CHECK(pool->idle <= keep); }
        if (round == 2) { pin.refuse = true; void* p = pool->take(300 * M); CHECK(p != nullptr); touch(p, 300 * M); pool->give(p); pin.refuse = false; }      // no idle block holds it, none can be pinned: pageable, at its bytes
        pool->give(malloc(100));
    }
    for (void* p : held) pool->give(p);
    CHECK(pool->idle <= keep && pin.unknownFrees == 0 && pin.allocated.size() == pin.freed.size() + pin.live.size());
    for (auto& kv : pool->blocks) { CHECK(!kv.second.busy); pin.unpin(kv.first); }      // what the limit let the pool keep
    CHECK(pin.live.empty() && pin.allocated.size() == pin.freed.size());
    delete pool;
}
static void run_trim()
{
    g_case++;
    const size_t F = (size_t)64 << 20;
    Exact<size_t> caps(5); Exact<bool> flags(5);
    const size_t c[5] = {F + 1, 3 * F, F, 3 * F, 10 * F}; const bool t[5] = {true, true, true, true, false};
    for (int i = 0; i < 5; i++) { caps.p[i] = c[i]; flags.p[i] = t[i]; }
    CHECK(host_trim_order(caps.p, flags.p, 5, 0) == (std::vector<size_t>{1, 3, 0}));
    CHECK(host_trim_order(caps.p, flags.p, 5, 15 * F + 1).size() == 1 && host_trim_order(caps.p, flags.p, 5, 18 * F + 1).empty() && host_trim_order(caps.p, flags.p, 0, 0).empty());
}
// the fan-out over 1 .. 8 slots: clean runs, failing runs and runs that throw; nothing a run or the merge allocated is left behind
static void run_fan_out(StubDevices& dev)
{
    const std::vector<std::vector<uint64_t>> lists = {{1}, {0, 0, 0}, {5, 5}, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13}, {100, 1, 1, 1, 1, 1, 1, 1, 1}};
    for (const auto& sizes : lists) for (size_t d = 1; d <= 8; d++) for (int mode = 0; mode <= 3; mode++) for (size_t bad : {(size_t)0, sizes.size() / 2, sizes.size() - 1}) {
        g_case++;
        Exact<uint64_t> sz(sizes.size()); Exact<uint8_t> md(sizes.size());
        for (size_t i = 0; i < sizes.size(); i++) { sz.p[i] = sizes[i]; md.p[i] = i == bad || (mode && i == sizes.size() - 1) ? (uint8_t)mode : 0; }
        StubCall call; call.mode = md.p;
        StubCall::current() = &call;
        zhip_error err; std::string text; std::vector<uint64_t> order;
        const int rc = call.call(dev.pool, d, sz.p, sizes.size(), &err, &text, &order);
        CHECK(call.emptyRuns == 0 && call.liveBufs == 0 && call.runs == call.afters);
        if (mode == 0) { CHECK(rc == 0 && order.size() == sizes.size()); for (size_t i = 0; i < order.size(); i++) CHECK(order[i] == i); }
        else CHECK(rc == (mode == 1 ? ZHIP_ERR_ZSTD : mode == 2 ? ZHIP_ERR_NO_MEMORY : ZHIP_ERR_HIP) && err.kind == rc && order.empty() && !text.empty());
    }
}

int main()
{
    const uint64_t stage = 1000;          // an upload step, in place of 512 MiB
    std::vector<std::vector<size_t>> lists = {
        {}, {0}, {1}, {0, 0, 0}, {1, 1, 1, 1, 1, 1, 1, 1}, {1000}, {1001}, {999, 1}, {1000, 1000, 1000}, {0, 1000, 0, 1000, 0}, {5000}, {1, 5000, 1}, {5000, 5000},
        {500, 500, 1}, {499, 500, 1, 0, 0, 0}, {64, 64, 64, 64, 64, 64}, {10, 20, 30, 40, 50, 60, 70, 80, 90, 100, 110, 120}, {300, 0, 300, 0, 300, 0, 99, 1},
    };
    for (size_t n : {7u, 16u, 33u, 100u}) {          // mixed sizes, a fixed sequence: empty, one-byte, small and above-a-step items
        std::vector<size_t> v(n);
        for (size_t i = 0; i < n; i++) { const size_t r = (i * 2654435761u >> 5) % 97; v[i] = r < 8 ? 0 : r < 16 ? 1 : r < 90 ? r * 3 : r * 40; }
        lists.push_back(v);
    }
    int cases = 0;
    for (const auto& v : lists) {
        run_case(v, stage, (uint64_t)1 << 30, 32768, 0); cases++;          // one chunk
        run_case(v, stage, 1500, 5, 2); cases++;                          // several chunks, a smaller first one
    }
    for (size_t keep : {(size_t)0, (size_t)10 << 20, (size_t)200 << 20, (size_t)24 << 30}) { run_pool(keep); cases++; }
    run_trim(); cases++;
    {   static StubDevices* dev = new StubDevices();      // (its threads never end: kept reachable, as the library keeps its own)
        const int before = g_case;
        run_fan_out(*dev);
        cases += g_case - before;
    }
    printf("ok: %d cases\n", cases);
    return 0;
}
