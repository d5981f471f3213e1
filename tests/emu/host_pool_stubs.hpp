// tests/emu/host_pool_stubs.hpp -- what the CPU tests pass to python-zstandard_amd/csrc/zhip_host_pool.hpp in place of HIP: a counting allocator behind PinPool, a device pool
// whose bind() only records, and a stub for one run of a host-buffer call. Test infrastructure only (emu_host_calls.cpp, host_calls_main.cpp, host_pool_tsan_main.cpp).
#pragma once
#include "../../python-zstandard_amd/csrc/zhip_host_pool.hpp"
#include <atomic>
#include <stdexcept>

// "pinned" blocks: malloc() of exactly the capacity asked for -- or, exact = false, of 16 bytes (the pool never touches a block's bytes) -- the capacity remembered beside it
struct CountingPin {
    bool exact = false;
    std::mutex mu;
    std::unordered_map<void*, size_t> live;      // block -> the capacity it was asked with
    std::vector<size_t> allocated, freed;        // capacities, in call order
    bool refuse = false;                         // alloc() answers nullptr: "no pinned memory"
    int unknownFrees = 0;                        // free() of what alloc() never gave, or gave and took back already
    void* alloc(size_t cap)
    {
        std::lock_guard<std::mutex> g(mu);
        if (refuse) return nullptr;
        void* p = malloc(exact ? cap : 16);
        live[p] = cap; allocated.push_back(cap);
        return p;
    }
    void unpin(void* p)
    {
        std::lock_guard<std::mutex> g(mu);
        auto it = live.find(p);
        if (it == live.end()) { unknownFrees++; return; }
        freed.push_back(it->second); live.erase(it);
        free(p);
    }
    PinPool* pool(size_t keep) { return new PinPool([this](size_t cap) { return alloc(cap); }, [this](void* p) { unpin(p); }, keep); }
};

// eight slots "on" devices 10 .. 17 of 32; every worker thread's first action is recorded
struct StubDevices {
    std::mutex mu; std::vector<int> bound;
    DevPool pool;
    StubDevices() : pool([this](int device) { std::lock_guard<std::mutex> g(mu); bound.push_back(device); }) { pool.parse(32, "10,11,12,13,14,15,16,17", nullptr); }
};

// one run of a call over items [lo, hi): an output per item, its dataSize the item's index in the whole batch. mode[i]: 0 fine, 1 the run fails at item i (ZHIP_ERR_ZSTD, zstd error
// 70, index counted from lo, its own outputs freed), 2 the run throws std::bad_alloc there, 3 std::runtime_error("stub: boom")
struct StubCall {
    const uint8_t* mode = nullptr;
    std::atomic<int> runs{0}, emptyRuns{0}, afters{0}, freedBufs{0}, liveBufs{0};
    static StubCall*& current() { static StubCall* c = nullptr; return c; }      // (freeOut is a plain function pointer)
    int one(size_t lo, size_t hi, zhip_outbuf** out, size_t* nOut, zhip_error* err)
    {
        runs++;
        if (lo >= hi) emptyRuns++;
        *out = nullptr; *nOut = 0;
        for (size_t i = lo; i < hi; i++) {
            if (mode && mode[i] == 1) { err->kind = ZHIP_ERR_ZSTD; err->zstdErr = 70; err->index = i - lo; return ZHIP_ERR_ZSTD; }
            if (mode && mode[i] == 2) throw std::bad_alloc();
            if (mode && mode[i] == 3) throw std::runtime_error("stub: boom");
        }
        zhip_outbuf* ob = (zhip_outbuf*)calloc(hi - lo, sizeof(zhip_outbuf));
        for (size_t i = lo; i < hi; i++) { ob[i - lo].data = malloc(1); ob[i - lo].segs = (zhip_segment*)malloc(sizeof(zhip_segment)); ob[i - lo].dataSize = i; ob[i - lo].nSegs = 0; }
        liveBufs += (int)(hi - lo);
        *out = ob; *nOut = hi - lo;
        return ZHIP_ERR_NONE;
    }
    static void release(zhip_outbuf* b, size_t n)
    {
        for (size_t i = 0; b && i < n; i++) { free(b[i].data); free(b[i].segs); }
        free(b);
        current()->liveBufs -= (int)n;
    }
    static void free_out(zhip_outbuf* b, size_t n) { release(b, n); current()->freedBufs += (int)n; }      // what the fan-out frees of the runs that did not fail
    // the whole call; frees what it got. order: the outputs' dataSize in the order they came back
    int call(DevPool& pool, size_t d, const uint64_t* sizes, size_t n, zhip_error* err, std::string* text, std::vector<uint64_t>* order)
    {
        zhip_outbuf* out = nullptr; size_t nOut = 0;
        memset(err, 0, sizeof *err);
        const int rc = host_fan_out(pool, d, sizes, n, [this](size_t lo, size_t hi, zhip_outbuf** o, size_t* no, zhip_error* e) { return one(lo, hi, o, no, e); },
                                    [this](size_t, int r) { afters++; return r ? std::string("stub: run failed") : std::string(); }, free_out, &out, &nOut, err, text);
        if (order) for (size_t k = 0; k < nOut; k++) order->push_back(out[k].dataSize);
        release(out, nOut);
        return rc;
    }
};
