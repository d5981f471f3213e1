// zhip_host_pool.hpp -- HOST side, free of HIP: the threads and the pooled memory behind the host-buffer batch calls. The pinned payload pool, the per-device worker threads and
// the fan-out of one call over them are plain C++ here; everything that is HIP -- how a block is pinned and unpinned, what binds a thread to its device, what one run of a call
// does -- arrives as a parameter. zhip_lib.hip passes the HIP calls in; the CPU tests (tests/emu/emu_host_calls.cpp, tests/emu/host_calls_main.cpp under AddressSanitizer,
// tests/emu/host_pool_tsan_main.cpp under ThreadSanitizer) pass stubs.
#pragma once
#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include "zhip_host_calls.hpp"

// ------------------------------------------------------------------------------------------ the payload pool
#define ZHIP_PIN_MIN ((size_t)1 << 20)                // payloads below 1 MiB are plain malloc() (one-shot calls, small batches)
// Payload blocks of the results: pinning costs far more than the copy it speeds up, so blocks return here when the caller frees them and serve later calls. take(n): the smallest
// idle block of at least n bytes, unless even that one is larger than n + n/2 + 64 MiB -- then a new one, rounded up to 2 MiB, from alloc(cap) (nullptr: no pinned memory, the
// payload is pageable malloc). give(p): idle again; above `keep` idle bytes the largest idle blocks are unpinned first, outside the lock. A pointer the pool does not know is free()d.
struct PinPool {
    const std::function<void*(size_t)> alloc; const std::function<void(void*)> unpin; const size_t keep;
    struct Block { size_t cap; bool busy; };
    std::mutex mu;
    std::unordered_map<void*, Block> blocks;
    size_t idle = 0;
    PinPool(std::function<void*(size_t)> alloc_, std::function<void(void*)> unpin_, size_t keep_) : alloc(std::move(alloc_)), unpin(std::move(unpin_)), keep(keep_) {}
    void* take(size_t n)
    {
        if (n < ZHIP_PIN_MIN) return malloc(n ? n : 1);
        {
            std::lock_guard<std::mutex> g(mu);
            void* best = nullptr; size_t bestCap = ~(size_t)0;
            for (auto& kv : blocks) if (!kv.second.busy && kv.second.cap >= n && kv.second.cap < bestCap) { best = kv.first; bestCap = kv.second.cap; }
            if (best && bestCap <= n + (n >> 1) + ((size_t)64 << 20)) { blocks[best].busy = true; idle -= bestCap; return best; }
        }
        const size_t cap = (n + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
        void* p = alloc(cap);
        if (!p) return malloc(n);     // pageable still works, slower
        std::lock_guard<std::mutex> g(mu);
        blocks[p] = Block{cap, true};
        return p;
    }
    void give(void* p)
    {
        if (!p) return;
        std::vector<void*> drop;
        {
            std::lock_guard<std::mutex> g(mu);
            auto it = blocks.find(p);
            if (it == blocks.end()) { free(p); return; }
            it->second.busy = false; idle += it->second.cap;
            while (idle > keep) {                       // unpin the largest idle blocks first
                void* big = nullptr; size_t bigCap = 0;
                for (auto& kv : blocks) if (!kv.second.busy && kv.second.cap > bigCap) { big = kv.first; bigCap = kv.second.cap; }
                if (!big) break;
                idle -= bigCap; blocks.erase(big); drop.push_back(big);
            }
        }
        for (void* q : drop) unpin(q);
    }
};

// ------------------------------------------------------------------------------------------ a thread per device slot
// persistent, created on first use, detached and never destroyed (its thread-local context lives as long as the process). Its first action is bind(device)
struct DevWorker {
    std::mutex mu; std::condition_variable cv;
    std::deque<std::function<void()>> q;
    void loop()
    {
        for (;;) {
            std::function<void()> fn;
            { std::unique_lock<std::mutex> l(mu); cv.wait(l, [&] { return !q.empty(); }); fn = std::move(q.front()); q.pop_front(); }
            fn();
        }
    }
    void post(std::function<void()> fn) { { std::lock_guard<std::mutex> l(mu); q.push_back(std::move(fn)); } cv.notify_one(); }      // (a worker and its cv are never destroyed)
};
struct DevPool {
    const std::function<void(int)> bind;         // what a worker thread does first with its device ordinal (the library: hipSetDevice)
    std::mutex mu;
    bool explicitList = false;
    std::vector<int> slots;                      // device ordinal of every slot
    std::vector<DevWorker*> workers;
    uint64_t minBytes = (uint64_t)256 << 20;
    explicit DevPool(std::function<void(int)> bind_) : bind(std::move(bind_)) {}
    // once, before the pool is shared: `count` visible devices, ZHIP_DEVICES and ZHIP_DEVICE_MIN_BYTES as the environment has them (nullptr: unset)
    void parse(int count, const char* devices, const char* minBytesText)
    {
        if (minBytesText) minBytes = strtoull(minBytesText, nullptr, 10);
        explicitList = devices != nullptr;
        if (devices) slots = host_parse_devices(devices, count);
        else for (int d = 0; d < count; d++) slots.push_back(d);
        workers.assign(slots.size(), nullptr);
    }
    DevWorker* worker(size_t slot)
    {
        std::lock_guard<std::mutex> l(mu);
        if (!workers[slot]) { DevWorker* w = new DevWorker(); const int device = slots[slot]; std::thread([this, w, device] { bind(device); w->loop(); }).detach(); workers[slot] = w; }
        return workers[slot];
    }
    // device slots a batch of `n` items / `bytes` input bytes is cut over (0: the calling thread's current device, inline)
    size_t slotsFor(size_t n, uint64_t bytes) const { return host_slots_for(slots.size(), explicitList, minBytes, n, bytes); }
};

// ------------------------------------------------------------------------------------------ one call over the slots
// Cuts the n items over d slots (host_partition_by_bytes), runs one(lo, hi, &out, &nOut, &err) -> rc for every run on its slot's thread, then after(slot, rc) -> the run's error
// text on the same thread, waits for all of them, and merges: the lowest failing run's code, error (index counted from the call's first item) and text, every other run's buffers
// given to freeOut; else the runs' buffers in run order, which is item order. A run that throws std::bad_alloc counts as ZHIP_ERR_NO_MEMORY, any other std::exception as
// ZHIP_ERR_HIP with what() as its text, index 0 both.
// Lifetime: everything a job touches after one() -- the lock, the condition variable, the count, its run -- is in ONE heap object that every posted job holds by shared_ptr.
// The caller may return the moment it sees pending == 0; a worker still between its unlock and its notify then signals an object its own reference keeps alive.
// (one() itself may refer to the caller's frame: it has returned before the job counts down.)
template <typename One, typename After>
int host_fan_out(DevPool& pool, size_t d, const uint64_t* sizes, size_t n, One one, After after, void (*freeOut)(zhip_outbuf*, size_t),
                 zhip_outbuf** out, size_t* nOut, zhip_error* err, std::string* text)
{
    struct State {
        One one; After after;
        std::mutex mu; std::condition_variable cv; size_t pending;
        std::vector<HostRun> runs; std::vector<std::string> text;      // what every run's call returned, and its thread's error text
        State(One o, After a, size_t used) : one(std::move(o)), after(std::move(a)), pending(used), runs(used), text(used) {}
    };
    std::vector<size_t> bounds(2 * d);
    const size_t used = host_partition_by_bytes(sizes, n, d, bounds.data());
    auto st = std::make_shared<State>(std::move(one), std::move(after), used);
    for (size_t w = 0; w < used; w++) {
        const size_t lo = bounds[2 * w], hi = bounds[2 * w + 1];
        pool.worker(w)->post([st, w, lo, hi] {
            HostRun& r = st->runs[w];
            r.lo = lo;
            memset(&r.err, 0, sizeof r.err);
            bool threw = false; std::string what;
            try { r.rc = st->one(lo, hi, &r.out, &r.nOut, &r.err); }
            catch (const std::bad_alloc&) { threw = true; r.rc = ZHIP_ERR_NO_MEMORY; what = "out of host memory"; }
            catch (const std::exception& e) { threw = true; r.rc = ZHIP_ERR_HIP; what = e.what(); }
            if (threw) { memset(&r.err, 0, sizeof r.err); r.err.kind = r.rc; r.out = nullptr; r.nOut = 0; }
            st->text[w] = st->after(w, r.rc);
            if (threw) st->text[w] = what;
            { std::lock_guard<std::mutex> l(st->mu); st->pending--; }
            st->cv.notify_one();
        });
    }
    { std::unique_lock<std::mutex> l(st->mu); st->cv.wait(l, [&] { return st->pending == 0; }); }
    std::vector<HostRun>& runs = st->runs;
    const size_t bad = host_merge_failing(runs.data(), used, err);
    if (bad < used) {
        for (size_t v = 0; v < used; v++) if (!runs[v].rc) freeOut(runs[v].out, runs[v].nOut);
        *text = st->text[bad];
        return runs[bad].rc;
    }
    zhip_outbuf* all = host_merge_concat(runs.data(), used, nOut);
    if (!all) { for (size_t w = 0; w < used; w++) freeOut(runs[w].out, runs[w].nOut); if (err) { memset(err, 0, sizeof *err); err->kind = ZHIP_ERR_NO_MEMORY; } return ZHIP_ERR_NO_MEMORY; }
    *out = all;
    return ZHIP_ERR_NONE;
}
