// tests/emu/host_pool_tsan_main.cpp -- a stand-alone program (its own main) over python-zstandard_amd/csrc/zhip_host_pool.hpp for ThreadSanitizer
// (tests/emu/build_host_pool_tsan.sh; nothing is loaded into python). Two things run from several threads at once in the library and nowhere on the CPU otherwise:
// (1) host_fan_out, back to back from 4 caller threads over 3 shared slots, with a stub run that returns at once -- the caller is then most likely to return while a worker
//     still stands between its count-down and its notify, which is the window in which per-call state on the caller's stack would be touched after its frame is gone;
// (2) PinPool::take / give from 8 threads over a counting allocator.
// Exits 0 and prints what it ran; any ThreadSanitizer report is a finding.
#include "host_pool_stubs.hpp"
#include <stdio.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s failed (line %d)\n", #x, __LINE__); exit(1); } } while (0)

int main(int argc, char** argv)
{
    const int calls = argc > 1 ? atoi(argv[1]) : 1500;          // per caller thread
    static StubDevices* dev = new StubDevices();                // persistent and never destroyed, like the library's
    static StubCall call;                                       // no failing items: every call returns its items in order
    StubCall::current() = &call;
    std::atomic<long> outputs{0};
    {
        std::vector<std::thread> callers;
        for (int t = 0; t < 4; t++) callers.emplace_back([&, t] {
            const uint64_t sizes[7] = {3, 0, 5, 1, 1, 9, (uint64_t)t};
            for (int k = 0; k < calls; k++) {
                zhip_error err; std::string text; std::vector<uint64_t> order;
                const size_t n = 1 + (size_t)(k + t) % 7;
                CHECK(call.call(dev->pool, 3, sizes, n, &err, &text, &order) == 0 && order.size() == n);
                for (size_t i = 0; i < n; i++) CHECK(order[i] == i);
                outputs += (long)n;
            }
        });
        for (auto& th : callers) th.join();
    }
    CHECK(call.liveBufs == 0 && call.emptyRuns == 0 && call.runs == call.afters);

    CountingPin pin;
    PinPool* pool = pin.pool((size_t)40 << 20);
    {
        std::vector<std::thread> users;
        for (int t = 0; t < 8; t++) users.emplace_back([&, t] {
            const size_t M = (size_t)1 << 20, want[5] = {ZHIP_PIN_MIN - 1, 2 * M, 7 * M, 30 * M, 3 * M + (size_t)t};
            void* held[4] = {nullptr, nullptr, nullptr, nullptr};
            for (int k = 0; k < 2000; k++) {
                void*& h = held[(k + t) % 4];
                if (h) { pool->give(h); h = nullptr; }
                else { h = pool->take(want[(k * 7 + t) % 5]); CHECK(h != nullptr); *(volatile char*)h = (char)t; }      // (only the holder writes a block)
            }
            for (void* h : held) pool->give(h);
        });
        for (auto& th : users) th.join();
    }
    CHECK(pool->idle <= ((size_t)40 << 20) && pin.unknownFrees == 0);
    for (auto& kv : pool->blocks) { CHECK(!kv.second.busy); pin.unpin(kv.first); }
    CHECK(pin.live.empty() && pin.allocated.size() == pin.freed.size());
    delete pool;
    printf("ok: %d fan-out calls from 4 threads over 3 slots (%ld outputs, %d runs), %zu blocks pinned by 8 threads\n", 4 * calls, outputs.load(), (int)call.runs, pin.allocated.size());
    return 0;
}
