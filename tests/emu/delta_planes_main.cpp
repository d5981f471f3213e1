// tests/emu/delta_planes_main.cpp -- the stand-alone sanitizer program of the delta filter's kernels (tests/emu/build_asan_planes.sh): the split-with-delta, tile
// sums, tile offsets and join-scan-store bodies of python-zstandard_amd/csrc/zhip_seekable_typed.hpp under the host wave emulator, every buffer a heap
// allocation of exactly the bytes the kernel may touch, at byte offsets 0, 1 and 3 from the allocation -- a read or a write one byte outside is the
// sanitizer's finding. The results are checked against plain loops. Exit 0: every case held. Test infrastructure only.
#include "emu_seekable_delta.cpp"
#include "exact_buffers.hpp"

static uint64_t element(const uint8_t* p, uint32_t k) { uint64_t v = 0; for (uint32_t b = 0; b < k; b++) v |= (uint64_t)p[b] << (8 * b); return v; }

int main()
{
    g_seed = 54321;
    static const uint32_t sizes[] = {1, 15, 16, 17, 1023, 1024, 1025, 2067, 3077}, lasts[] = {1, 15, 17}, offsets[] = {0, 1, 3}, ks[] = {2, 4, 8};
    int cases = 0, shape = 0;
    for (uint32_t k : ks) for (uint32_t m : sizes) for (uint32_t last : lasts) for (int fill = 1; fill <= 2; fill++) {
        // two groups of m and a last one: random bytes (every subtraction wraps), and all bits set (the differences' sums carry through every byte); the
        // byte offsets take turns
        if (last > m) continue;
        const uint32_t off = offsets[shape++ % 3];
        const uint64_t elements = 2 * (uint64_t)m + last, size = elements * k, mask = k == 8 ? ~0ull : (1ull << (8 * k)) - 1;
        const uint32_t nGroups = (uint32_t)zsk_frame_count(elements, m);
        Exact src(size, off, fill), planar(size, (off + 1) % 4, 0), back(size, off, 0);
        std::vector<uint64_t> records(2 * (size_t)nGroups * k);
        for (uint32_t grid : {emu_typed_grid(1, size, k, m), 1u}) {
            if (grid == 1 && fill != 1) continue;      // (one workgroup, the grid-stride loop: once per shape)
            emu_delta_split(src.at, size, k, m, planar.at, grid, records.data());
            std::vector<uint64_t> wantOffsets;
            for (uint64_t g = 0; g < nGroups; g++) {
                const uint64_t e = zsk_group_len(elements, m, g), base = g * m * k;
                uint64_t before = 0, run = 0;
                for (uint64_t i = 0; i < e; i++) {
                    const uint64_t x = element(src.at + base + i * k, k), d = (x - before) & mask;
                    if (i % ZSK_PLANE_TILE == 0) wantOffsets.push_back(run);
                    run += d; before = x;
                    for (uint32_t p = 0; p < k; p++) if (planar.at[base + p * e + i] != (uint8_t)(d >> (8 * p))) return fail("split", k, m, off);
                }
                for (uint64_t t = zsk_join_tiles(e); t < zsk_join_tiles(m); t++) wantOffsets.push_back(run);      // (the empty tiles behind a shorter last group)
                for (uint32_t p = 0; p < k; p++) if (records[2 * (g * k + p)] != base + p * e || records[2 * (g * k + p) + 1] != e) return fail("records", k, m, off);
            }
            const uint64_t tiles = emu_delta_join(planar.at, back.at, nullptr, 0, size, k, m, grid, nullptr);
            if (tiles != wantOffsets.size()) return fail("tiles", k, m, off);
            std::unique_ptr<uint64_t[]> sums(new uint64_t[(size_t)tiles]);
            emu_delta_join(planar.at, back.at, nullptr, 0, size, k, m, grid, sums.get());
            if (memcmp(back.at, src.at, (size_t)size)) return fail("join", k, m, off);
            if (memcmp(sums.get(), wantOffsets.data(), (size_t)tiles * 8)) return fail("tile offsets", k, m, off);
            cases++;
        }
        if (last != 1 || fill != 1) continue;
        // one job of m elements that skips some and trims its ends: the destination holds exactly the bytes that remain
        for (uint64_t skip : {(uint64_t)0, (uint64_t)1, (uint64_t)m / 2, (uint64_t)m - 1}) for (uint32_t h : {0u, 1u, k - 1}) for (uint32_t t : {0u, k - 1}) {
            if (skip >= m || skip * k + h + t >= (uint64_t)m * k) continue;
            const uint64_t bytes = (uint64_t)m * k - skip * k - h - t;
            Exact pl((size_t)m * k, off, 1), out(bytes, (off + 2) % 4, 0);
            const uint64_t job[6] = {0, m, 0, h, t, skip};
            std::unique_ptr<uint64_t[]> sums(new uint64_t[(size_t)zsk_join_tiles(m)]);
            emu_delta_join(pl.at, out.at, job, 1, 0, k, 1, 2, sums.get());
            uint64_t run = 0;
            for (uint64_t i = 0; i < m; i++) {
                uint64_t d = 0;
                for (uint32_t p = 0; p < k; p++) d |= (uint64_t)pl.at[p * m + i] << (8 * p);
                run += d;
                for (uint32_t p = 0; p < k; p++) { const uint64_t j = i * k + p; if (j >= skip * k + h && j < (uint64_t)m * k - t && out.at[j - skip * k - h] != (uint8_t)(run >> (8 * p))) return fail("skipped join", k, m, off); }
            }
            cases++;
        }
    }
    printf("%d cases\n", cases);
    return 0;
}
