// tests/emu/xor_planes_main.cpp -- the stand-alone sanitizer program of the xor-with-base filter's kernels (tests/emu/build_asan_planes.sh): the split-with-xor and
// join-with-xor bodies of python-zstandard_amd/csrc/zhip_seekable_typed.hpp under the host wave emulator, every buffer -- the base among them -- a heap
// allocation of exactly the bytes the kernel may touch, at byte offsets 0, 1 and 3 from the allocation: a read or a write one byte outside is the
// sanitizer's finding. The results are checked against plain loops. Exit 0: every case held. Test infrastructure only.
#include "emu_seekable_xor_base.cpp"
#include "exact_buffers.hpp"

int main()
{
    g_seed = 97531;
    static const uint32_t sizes[] = {1, 15, 16, 17, 1023, 1024, 1025, 2500}, lasts[] = {1, 15, 17}, offsets[] = {0, 1, 3}, ks[] = {2, 4, 8};
    int cases = 0, shape = 0;
    for (uint32_t k : ks) for (uint32_t m : sizes) for (uint32_t last : lasts) for (int kind = 0; kind < 3; kind++) {
        // two groups of m and a last one; the base: the source, random bytes, the source with low bits flipped. The byte offsets take turns
        if (last > m) continue;
        const uint32_t off = offsets[shape++ % 3];
        const uint64_t elements = 2 * (uint64_t)m + last, size = elements * k;
        const uint32_t nGroups = (uint32_t)zsk_frame_count(elements, m);
        Exact src(size, off, 1), base(size, (off + 2) % 4, 1), planar(size, (off + 1) % 4, 0), back(size, off, 0);
        if (kind != 1) for (uint64_t i = 0; i < size; i++) base.at[i] = kind == 0 || i % k ? src.at[i] : src.at[i] ^ (next_byte() & 7);
        std::vector<uint64_t> records(2 * (size_t)nGroups * k);
        for (uint32_t grid : {emu_typed_grid(1, size, k, m), 1u}) {
            if (grid == 1 && kind != 1) continue;      // (one workgroup, the grid-stride loop: once per shape)
            emu_xor_split(src.at, base.at, size, k, m, planar.at, grid, records.data());
            for (uint64_t g = 0; g < nGroups; g++) {
                const uint64_t e = zsk_group_len(elements, m, g), at = g * m * k;
                for (uint64_t i = 0; i < e; i++) for (uint32_t p = 0; p < k; p++)
                    if (planar.at[at + p * e + i] != (uint8_t)(src.at[at + i * k + p] ^ base.at[at + i * k + p])) return fail("split", k, m, off);
                for (uint32_t p = 0; p < k; p++) if (records[2 * (g * k + p)] != at + p * e || records[2 * (g * k + p) + 1] != e) return fail("records", k, m, off);
            }
            emu_xor_join(planar.at, base.at, back.at, nullptr, 0, size, k, m, grid);
            if (memcmp(back.at, src.at, (size_t)size)) return fail("join", k, m, off);
            cases++;
        }
        if (last != 1 || kind != 1) continue;
        // one job of m elements that trims its ends, its base bytes `content` bytes into a base of exactly content + the bytes the job stores: the kernel
        // is handed base - h', so that a read of a trimmed byte is a read outside the allocation
        for (uint64_t content : {(uint64_t)0, (uint64_t)7 * k}) for (uint32_t h : {0u, 1u, k - 1}) for (uint32_t t : {0u, k - 1}) {
            if (h + t >= (uint64_t)m * k) continue;
            const uint64_t bytes = (uint64_t)m * k - h - t;
            Exact pl((size_t)m * k, off, 1), b2(bytes, (off + 1) % 4, 1), out(bytes, (off + 2) % 4, 0);
            const uint64_t job[6] = {0, m, 0, h, t, content};
            emu_xor_join(pl.at, b2.at - h - content, out.at, job, 1, 0, k, 1, 2);      // base + content + h is b2's first byte
            for (uint64_t j = h; j < (uint64_t)m * k - t; j++)
                if (out.at[j - h] != (uint8_t)(pl.at[(j % k) * m + j / k] ^ b2.at[j - h])) return fail("trimmed join", k, m, off);
            cases++;
        }
    }
    printf("%d cases\n", cases);
    return 0;
}
