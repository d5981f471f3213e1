// tests/emu/chain_planes_main.cpp -- the stand-alone sanitizer program of the chain join kernel (tests/emu/build_asan_planes.sh): zsk_planes_join_chain_body of
// python-zstandard_amd/csrc/zhip_seekable_typed.hpp under the host wave emulator with 1, 2, 3 and 16 links, with and without a base, every buffer -- every
// link's planar buffer and the base among them -- a heap allocation of exactly the bytes the kernel may touch, at byte offsets 0, 1 and 3 from the
// allocation: a read or a write one byte outside is the sanitizer's finding. The results are checked against plain loops. Exit 0: every case held. Test
// infrastructure only.
#include "emu_seekable_chain.cpp"
#include "exact_buffers.hpp"

static int fail(const char* what, uint32_t k, uint64_t m, uint32_t links, uint32_t off) { fprintf(stderr, "%s: k = %u, m = %llu, %u links, offset %u\n", what, k, (unsigned long long)m, links, off); return 1; }

int main()
{
    g_seed = 24681;
    static const uint32_t sizes[] = {1, 15, 16, 17, 1023, 1024, 1025, 2500}, lasts[] = {1, 15, 17}, offsets[] = {0, 1, 3}, ks[] = {2, 4, 8}, counts[] = {1, 2, 3, 16};
    int cases = 0, shape = 0;
    for (uint32_t k : ks) for (uint32_t m : sizes) for (uint32_t last : lasts) for (uint32_t links : counts) for (int withBase = 0; withBase < 2; withBase++) {
        // two groups of m and a last one. The byte offsets take turns, and differ between the links
        if (last > m) continue;
        const uint32_t off = offsets[shape++ % 3];
        const uint64_t elements = 2 * (uint64_t)m + last, size = elements * k;
        const uint32_t nGroups = (uint32_t)zsk_frame_count(elements, m);
        std::vector<std::unique_ptr<Exact>> pl;
        std::vector<const uint8_t*> ptrs;
        for (uint32_t i = 0; i < links; i++) { pl.emplace_back(new Exact(size, (off + i) % 4, 1)); ptrs.push_back(pl.back()->at); }
        Exact base(size, (off + 2) % 4, 1), out(size, (off + 1) % 4, 0);
        for (uint32_t grid : {emu_typed_grid(1, size, k, m), 1u}) {
            if (grid == 1 && (links != 3 || last != 17)) continue;      // (one workgroup, the grid-stride loop: once per group size)
            emu_chain_join(ptrs.data(), links, withBase ? base.at : nullptr, out.at, nullptr, 0, size, k, m, grid);
            for (uint64_t g = 0; g < nGroups; g++) {
                const uint64_t e = zsk_group_len(elements, m, g), at = g * m * k;
                for (uint64_t i = 0; i < e; i++) for (uint32_t p = 0; p < k; p++) {
                    uint8_t want = withBase ? base.at[at + i * k + p] : 0;
                    for (uint32_t l = 0; l < links; l++) want ^= ptrs[l][at + p * e + i];
                    if (out.at[at + i * k + p] != want) return fail("join", k, m, links, off);
                }
            }
            cases++;
        }
        if (last != 1 || (links != 2 && links != 3)) continue;
        // one job of m elements that trims its ends, its base bytes `content` bytes into a base of exactly the bytes the job stores: the kernel is handed
        // base - h - content, so that a read of a trimmed byte is a read outside the allocation
        for (uint64_t content : {(uint64_t)0, (uint64_t)7 * k}) for (uint32_t h : {0u, 1u, k - 1}) for (uint32_t t : {0u, k - 1}) {
            if (h + t >= (uint64_t)m * k) continue;
            const uint64_t bytes = (uint64_t)m * k - h - t;
            std::vector<std::unique_ptr<Exact>> jp;
            std::vector<const uint8_t*> jptrs;
            for (uint32_t i = 0; i < links; i++) { jp.emplace_back(new Exact((size_t)m * k, (off + i) % 4, 1)); jptrs.push_back(jp.back()->at); }
            Exact b2(bytes, (off + 1) % 4, 1), o2(bytes, (off + 2) % 4, 0);
            const uint64_t job[6] = {0, m, 0, h, t, content};
            emu_chain_join(jptrs.data(), links, withBase ? b2.at - h - content : nullptr, o2.at, job, 1, 0, k, 1, 2);      // base + content + h is b2's first byte
            for (uint64_t j = h; j < (uint64_t)m * k - t; j++) {
                uint8_t want = withBase ? b2.at[j - h] : 0;
                for (uint32_t l = 0; l < links; l++) want ^= jptrs[l][(j % k) * m + j / k];
                if (o2.at[j - h] != want) return fail("trimmed join", k, m, links, off);
            }
            cases++;
        }
    }
    printf("%d cases\n", cases);
    return 0;
}
