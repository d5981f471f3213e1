// tests/emu/typed_planes_main.cpp -- the stand-alone sanitizer program of the typed seekable kernels (tests/emu/build_asan_planes.sh): the split, join and seal
// bodies of python-zstandard_amd/csrc/zhip_seekable_typed.hpp under the host wave emulator, every buffer a heap allocation of exactly the bytes the kernel may
// touch, at byte offsets 0, 1 and 3 from the allocation -- a read or a write one byte outside is the sanitizer's finding. The results are checked against
// plain loops. Exit 0: every case held. Test infrastructure only.
#include "emu_seekable_typed.cpp"
#include "exact_buffers.hpp"

static inline void zsk_wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

int main()
{
    g_seed = 12345;
    static const uint32_t sizes[] = {1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025}, offsets[] = {0, 1, 3}, ks[] = {2, 4, 8};
    int cases = 0;
    for (uint32_t k : ks) for (uint32_t m : sizes) for (uint32_t off : offsets) {
        // split and whole-buffer join: two groups of m and a shorter last one, on 1 workgroup (the grid-stride loop) and on the library's grid
        const uint64_t elements = 2 * (uint64_t)m + (m > 1 ? m / 3 + 1 : 1), size = elements * k;
        const uint32_t nGroups = (uint32_t)zsk_frame_count(elements, m);
        Exact src(size, off, true), planar(size, (off + 1) % 4, false), back(size, off, false);
        std::vector<uint64_t> records(2 * (size_t)nGroups * k);
        for (uint32_t grid : {1u, emu_typed_grid(1, size, k, m)}) {
            emu_planes_split(src.at, size, k, m, planar.at, grid, records.data());
            for (uint64_t g = 0; g < nGroups; g++) {
                const uint64_t e = zsk_group_len(elements, m, g), base = g * m * k;
                for (uint64_t i = 0; i < e; i++) for (uint32_t p = 0; p < k; p++) if (planar.at[base + p * e + i] != src.at[base + i * k + p]) return fail("split", k, m, off);
                for (uint32_t p = 0; p < k; p++) if (records[2 * (g * k + p)] != base + p * e || records[2 * (g * k + p) + 1] != e) return fail("records", k, m, off);
            }
            emu_planes_join(planar.at, back.at, nullptr, 0, size, k, m, grid);
            if (memcmp(back.at, src.at, (size_t)size)) return fail("join", k, m, off);
            cases++;
        }
        // one job of m elements under every trim pair: the destination holds exactly the bytes that remain
        for (uint32_t h = 0; h < k; h++) for (uint32_t t = 0; t < k; t++) {
            if (k != 4 && !((h == 0 && t == 0) || (h == 1 && t == 0) || (h == 0 && t == 1) || (h == k - 1 && t == k - 1))) continue;
            if ((uint64_t)h + t >= (uint64_t)m * k) continue;
            const uint64_t bytes = (uint64_t)m * k - h - t;
            Exact pl((size_t)m * k, off, true), out(bytes, (off + 2) % 4, false);
            const uint64_t job[5] = {0, m, 0, h, t};
            emu_planes_join(pl.at, out.at, job, 1, 0, k, 1, 2);
            for (uint64_t j = h; j < (uint64_t)m * k - t; j++) if (out.at[j - h] != pl.at[(j % k) * m + j / k]) return fail("trimmed join", k, m, off);
            cases++;
        }
    }
    // the seal: a table of n entries in a buffer that holds exactly the sealed stream, and in one a byte shorter
    for (uint32_t checksum = 0; checksum < 2; checksum++) for (uint32_t n : {0u, 1u, 2u, 5u, 300u}) for (uint32_t shortBy = 0; shortBy < 2; shortBy++) {
        const uint32_t entry = zsk_entry_size((int)checksum);
        const uint64_t frames = 7 * (uint64_t)n, plain = frames + zsk_table_size(n, (int)checksum), sealed = plain + ZSK_MARKER + entry, cap = sealed - shortBy;
        Exact dst(cap, 1, true);
        uint8_t* const table = dst.at + frames;
        zsk_wr32(table, ZSK_SKIP_MAGIC); zsk_wr32(table + 4, n * entry + ZSK_FOOTER);
        for (uint32_t i = 0; i < n; i++) { zsk_wr32(table + 8 + i * entry, 7); zsk_wr32(table + 12 + i * entry, 100 + i); if (checksum) zsk_wr32(table + 16 + i * entry, 0xC0DE0000u + i); }
        uint8_t* const f = table + 8 + (uint64_t)n * entry;
        zsk_wr32(f, n); f[4] = checksum ? 0x80 : 0; zsk_wr32(f + 5, ZSK_SEEK_MAGIC);
        int32_t status[2] = {-1, -1};
        const uint64_t size = emu_typed_seal(dst.at, cap, plain, n, checksum, 4, 4096, 3, status);
        if (shortBy) { if (size || status[0] != ZSK_ERR_DSTSIZE) return fail("seal one byte short", checksum, n, 1); cases++; continue; }
        if (size != sealed) return fail("seal: size", checksum, n, 0);
        uint32_t k = 0, frameSize = 0;
        if (zsk_parse_marker(dst.at + frames, &k, &frameSize) != 1 || k != 4 || frameSize != 4096) return fail("seal: marker", checksum, n, 0);
        ZskLayout lay;
        if (zsk_parse_footer(dst.at + size - ZSK_FOOTER, size, &lay) || lay.n != n + 1 || lay.tableOffset != frames + ZSK_MARKER || zsk_check_header(dst.at + lay.tableOffset, &lay)) return fail("seal: table", checksum, n, 0);
        const uint8_t* const e = dst.at + lay.tableOffset + ZSK_HEADER;
        for (uint32_t i = 0; i < n; i++) if (zsk_rd32(e + i * entry) != 7 || zsk_rd32(e + 4 + i * entry) != 100 + i || (checksum && zsk_rd32(e + 8 + i * entry) != 0xC0DE0000u + i)) return fail("seal: entries", checksum, n, 0);
        if (zsk_rd32(e + n * entry) != ZSK_MARKER || zsk_rd32(e + 4 + n * entry) != 0 || (checksum && zsk_rd32(e + 8 + n * entry) != ZSK_XXH_EMPTY)) return fail("seal: the marker's entry", checksum, n, 0);
        cases++;
    }
    printf("%d cases\n", cases);
    return 0;
}
