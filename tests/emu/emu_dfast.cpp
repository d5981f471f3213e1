// tests/emu/emu_dfast.cpp -- the double-fast searches on the host, each behind an entry point of its own: the lane-serial one (ze_dfast), the flat one with two, three and
// four probes a trip on the caller's tables (ze_dfast_flat_np<18, false, NP>), the block form over a frame cut at the caller's block ends (<ZE_MB_POS_BITS, true, NP>, tables
// and repeat offsets carried), the lane-serial block form with a window (ze_dfast_g: the one whose lowest valid index can be above 2), and the
// search of the table-copy mode against a dictionary (ze_dfast_ext). The first four have no cross-lane operation; the dictionary's digestion runs one emulated wave.
// Test infrastructure only (tests/test_emu_dfast.py, tests/test_emu_dfast_mutants.py, and with -DEMU_DFAST_MAIN the sanitizer program at the end); compiled with zhemu.cpp like emu_fast_flat.cpp. ZHIP_DFAST_HEADER names another copy of the encoder header (the mutants test compiles patched copies; never for a GPU).
#define ZHIP_EMU 1
#include <stdint.h>
extern "C" { long zd_trace_pos = -1; long zd_cur_frame = -1; long zd_stat[16]; }
#include "../../python-zstandard_amd/csrc/zhip_decode_pipeline.hpp"      // (zd_clock and friends: the encoder header relies on them, as in emu_kernels.cpp)
#ifdef ZHIP_DFAST_HEADER
#include ZHIP_DFAST_HEADER
#else
#include "../../python-zstandard_amd/csrc/zhip_encode_kernel.hpp"
#endif
#include <string.h>
#include <vector>

// the lane-serial search on zeroed tables of its own. Returns the sequence count; seqs has room for n / 4 + 8.
extern "C" uint32_t emu_dfast_serial(const uint8_t* src, uint32_t n, int hlog, int clog, int mml, uint64_t* seqs)
{
    std::vector<uint32_t> tables(((size_t)1 << hlog) + ((size_t)1 << clog), 0u);
    std::vector<uint8_t> lits((size_t)n + 8);
    ZePar cp; memset(&cp, 0, sizeof cp);
    cp.wlog = 17; cp.hlog = hlog; cp.clog = clog; cp.mml = mml; cp.strat = 2;
    uint32_t lit = 0;
    return ze_dfast(seqs, lits.data(), &lit, src, n, cp, tables.data(), tables.data() + ((size_t)1 << hlog));
}
// the flat search of a one-block source (16 ... 131 072 bytes) on the caller's tables: (1 << hlog) long cells, then (1 << clog) short ones. Cells of earlier launches stay in
// them: `epoch` tells them apart. np = 2, 3, 4 probes a trip.
extern "C" uint32_t emu_dfast_flat(const uint8_t* src, uint32_t n, int hlog, int clog, int mml, int np, uint32_t epoch, uint32_t* tables, uint64_t* seqs)
{
    static uint8_t idlePad[64];
    uint32_t* hashLong = tables; uint32_t* hashSmall = tables + ((size_t)1 << hlog);
    if (np == 4) return ze_dfast_flat_np<18, false, 4>(seqs, src, 0, n, hlog, clog, mml, hashLong, hashSmall, nullptr, idlePad, epoch);
    if (np == 3) return ze_dfast_flat_np<18, false, 3>(seqs, src, 0, n, hlog, clog, mml, hashLong, hashSmall, nullptr, idlePad, epoch);
    return ze_dfast_flat_np<18, false, 2>(seqs, src, 0, n, hlog, clog, mml, hashLong, hashSmall, nullptr, idlePad, epoch);
}
// the block form as ze_match_flat_mb_body drives it: blocks [ends[j - 1], ends[j]) of one frame in order, tables zeroed once, repeat offsets {1, 4} into the first block.
// counts[j] = the block's sequences (they follow each other in seqs); reps[2 * j], reps[2 * j + 1] = the repeat offsets it leaves. np = 2 or 4.
extern "C" uint32_t emu_dfast_blocks(const uint8_t* src, const uint32_t* ends, uint32_t nb, int hlog, int clog, int mml, int np, uint64_t* seqs, uint32_t* counts, uint32_t* reps)
{
    static uint8_t idlePad[64];
    std::vector<uint32_t> tables(((size_t)1 << hlog) + ((size_t)1 << clog), 0u);
    uint32_t* hl = tables.data(); uint32_t* hs = hl + ((size_t)1 << hlog);
    uint32_t rep[2] = {1, 4}, bs = 0, start = 0;
    for (uint32_t j = 0; j < nb; j++) {
        const uint32_t be = ends[j];
        const uint32_t ns = be - bs < 7 ? 0u
                          : np == 4 ? ze_dfast_flat_np<ZE_MB_POS_BITS, true, 4>(seqs + start, src, bs, be, hlog, clog, mml, hl, hs, rep, idlePad)
                                    : ze_dfast_flat_np<ZE_MB_POS_BITS, true, 2>(seqs + start, src, bs, be, hlog, clog, mml, hl, hs, rep, idlePad);
        counts[j] = ns; reps[2 * j] = rep[0]; reps[2 * j + 1] = rep[1];
        start += ns; bs = be;
    }
    return start;
}
// the lane-serial block form (what the generic kernel runs on sources above one block): the same cut, a window of 1 << wlog bytes -- below the frame's size the lowest valid
// index rises above 2 from the second block on.
extern "C" uint32_t emu_dfast_g_blocks(const uint8_t* src, const uint32_t* ends, uint32_t nb, int wlog, int hlog, int clog, int mml, uint64_t* seqs, uint32_t* counts, uint32_t* reps)
{
    std::vector<uint32_t> tables(((size_t)1 << hlog) + ((size_t)1 << clog), 0u);
    uint32_t* hl = tables.data(); uint32_t* hs = hl + ((size_t)1 << hlog);
    ZePar cp; memset(&cp, 0, sizeof cp);
    cp.wlog = wlog; cp.hlog = hlog; cp.clog = clog; cp.mml = mml; cp.strat = 2;
    uint32_t rep[2] = {1, 4}, bs = 0, start = 0;
    for (uint32_t j = 0; j < nb; j++) {
        const uint32_t be = ends[j];
        std::vector<uint8_t> lits((size_t)(be - bs) + 8);
        uint32_t lit = 0;
        const uint32_t ns = be - bs < 7 ? 0u : ze_dfast_g(seqs + start, lits.data(), &lit, src, src + bs, be - bs, cp, hl, hs, rep);
        counts[j] = ns; reps[2 * j] = rep[0]; reps[2 * j + 1] = rep[1];
        start += ns; bs = be;
    }
    return start;
}

// ---- ze_dfast_ext: ZSTD_compressBlock_doubleFast_extDict_generic, what a frame searched in libzstd's table-copy mode runs (a dictionary with content and a source above the
// attach cutoff, or of several blocks). The dictionary is digested by the product's own kernels under emulation, as emu_kernels.cpp does it (zd_dict_body, ze_cdict_body).
#include "../../python-zstandard_amd/csrc/zhip_cparams.hpp"
static ZdLDS g_xlds; static ZeLDS g_xelds;
static std::vector<uint8_t> g_xBlob; static ZhipDictEntropy g_xEntropy; static ZeCDict g_xcd; static std::vector<uint32_t> g_xTables; static ZeRows g_xRows;
static void x_dict_lane(void*) { zd_dict_body(g_xBlob.data(), (uint32_t)(g_xBlob.size() - 16), &g_xEntropy, g_xlds); }
static void x_cdict_lane(void*)
{
    const size_t cells = (size_t)1 << ZE_CDICT_MAX_HLOG;
    ze_cdict_body(g_xBlob.data(), (uint32_t)(g_xBlob.size() - 16), &g_xEntropy, g_xRows, &g_xcd, g_xTables.data(), g_xTables.data() + cells, g_xTables.data() + 2 * cells, g_xelds);
}
// the dictionary of the following emu_dfast_ext calls, digested for `level`. Returns 0 or the error of its digestion.
extern "C" int emu_dfast_ext_dict(const uint8_t* dict, uint32_t size, int level)
{
    g_xBlob.assign(dict, dict + size); g_xBlob.resize((size_t)size + 16, 0);
    memset(&g_xEntropy, 0, sizeof g_xEntropy); memset(&g_xcd, 0, sizeof g_xcd);
    zhemu::run_grid(1, x_dict_lane, nullptr);
    if (g_xEntropy.status) return g_xEntropy.status;
    g_xTables.assign(3 * ((size_t)1 << ZE_CDICT_MAX_HLOG), 0xDEADBEEFu);
    zhip_compression_parameters ov; memset(&ov, 0, sizeof ov);
    zh_resolve_rows(&g_xRows, level, &ov);
    zhemu::run_grid(1, x_cdict_lane, nullptr);
    return g_xcd.status;
}
// the search over the blocks of one frame of n bytes, as ze_compress_block drives it in copy mode: the dictionary's tagged cells copied as plain indices before the first
// block, the dictionary's repeat offsets in, tables and repeat offsets carried. Returns the sequence count, or -status when the parameters are refused.
extern "C" int64_t emu_dfast_ext(const uint8_t* src, uint32_t n, const uint32_t* ends, uint32_t nb, uint64_t* seqs, uint32_t* counts, uint32_t* reps)
{
    ZePar cp; memset(&cp, 0, sizeof cp);
    const int e = ze_dict_copy_cparams(cp, g_xcd, g_xRows, n);
    if (e) return -(int64_t)e;
    if (cp.strat != 2 || !g_xcd.contentSize) return -1000;
    const uint8_t* content = g_xBlob.data() + (g_xEntropy.hufCount ? g_xEntropy.contentOffset : 0u);
    const uint32_t* dl = g_xTables.data(); const uint32_t* dsm = g_xTables.data() + ((size_t)1 << ZE_CDICT_MAX_HLOG);
    std::vector<uint32_t> tables(((size_t)1 << cp.hlog) + ((size_t)1 << cp.clog));
    uint32_t* hl = tables.data(); uint32_t* hs = hl + ((size_t)1 << cp.hlog);
    for (uint32_t i = 0; i < (1u << cp.hlog); i++) hl[i] = dl[i] >> 8;
    for (uint32_t i = 0; i < (1u << cp.clog); i++) hs[i] = dsm[i] >> 8;
    uint32_t rep[2] = {g_xcd.rep[0], g_xcd.rep[1]}, bs = 0, start = 0;
    for (uint32_t j = 0; j < nb; j++) {
        const uint32_t be = ends[j];
        std::vector<uint8_t> lits((size_t)(be - bs) + 8);
        uint32_t lit = 0;
        const uint32_t ns = be - bs < 7 ? 0u : ze_dfast_ext(seqs + start, lits.data(), &lit, src, bs, be - bs, cp, g_xcd, content, hl, hs, rep);
        counts[j] = ns; reps[2 * j] = rep[0]; reps[2 * j + 1] = rep[1];
        start += ns; bs = be;
    }
    return (int64_t)start;
}

#ifdef EMU_DFAST_MAIN
// A stand-alone program for the sanitizers (tests/emu/build_asan.sh): every search above over the aimed sources of tests/golden/dfast_sources.bin
// (python -m tests.dfast_sources --write-fixture: "DFS1", count, then per source n, windowLog, hashLog, chainLog, minMatch, block count, block ends, n bytes;
// all uint32 little-endian). Every source lies in an allocation of exactly its size and every table in one of exactly its cells, so a read or write past either is reported.
// Prints the number of sequences per form: the values are compared by the pytest files, not here.
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s tests/golden/dfast_sources.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t head[2];
    if (fread(head, 4, 2, f) != 2 || head[0] != 0x31534644u) { fprintf(stderr, "not a dfast_sources fixture\n"); return 2; }
    unsigned long long total[7] = {0, 0, 0, 0, 0, 0, 0}, runs = 0;
    for (uint32_t k = 0; k < head[1]; k++) {
        uint32_t h[6];
        if (fread(h, 4, 6, f) != 6) { fprintf(stderr, "short fixture\n"); return 2; }
        const uint32_t n = h[0], nb = h[5]; const int wlog = (int)h[1], hlog = (int)h[2], clog = (int)h[3], mml = (int)h[4];
        std::vector<uint32_t> ends(nb);
        if (fread(ends.data(), 4, nb, f) != nb) { fprintf(stderr, "short fixture\n"); return 2; }
        uint8_t* src = (uint8_t*)malloc(n ? n : 1);
        if (n && fread(src, 1, n, f) != n) { fprintf(stderr, "short fixture\n"); return 2; }
        std::vector<uint64_t> seqs((size_t)n / 4 + 8 * (size_t)nb + 8);
        std::vector<uint32_t> counts(nb), reps(2 * (size_t)nb);
        if (nb == 1) {
            total[0] += emu_dfast_serial(src, n, hlog, clog, mml, seqs.data()); runs++;
            if (n >= 16) for (int np = 2; np <= 4; np++) {
                uint32_t* tables = (uint32_t*)calloc(((size_t)1 << hlog) + ((size_t)1 << clog), 4);
                total[np - 1] += emu_dfast_flat(src, n, hlog, clog, mml, np, (uint32_t)(k % 64), tables, seqs.data()); runs++;
                free(tables);
            }
        }
        if (((uint64_t)1 << wlog) >= n && (nb > 1 || n >= 16)) for (int np = 2; np <= 4; np += 2) { total[3 + np / 2] += emu_dfast_blocks(src, ends.data(), nb, hlog, clog, mml, np, seqs.data(), counts.data(), reps.data()); runs++; }
        total[6] += emu_dfast_g_blocks(src, ends.data(), nb, wlog, hlog, clog, mml, seqs.data(), counts.data(), reps.data()); runs++;
        free(src);
    }
    fclose(f);
    printf("%u sources, %llu runs; sequences: serial %llu, flat %llu %llu %llu, blocks %llu %llu, windowed %llu\n", head[1], runs, total[0], total[1], total[2], total[3], total[4], total[5], total[6]);
    return 0;
}
#endif
