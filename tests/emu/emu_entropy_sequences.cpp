// tests/emu/emu_entropy_sequences.cpp -- the entropy kernel driven by explicit sequences, on the host wave emulator: the loader (ze_load_sequences_body), the entropy
// kernel (ze_entropy_body) and the trailer kernel (ze_trailer_body) as zhip_compress_sequences_device launches them. Test infrastructure only
// (tests/test_emu_entropy_sequences.py, tests/stress_emu_entropy_sequences.py); a library of its own beside libzhip_emu.so, built by tests/emu/build.sh, because the
// kernel headers define their functions (compiled with zhemu.cpp like emu_greedy_row.cpp). -DEMU_ENTROPY_SEQUENCES_MAIN adds a main() that runs the cases of a
// fixture file (tests/golden/entropy_sequences.bin: lists and libzstd's frames for them) -- the stand-alone program tests/emu/build_asan.sh builds.
#define ZHIP_EMU 1
#include <stdint.h>
extern "C" { long zd_trace_pos = -1; long zd_cur_frame = -1; long zd_stat[16]; }
#include "../../python-zstandard_amd/csrc/zhip_decode_pipeline.hpp"      // (zd_clock and friends: the encoder header relies on them, as in emu_kernels.cpp)
#include "../../python-zstandard_amd/csrc/zhip_encode_kernel.hpp"
#include "../../python-zstandard_amd/csrc/zhip_cparams.hpp"
#include "../../python-zstandard_amd/csrc/zhip_encode_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static ZeLDS g_elds;
static ZdLDS g_dlds;
// compression dictionary digested by the product's own kernels (as emu_kernels.cpp's emu_set_cdict, which mirrors zhip_ctx_set_cparams)
static std::vector<uint8_t> g_cdBlob; static ZhipDictEntropy g_cdEntropy; static ZeCDict g_cd; static std::vector<uint32_t> g_cdTables;
static bool g_hasCD = false;
static zhip_compression_parameters ov_of(const int32_t* ov)
{
    zhip_compression_parameters o; memset(&o, 0, sizeof o);
    if (ov) { o.windowLog = (uint32_t)ov[0]; o.chainLog = (uint32_t)ov[1]; o.hashLog = (uint32_t)ov[2]; o.searchLog = (uint32_t)ov[3]; o.minMatch = (uint32_t)ov[4]; o.targetLength = (uint32_t)ov[5]; o.strategy = ov[6]; }
    return o;
}
struct DictLaunch { const uint8_t* dict; uint32_t size; ZhipDictEntropy* de; };
static void dict_lane(void* p) { DictLaunch* l = (DictLaunch*)p; zd_dict_body(l->dict, l->size, l->de, g_dlds); }
static void cdict_lane(void* p)
{
    const size_t cells = (size_t)1 << ZE_CDICT_MAX_HLOG;
    ze_cdict_body(g_cdBlob.data(), (uint32_t)(g_cdBlob.size() - 16), &g_cdEntropy, *(const ZeRows*)p, &g_cd, g_cdTables.data(), g_cdTables.data() + cells, g_cdTables.data() + 2 * cells, g_elds);
}
// the dictionary of the following emu_entropy_sequences calls (NULL: none); returns the zstd error code of its digestion. raw: content whatever the first bytes are
extern "C" int emu_seq_set_cdict(const uint8_t* dict, uint32_t size, int level, const int32_t* ov, int raw)
{
    g_hasCD = false;
    if (!dict || !size) return 0;
    g_cdBlob.assign(dict, dict + size); g_cdBlob.resize(size + 16, 0);
    memset(&g_cdEntropy, 0, sizeof g_cdEntropy); memset(&g_cd, 0, sizeof g_cd);
    if (!raw) {
        DictLaunch l = { g_cdBlob.data(), size, &g_cdEntropy };
        zhemu::run_grid(1, dict_lane, &l);
        if (g_cdEntropy.status) return g_cdEntropy.status;
    }
    g_cdTables.assign(3 * ((size_t)1 << ZE_CDICT_MAX_HLOG), 0xDEADBEEFu);
    const zhip_compression_parameters o = ov_of(ov);
    ZeRows rows; zh_resolve_rows(&rows, level, &o);
    zhemu::run_grid(1, cdict_lane, &rows);
    if (g_cd.status) return g_cd.status;
    g_hasCD = true;
    return 0;
}
extern "C" uint32_t emu_seq_dict_rep(int i) { return g_hasCD ? g_cd.rep[i] : (i == 0 ? 1u : i == 1 ? 4u : 8u); }      // the repeat offsets a frame starts from
extern "C" uint32_t emu_seq_capacity(void) { return ZE_ARENA_LIT / 8 - 8; }                                          // sequences a one-block slot holds

struct LoadLaunch { const ZhipEncodeArgs* a; ZeSeqLoad in; };
static void load_lane(void* p) { const LoadLaunch* l = (const LoadLaunch*)p; ze_load_sequences_body(*l->a, l->in); }
static void e2_lane(void* p) { ze_entropy_body(*(const ZhipEncodeArgs*)p, g_elds); }
static void ex_lane(void* p) { ze_trailer_body(*(const ZhipEncodeArgs*)p); }
// ov: the seven explicit fields (0 = unset) laid over `level`'s rows; flags: 1 content size, 2 checksum, 4 dictionary ID, 8 magicless; loadFlags: zhip_compress_sequences_device's
// (bit 0: the loader copies the literals). chunk: sources per launch (0: all). Mirrors zhip_compress_sequences_device.
extern "C" int emu_entropy_sequences(const uint8_t* src, const uint64_t* srcSegs, uint32_t n, const uint64_t* seqs, const uint64_t* seqSegs, uint8_t* dst, const uint64_t* dstSegs,
                                     uint64_t* outSizes, int32_t* status, int level, const int32_t* ov, uint32_t flags, uint32_t loadFlags, uint32_t nBlocks, uint32_t chunk)
{
    ZhipEncodeArgs a; memset(&a, 0, sizeof(a));
    const zhip_compression_parameters o = ov_of(ov);
    uint32_t counters[2] = {0, 0};
    if (chunk == 0 || chunk > n) chunk = n ? n : 1;
    a.src = src; a.srcSegs = srcSegs; a.dst = dst; a.dstSegs = dstSegs; a.outSizes = outSizes; a.status = status;
    a.counter = counters; a.n = n; a.level = level; zh_resolve_rows(&a.rows, level, &o);
    a.contentSizeFlag = flags & 1; a.checksumFlag = (flags >> 1) & 1; a.dictIDFlag = (flags >> 2) & 1; a.magicless = (flags >> 3) & 1;
    if (g_hasCD) {
        a.cdict = &g_cd;
        a.cdictContent = g_cdBlob.data() + (g_cdEntropy.hufCount ? g_cdEntropy.contentOffset : 0u);
        a.cdictHashLong = g_cdTables.data(); a.cdictHashSmall = g_cdTables.data() + ((size_t)1 << ZE_CDICT_MAX_HLOG);
    }
    {   // the slots of the product's plan for this call, without a size hint
        ZePlanIn in; in.rows = a.rows; in.n = n;
        if (g_hasCD) { in.dict.present = true; in.dict.hlog = g_cd.hlog; in.dict.clog = g_cd.clog; in.dict.strat = g_cd.strat; in.dict.contentSize = g_cd.contentSize;
                       in.dict.attachMax = g_cd.strat == 1 ? ZE_DICT_ATTACH_MAX_FAST : ZE_DICT_ATTACH_MAX; }
        const ZeSlotPlan s = ze_sequences_plan(in);
        a.arenaStride = s.arenaStride; a.arenaLit = s.arenaLit; a.slotSrcMax = s.slotSrcMax;
    }
    a.workspace = (uint8_t*)malloc((size_t)nBlocks * ZE_E2_STRIDE + ZHIP_ENC_STRIDE);
    a.meta = (ZeMeta*)malloc((size_t)chunk * sizeof(ZeMeta)); memset(a.meta, 0xA5, (size_t)chunk * sizeof(ZeMeta));
    // exactly the slots, nothing behind them: a write past the last slot is the sanitizer's to see
    a.arena = (uint8_t*)malloc((size_t)chunk * a.arenaStride); memset(a.arena, 0xA5, (size_t)chunk * a.arenaStride);
    static uint8_t idlePad[64]; a.idle = idlePad;
    memset(&g_elds, 0xA5, sizeof g_elds);
    LoadLaunch l; l.a = &a; l.in.seqs = seqs; l.in.table = seqSegs; l.in.copyLits = loadFlags & 1u;
    for (uint32_t first = 0; first < n; first += chunk) {
        a.first = first; a.count = n - first < chunk ? n - first : chunk;
        counters[0] = counters[1] = 0;
        zhemu::run_grid((a.count + 63) / 64, load_lane, &l);
        a.xxLater = a.checksumFlag ? 1u : 0u;
        zhemu::run_grid(nBlocks, e2_lane, &a);
        if (a.xxLater) zhemu::run_grid(nBlocks, ex_lane, &a);
        a.xxLater = 0;
    }
    free(a.workspace); free(a.meta); free(a.arena);
    return 0;
}

#ifdef EMU_ENTROPY_SEQUENCES_MAIN
// The fixture: "ZESQ", u32 cases; per case i32 level, u32 flags, u32 srcSize, u32 nbSeq, i32 wantStatus, u32 wantSize, then the source, the packed sequences, libzstd's frame.
// Every case runs alone (buffers of exactly the sizes the call may touch), on both loader routes; exit status 0 = every frame is libzstd's, byte for byte.
static uint32_t rd_u32(const uint8_t*& p) { uint32_t v; memcpy(&v, p, 4); p += 4; return v; }
int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s FIXTURE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> blob; { uint8_t buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) blob.insert(blob.end(), buf, buf + k); }
    fclose(f);
    const uint8_t* p = blob.data();
    if (blob.size() < 8 || memcmp(p, "ZESQ", 4)) { fprintf(stderr, "not a fixture\n"); return 2; }
    p += 4;
    const uint32_t cases = rd_u32(p);
    int bad = 0; uint32_t ran = 0;
    for (uint32_t c = 0; c < cases; c++) {
        const int level = (int)rd_u32(p); const uint32_t flags = rd_u32(p), srcSize = rd_u32(p), nbSeq = rd_u32(p); const int wantStatus = (int)rd_u32(p); const uint32_t wantSize = rd_u32(p);
        // buffers of exactly the sizes the call may touch
        std::vector<uint8_t> src(p, p + srcSize); p += srcSize;
        std::vector<uint64_t> seqs(nbSeq); if (nbSeq) memcpy(seqs.data(), p, (size_t)nbSeq * 8); p += (size_t)nbSeq * 8;
        const uint8_t* want = p; p += wantSize;
        const uint64_t bound = (uint64_t)srcSize + (srcSize >> 8) + (srcSize < (128u << 10) ? ((128u << 10) - srcSize) >> 11 : 0);
        for (uint32_t route = 0; route < 2; route++) {
            std::vector<uint8_t> dst(bound);
            const uint64_t ss[2] = {0, srcSize}, qs[2] = {0, nbSeq}, ds[2] = {0, bound};
            uint64_t size = ~0ull; int32_t st = -1;
            emu_entropy_sequences(src.data(), ss, 1, seqs.data(), qs, dst.data(), ds, &size, &st, level, nullptr, flags, route, 2, 0);
            ran++;
            if (st != wantStatus || (st == 0 && (size != wantSize || memcmp(dst.data(), want, wantSize)))) {
                fprintf(stderr, "case %u route %u: status %d size %llu, want status %d size %u\n", c, route, st, (unsigned long long)size, wantStatus, wantSize); bad++;
            }
        }
    }
    printf("%u runs of %u cases, %d differ from libzstd\n", ran, cases, bad);
    return bad ? 1 : 0;
}
#endif
