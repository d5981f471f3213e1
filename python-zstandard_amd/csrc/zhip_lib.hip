// zhip_lib.hip -- libzstd_hip.so: C ABI (include/zstd_hip.h) + kernel entry points, compiled for gfx950 only.
//
// Host side = the batch dispatcher that replaces compress_from_datasources / decompress_from_framesources
// (c-ext/compressor.c:1083, c-ext/decompressor.c:1185): instead of partitioning frames over a pthread pool
// (POOL_*, zstd.c:7537-7975) it stages them in HBM and launches persistent one-wave workgroups that pull frame
// indices from an atomic counter.
#include <atomic>
#include <chrono>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <time.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/zstd_hip.h"
#include "zhip_decode_pipeline.hpp"
#include "zhip_encode_kernel.hpp"
#include "zhip_encode_wave.hpp"
#include "zhip_encode_none.hpp"
#include "zhip_cparams.hpp"
#include "zhip_encode_plan.hpp"
#include "zhip_encode_auto.hpp"
#include "zhip_decode_plan.hpp"
#include "zhip_seekable_calls.hpp"
#include "zhip_seekable_typed_calls.hpp"
#include "zhip_host_calls.hpp"
#include "zhip_host_pool.hpp"

#define ZHIP_LDS_BYTES (160u * 1024u)      // per CU on gfx950
static_assert(sizeof(ZpSeqQLDS) <= ZHIP_LDS_BYTES && sizeof(ZpHufKernelLDS) <= ZHIP_LDS_BYTES, "a workgroup's LDS must fit a CU");

// ------------------------------------------------------------------------------------------ kernels
ZH_GLOBAL __launch_bounds__(64, 2) void zhip_decode_frames_kernel(ZhipDecodeArgs a)
{
    __shared__ ZdLDS L;
    zd_kernel_body(a, L);
}
ZH_GLOBAL __launch_bounds__(64, 2) void zhip_decode_lit_kernel(ZhipPipeArgs a)
{
    __shared__ ZdLDS L;
    zp_lit_body(a, L);
}
ZH_GLOBAL __launch_bounds__(64) void zhip_decode_lit_lanes_kernel(ZhipPipeArgs a) { zp_lit_lanes_body(a); }      // K1's lane-per-frame pass over dictionary batches
ZH_GLOBAL __launch_bounds__(64) void zhip_decode_check_kernel(ZhipPipeArgs a) { zp_check_body(a); }      // KX: content checksums, a lane per frame, after K3
ZH_GLOBAL __launch_bounds__(64) void zhip_decode_pre_kernel(ZhipPipeArgs a)           // K0: a lane per frame walks what K1's lane 0 used to (Huffman weights, sequence distributions)
{
    __shared__ ZpPreLDS L;
    zp_pre_body(a, L);
}
ZH_GLOBAL __launch_bounds__(64) void zhip_decode_bin_kernel(ZhipPipeArgs a)
{
    __shared__ ZpBinLDS L;
    zp_bin_body(a, L);
}
ZH_GLOBAL __launch_bounds__(64) void zhip_decode_huf_kernel(ZhipPipeArgs a)
{
    __shared__ ZpHufKernelLDS L;
    zp_huf_body(a, L);
}
ZH_GLOBAL __launch_bounds__(64) void zhip_decode_seq_kernel(ZhipPipeArgs a)           // K2: a quad of lanes per frame, four waves per CU
{
    __shared__ ZpSeqQLDS L;
    zp_seqq_body<false>(a, L);
}
// ---- frames of several blocks (ZpFrameRec in zhip_format.hpp): K1 per frame over its blocks, K2 per block, K3 per frame over its blocks
ZH_GLOBAL __launch_bounds__(64, 2) void zhip_decode_lit_mb_kernel(ZhipPipeArgs a)
{
    __shared__ ZdLDS L;
    zp_lit_mb_body(a, L);
}
ZH_GLOBAL __launch_bounds__(64) void zhip_decode_seq_mb_kernel(ZhipPipeArgs a)
{
    __shared__ ZpSeqQLDS L;
    zp_seqq_body<true>(a, L);
}
#ifndef ZP_K3_MINWAVES
#define ZP_K3_MINWAVES 6         // 77 VGPRs: own-lane items <= 16 bytes (zhip_decode_pipeline.hpp: ZP_LIT_SHORT / ZP_FAR_SHORT, r03g: 113 -> 96) and the phase timers
                                 // in their own instantiation (r03n: 96 -> 77). Six waves per SIMD; seven (72 VGPRs) and eight measured the same
#endif
ZH_GLOBAL __launch_bounds__(64, ZP_K3_MINWAVES) void zhip_decode_exec_kernel(ZhipPipeArgs a)
{
    __shared__ ZpExecLDS L;
    zp_exec_body<false, false>(a, L);
}
ZH_GLOBAL __launch_bounds__(64, 4) void zhip_decode_exec_prof_kernel(ZhipPipeArgs a)      // ZHIP_PROF=1: the same kernel with its phase timers
{
    __shared__ ZpExecLDS L;
    zp_exec_body<false, true>(a, L);
}
#ifndef ZP_K3D_MINWAVES
#define ZP_K3D_MINWAVES 4        // 113 VGPRs since round 3 (round 2: 168 at three waves per SIMD, 208 bytes of spills at four, r02y)
#endif
ZH_GLOBAL __launch_bounds__(64, ZP_K3D_MINWAVES) void zhip_decode_exec_dict_kernel(ZhipPipeArgs a)      // the context has a dictionary
{
    __shared__ ZpExecLDS L;
    zp_exec_body<true, false>(a, L);
}
ZH_GLOBAL __launch_bounds__(64, 4) void zhip_decode_exec_mb_kernel(ZhipPipeArgs a)
{
    __shared__ ZpExecLDS L;
    zp_exec_body<false, false, true>(a, L);
}
ZH_GLOBAL __launch_bounds__(64, 4) void zhip_decode_exec_mb_dict_kernel(ZhipPipeArgs a)
{
    __shared__ ZpExecLDS L;
    zp_exec_body<true, false, true>(a, L);
}
ZH_GLOBAL __launch_bounds__(64, 3) void zhip_encode_frames_kernel(ZhipEncodeArgs a)
{
    __shared__ ZeLDS L;
    __shared__ ZeLDSMulti M;
    ze_kernel_body(a, L, M);
}
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_match_kernel(ZhipEncodeArgs a) { ze_match_body(a); }
// the greedy strategy's search (ze_greedy_row: level 5 on sources of 16 385 ... 131 072 bytes), lane-serial like the kernel above and launched in its place: a kernel of its own, that one is untouched
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_match_greedy_kernel(ZhipEncodeArgs a) { ze_match_body<true>(a); }
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_split_kernel(ZhipEncodeArgs a)          // block layout of sources of several blocks for the flat match kernel
{
    __shared__ ZeLDS L;
    ze_split_body(a, L);
}
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_trailer_kernel(ZhipEncodeArgs a) { ze_trailer_body(a); }      // EX: checksum trailers, a lane per frame, after E2
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_load_sequences_kernel(ZhipEncodeArgs a, ZeSeqLoad in) { ze_load_sequences_body(a, in); }      // zhip_compress_sequences_device: in place of the match kernels
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_match_flat_kernel(ZhipEncodeArgs a) { ze_match_flat_body<2>(a); }
// four probes per trip: chunks small enough to be bound by a source's serial chain rather than by the memory system (ze_dfast_flat_np)
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_match_flat4_kernel(ZhipEncodeArgs a) { ze_match_flat_body<4>(a); }
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_match_flat3_kernel(ZhipEncodeArgs a) { ze_match_flat_body<3>(a); }      // three probes: launches of up to 65 536 sources
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_match_flat_mb_kernel(ZhipEncodeArgs a) { ze_match_flat_mb_body(a); }
// the fast strategy's flat search (ze_fast_flat_np), one and two pairs of the reference's loop per trip: kernels of their own, the double-fast ones are untouched
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_match_flat_fast_kernel(ZhipEncodeArgs a) { ze_match_flat_body<1, true>(a); }
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_match_flat_fast2_kernel(ZhipEncodeArgs a) { ze_match_flat_body<2, true>(a); }
static_assert(sizeof(ZeSrcLDS<ZF_BLOCK_MAX>) <= ZHIP_LDS_BYTES, "a workgroup's LDS must fit a CU");
template <uint32_t BYTES, int NPROBE> __global__ __launch_bounds__(64) void zhip_encode_match_lds_kernel(ZhipEncodeArgs a)
{
    __shared__ ZeSrcLDS<BYTES> L;
    ze_match_lds_body<NPROBE>(a, L.b, BYTES);
}
template <uint32_t BYTES, int NPAIR> __global__ __launch_bounds__(64) void zhip_encode_match_lds_fast_kernel(ZhipEncodeArgs a)      // the fast strategy's search on a source in LDS
{
    __shared__ ZeSrcLDS<BYTES> L;
    ze_match_lds_body<NPAIR, true>(a, L.b, BYTES);
}
// the wave-parallel match finder (ZHIP_FINDER_WAVE, zhip_encode_wave.hpp): one wave per source, 1 << H table cells in LDS -- 16 / 32 / 64 KiB a workgroup
template <int H> __global__ __launch_bounds__(64) void zhip_encode_match_wave_kernel(ZhipEncodeArgs a)
{
    __shared__ uint32_t table[1u << H];
    ze_match_wave_body<H>(a, table);
}
// no match search (ZHIP_FINDER_NONE, zhip_encode_none.hpp): literals-only frames, one wave per source, launched once per chunk in place of BOTH the match and the entropy kernel
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_none_kernel(ZhipEncodeArgs a)
{
    __shared__ ZeLDS L;
    ze_none_body(a, L);
}
// the match finder chosen per source (ZHIP_FINDER_AUTO, zhip_encode_auto.hpp): the classifier, one wave per source, and the three small kernels of the split
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_classify_kernel(ZhipClassifyArgs a)
{
    __shared__ ZaLDS L;
    ze_classify_body(a, L);
}
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_auto_partition_kernel(ZhipSplitArgs a) { ze_auto_partition_body(a); }
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_auto_gather_kernel(ZhipSplitArgs a) { ze_auto_gather_body(a); }
ZH_GLOBAL __launch_bounds__(64) void zhip_encode_auto_scatter_kernel(ZhipSplitArgs a) { ze_auto_scatter_body(a); }
#ifndef ZHIP_WAVE_HLOG
#define ZHIP_WAVE_HLOG 12                  // table cells of the wave match finder, log2: 12 by the rate measurement (profiles/r11_wave_finder_rate.txt, DESIGN.md 4.2 -- the kernel's rate is its resident
                                           // waves, which LDS bounds: 16 384 x 128 KiB 77 / 140 / 174 ms at 12 / 13 / 14). ZHIP_WAVE_HLOG in the environment overrides it FOR THAT MEASUREMENT ONLY
                                           // (tests/tools/wave_finder_rate.py): the frames differ with the table size, so a process that sets it gives up "the same bytes everywhere"
#endif
#ifndef ZE_E2_MINWAVES
#define ZE_E2_MINWAVES 4
#endif
ZH_GLOBAL __launch_bounds__(64, ZE_E2_MINWAVES) void zhip_encode_entropy_kernel(ZhipEncodeArgs a)
{
    __shared__ ZeLDS L;
    ze_entropy_body(a, L);
}
ZH_GLOBAL __launch_bounds__(64) void zhip_build_cdict_kernel(const uint8_t* dict, uint32_t dictSize, const ZhipDictEntropy* de, ZeRows rows,
                                                              ZeCDict* cd, uint32_t* hashLong, uint32_t* hashSmall, uint32_t* tmpLong)
{
    __shared__ ZeLDS L;
    ze_cdict_body(dict, dictSize, de, rows, cd, hashLong, hashSmall, tmpLong, L);
}
ZH_GLOBAL void zhip_selftest_kernel(uint32_t* out)
{
    uint32_t v = zh_scan_add(zh_lane());                  // 0+1+..+lane
    uint64_t m = zh_ballot((zh_lane() & 1) != 0);
    out[zh_lane()] = v + (uint32_t)zh_popc64(m) + zh_shfl(zh_lane(), 63) + zh_first(zh_lane() + 7);
}
ZH_GLOBAL __launch_bounds__(64) void zhip_dict_tables_kernel(const ZhipDictEntropy* de, ZhipDictTables* out)
{
    __shared__ ZdLDS L;
    zp_dict_tables_body(de, out, L);
}
ZH_GLOBAL __launch_bounds__(64) void zhip_parse_dict_kernel(const uint8_t* dict, uint32_t dictSize, ZhipDictEntropy* de)
{
    __shared__ ZdLDS L;
    zd_dict_body(dict, dictSize, de, L);
}

// ------------------------------------------------------------------------------------------ errors
static thread_local std::string g_lastError;
static int hip_fail(hipError_t e, const char* what)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    g_lastError = buf;
    return ZHIP_ERR_HIP;
}
#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return hip_fail(e_, #x); } while (0)

extern "C" const char* zhip_last_error(void) { return g_lastError.c_str(); }
extern "C" int zhip_abi_version(void) { return ZHIP_ABI_VERSION; }
extern "C" int zhip_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { hip_fail(e, "hipGetDeviceCount"); return 0; }
    return n;
}
extern "C" int zhip_set_device(int d) { HIP_TRY(hipSetDevice(d)); return 0; }
extern "C" size_t zhip_compress_bound(size_t n) { return host_compress_bound(n); }

extern "C" const char* zhip_error_name(int code)
{
    switch (code) {   // strings of ERR_getErrorString, zstd.c:3580-3616
    case ZE_OK: return "No error detected";
    case ZE_GENERIC: return "Error (generic)";
    case ZE_PREFIX_UNKNOWN: return "Unknown frame descriptor";
    case ZE_FRAMEPARAM_UNSUPPORTED: return "Unsupported frame parameter";
    case ZE_WINDOW_TOO_LARGE: return "Frame requires too much memory for decoding";
    case ZE_CORRUPTION: return "Data corruption detected";
    case ZE_CHECKSUM_WRONG: return "Restored data doesn't match checksum";
    case ZE_LITERALS_HEADER_WRONG: return "Header of Literals' block doesn't respect format specification";
    case ZE_DICT_CORRUPTED: return "Dictionary is corrupted";
    case ZE_DICT_WRONG: return "Dictionary mismatch";
    case ZE_PARAM_UNSUPPORTED: return "Unsupported parameter";
    case ZE_PARAM_OUTOFBOUND: return "Parameter is out of bound";
    case ZE_TABLELOG_TOO_LARGE: return "tableLog requires too much memory : unsupported";
    case ZE_MAXSYMBOL_TOO_LARGE: return "Unsupported max Symbol Value : too large";
    case ZE_MAXSYMBOL_TOO_SMALL: return "Specified maxSymbolValue is too small";
    case ZE_MEMORY: return "Allocation error : not enough memory";
    case ZE_DST_TOO_SMALL: return "Destination buffer is too small";
    case ZE_SRC_SIZE_WRONG: return "Src size is incorrect";
    case ZE_SEQ_INVALID: return "External sequences are not valid";
    default: return "Unspecified error code";
    }
}

// ------------------------------------------------------------------------------------------ frame inspection (host: zhip_host_calls.hpp)
extern "C" uint64_t zhip_frame_content_size_format(const void* src, size_t n, int format) { return host_frame_content_size((const uint8_t*)src, n, format); }
extern "C" uint64_t zhip_frame_content_size(const void* src, size_t n) { return zhip_frame_content_size_format(src, n, ZHIP_FORMAT_ZSTD1); }
extern "C" int64_t zhip_find_frame_compressed_size_format(const void* src, size_t n, int format) { return host_frame_compressed_size((const uint8_t*)src, n, format); }
extern "C" int64_t zhip_find_frame_compressed_size(const void* src, size_t n) { return zhip_find_frame_compressed_size_format(src, n, ZHIP_FORMAT_ZSTD1); }
extern "C" void zhip_get_cparams(int level, uint64_t srcSizeHint, size_t dictSize, zhip_compression_parameters* out) { if (out) zh_get_cparams(level, srcSizeHint, dictSize, out); }

// ------------------------------------------------------------------------------------------ context
#ifndef ZHIP_E1LDS_PROBES
#define ZHIP_E1LDS_PROBES 2       // probes per trip of the LDS-source match kernel (small batches: one source per CU)
#endif
#ifndef ZHIP_E1LDS_FAST_PAIRS
#define ZHIP_E1LDS_FAST_PAIRS 2   // pairs per trip of the fast strategy's LDS-source match kernel: one source per CU is pure latency, and the second pair's loads ride in the same rounds
#endif
#ifndef ZHIP_TRAILER_LATER
#define ZHIP_TRAILER_LATER 1     // compress: checksum trailers by EX after the entropy kernel; 0: by the entropy kernel on one lane per frame (A/B build)
#endif
#ifndef ZHIP_PICK_MIN
#define ZHIP_PICK_MIN 16384       // sources per launch from which a context's first flat-search launch picks its tables' placement (49 152 while a probe was a whole launch: with probes at ~9 ms per
                                  // 16 384 sources the host-buffer API's chunks of 32 768 pick too -- multi_compress_to_buffer of 65 536 x 128 KiB 12.4-13.5 -> 13.5-13.9 GB/s in five alternating pairs, r06zzt)
#endif
#ifndef ZHIP_PICK_CANDIDATES
#define ZHIP_PICK_CANDIDATES 8     // table allocations the placement pick probes (3, up to 6 when alike, until r06zzv)
#endif
#ifndef ZHIP_PICK_STUDY
#define ZHIP_PICK_STUDY 0        // 1: DIAGNOSTIC build -- the placement pick also times eight candidate allocations whole and over the sources' first bytes, and prints them
#endif
static thread_local int g_reserveRc = ZHIP_ERR_HIP;      // why the last failed DevBuf::reserve failed (ZHIP_ERR_NO_MEMORY or ZHIP_ERR_HIP)
// (device bytes are accounted per CONTEXT -- zhip_ctx::device_bytes sums its buffers -- not in a thread-local counter: a context may be
// destroyed, or grown, on another thread than the one that created it, and a counter that is decremented where it was never incremented
// wraps)
struct DevBuf {
    void* p = nullptr; size_t cap = 0;
    uint64_t gen = 0;            // which allocation this is, process-wide (a released buffer's address may come back with other contents: whoever remembers something ABOUT the contents remembers this too)
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }     // (the owner waits for the device first: zhip_ctx_destroy synchronises, and hipFree itself waits)
    int reserve(size_t n) {
        if (n <= cap) return 0;
        release();
        size_t want = n + (n >> 3) + 4096;
        if (want < n) { g_lastError = "allocation size overflow"; return g_reserveRc = ZHIP_ERR_NO_MEMORY; }
        const hipError_t e = hipMalloc(&p, want);
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); p = nullptr; g_lastError = "out of device memory"; return g_reserveRc = ZHIP_ERR_NO_MEMORY; }
        if (e != hipSuccess) { p = nullptr; return g_reserveRc = hip_fail(e, "hipMalloc"); }
        static std::atomic<uint64_t> g_gen{0};
        cap = want; gen = ++g_gen; return 0;
    }
    int reserve_exact(size_t bytes)      // at exactly its bytes, no head-room (areas as large as what a caller asked to read)
    {
        if (bytes <= cap) return 0;
        release();
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); g_lastError = "out of device memory"; return ZHIP_ERR_NO_MEMORY; }
        cap = bytes;
        return 0;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
};
// pinned host memory, owned: reserve(n, 3) keeps n / 8 of head-room (the staging slots), reserve(n, 2) n / 4 (the small meta area, the seekable calls' slots)
struct PinBuf {
    void* p = nullptr; size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { release(); }
    hipError_t reserve(size_t n, int headroomShift)
    {
        if (n <= cap) return hipSuccess;
        release();
        const size_t want = n + (n >> headroomShift) + 4096;
        const hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);      // (write-combined / non-coherent staging: no difference, profiles/r05zb_*)
        if (e != hipSuccess) p = nullptr; else cap = want;
        return e;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
    }
};
#define ZHIP_NTIMER 13
struct KTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;   // owned: destroyed after reading
    std::vector<std::pair<hipEvent_t, hipEvent_t>> shared;    // borrowed: another timer owns the events
    double totalMs = 0; uint64_t launches = 0;
};

// pinned memory a host table is uploaded from: written again only after the event behind its upload has completed (zsk_take_slot)
// (whoever owns slots waits for the device before they go: neither a slot's memory nor its event is in flight then)
struct ZskPinSlot {
    hipEvent_t done = nullptr; PinBuf pin;
    ZskPinSlot() = default;
    ZskPinSlot(const ZskPinSlot&) = delete;
    ~ZskPinSlot() { if (done) (void)hipEventDestroy(done); }
};

// Every device buffer of a context, ONCE: X(member, trimmable). The members are declared from this list, device_bytes() sums it, tls_trim picks from it, and each
// DevBuf releases itself when the context goes. trimmable = 1: a working area the host-buffer calls give back above the keep limit -- the 14 that tls_trim has
// always named, in its order (ties go to the earlier one): pipeMeta pipeLit pipeFse pipeHuf pipeBases encArena encTables encFlatTables encWorkspace encBigWs scratch
// hSrc hDst hDense. The rest is small or holds state a later call relies on (counters, dictionaries, lists).
#define ZHIP_CTX_DEVBUFS(X) \
    /* decode pipeline */ \
    X(pipeMeta, 1) X(pipeLit, 1) X(pipeCounters, 0) X(pipeFallback, 0) X(pipeFse, 1) X(pipeOrder, 0) X(pipeHuf, 1) X(pipeOrderLit, 0) X(pipeItemFrame, 0) X(pipeItemReps, 0) \
    X(pipeFrameRecs, 0) X(pipeBases, 1) X(pipePre, 0) \
    /* encode */ \
    X(encArena, 1) X(encTables, 1) X(encFlatTables, 1) X(encWorkspace, 1) X(encBigWs, 1) X(encMeta, 0) X(encBigList, 0) X(encE1List, 0) X(encMbBlocks, 0) X(encMbCount, 0) X(encMbSeqs, 0) X(encAuto, 0) \
    X(scratch, 1) X(counter, 0) \
    /* dictionary, compress side: raw bytes, parsed entropy section, digested form and its tagged tables; decode side */ \
    X(cdictBlob, 0) X(cdictEntropy, 0) X(cdictDigest, 0) X(cdictTables, 0) X(dictBlob, 0) X(dictEntropy, 0) X(dictTables, 0) \
    /* host-API staging */ \
    X(hSrc, 1) X(hDst, 1) X(hDense, 1) X(hSegs, 0) X(hStatus, 0) \
    /* seekable streams: the chunks' compressBound-sized slots; segments, sizes, statuses and the scan's cells; the delta join on its own (a uint64 per tile) */ \
    X(skSlots, 0) X(skMeta, 0) X(skTileSums, 0) \
    /* typed seekable compress: the planar copy of the source (its bytes), the plane frames' records, the seal's stash */ \
    X(skStaging, 0) X(skRecords, 0) X(skStash, 0)

struct zhip_ctx {
    int device = 0;
    int numCU = 0;
    int decBlocksPerCU = 0;
    int encBlocksPerCU = 0;
    int k1PerCU = 0, k3PerCU = 0;
#define ZHIP_X(name, trim) DevBuf name;
    ZHIP_CTX_DEVBUFS(ZHIP_X)
#undef ZHIP_X
    hipStream_t slotStream[ZHIP_NSLOT] = {};
    hipStream_t sideStream[ZHIP_NSLOT] = {};
    int e1PerCU = 0, e2PerCU = 0;
    int matchFinder = ZHIP_FINDER_LIBZSTD;     // zhip_ctx_set_match_finder
    int classifyPerCU = 0;             // resident workgroups per CU of the classify kernel (ZHIP_FINDER_AUTO)
    int wavePerCU[3] = {0, 0, 0};      // resident workgroups per CU of the wave match kernel at H = 12, 13, 14
    size_t srcMaxHint = 0;             // largest source of the batch being launched when the caller knows it (host-buffer API), else 0
    size_t itemHint = 0;               // zhip_ctx_set_size_hint: what a device-API caller says about its items' uncompressed sizes (0 = nothing)
    zhip_cparams cparams = {3, 1, 0, 1, nullptr, 0, 0, 0, {0, 0, 0, 0, 0, 0, 0}};
    ZeRows rows = {};                  // cparams resolved per source-size class (zhip_cparams.hpp)
    // dictionary (compress side)
    bool hasCDict = false; uint32_t cdictContentOffset = 0, cdictAttachMax = ZE_DICT_ATTACH_MAX; int cdictHlog = 0, cdictClog = 0, cdictStrat = 2;
    uint32_t cdictContentSize = 0;
    // launch numbers in the cells of the flat dictionary search's tables (ZhipEncodeArgs.tabEpoch): the last one used on the allocation at encEpochPtr, the index width and
    // dictionary it was counted for -- any of them changing, or the numbers running out, zeroes the allocation and starts again at 1
    uint32_t encEpoch = 0, encEpochShift = 0; void* encEpochPtr = nullptr; uint64_t encEpochKey = 0, encEpochGen = 0; size_t encEpochBytes = 0;      // (encEpochBytes: how much of the allocation has been zeroed -- a larger batch that still fits the allocation reaches slots that never were)
    uint64_t cdictKey = 0, ddictKey = 0;     // fingerprint of the dictionary currently digested (skip re-digesting per call)
    // dictionary (decode side)
    uint32_t dictSize = 0, dictID = 0, dictContentOffset = 0; bool dictHasEntropy = false;
    uint64_t maxWindowSize = (1ull << 27) + 1;
    int dformat = ZHIP_FORMAT_ZSTD1;
    // host-API staging
    std::deque<ZskPinSlot> skPins;     // the pick list of an edit without an opened stream travels through these
    PinBuf pinned;                     // small pinned area for per-item sizes / status / chunk totals coming back
    bool hpReady = false; hipStream_t hpH2D = nullptr, hpCompute = nullptr, hpD2H = nullptr;     // host pipeline: copy-in, kernels, copy-out
    PinBuf hpStage[2]; hipEvent_t hpStageFree[2] = {nullptr, nullptr}; int hpNextSlot = 0;
    // bring-up / tuning knobs, read from the environment ONCE when the context is created (never in a launch path)
    struct Knobs : ZeEncodeKnobs, ZdDecodeKnobs {      // (the knobs the launch plans read: ZeEncodeKnobs, zhip_encode_plan.hpp; ZdDecodeKnobs, zhip_decode_plan.hpp)
        // bring-up aids
        bool prof = false;                  // ZHIP_PROF: the kernels' phase timers (a separate instantiation of K3; printed to stderr)
        // encode (the rest: ZeEncodeKnobs)
        int waveH = ZHIP_WAVE_HLOG;         // ZHIP_WAVE_HLOG: table cells of the wave match finder, log2 (12, 13, 14)
        bool e1fPick = true;                // ZHIP_E1F_PICK=0: take the flat tables where the first allocation put them (zhip_compress_batch_device)
        // host-buffer pipeline
        size_t hchunkE = 32768, hchunkE0 = 0;   // compress: items per chunk, items of the first chunk (0: like the others)
        size_t hchunkD0 = 2048;             // decompress: items of the first chunk of batches above 8 192 (0: like the others)
        unsigned packThreads = 0;           // host threads packing items into the pinned staging slots (0: ZHIP_PACK_THREADS)
    } knob;
    size_t flatMaxCached = 0;                    // frames per launch of the flat match kernel for batches above 65 536 (0: not decided yet)
    bool e1fPicked = false; float e1fPickMs[3] = {0, 0, 0}; int e1fPickKept = 0; void* e1fPickedPtr = nullptr;      // the flat match kernel's tables: placement picked once per context (zhip_compress_batch_device)
    bool timing = false;                         // per-kernel HIP-event timers: off until zhip_ctx_kernel_time() is first called
    unsigned long long* profDecode = nullptr;    // ZHIP_PROF phase-timer accumulators, owned by the context (one context == one caller)
    unsigned long long* profPipe = nullptr;
    unsigned long long* profEncode = nullptr;
    KTimer timer[ZHIP_NTIMER];   // (10: the wave match kernel, 11: the literals-only kernel of ZHIP_FINDER_NONE, 12: the classify kernel of ZHIP_FINDER_AUTO) 0 fused decode, 1 fused encode, 2 K1 literals, 3 K2 sequences, 4 K3 execution, 5 E1 match, 6 E2 entropy, 7 K1b Huffman streams, 8 the flat match kernel, 9 the decode pipeline of a chunk from K1's start to K3's end (K1b runs beside K2)
    size_t device_bytes() const
    {
        size_t n = 0;
#define ZHIP_X(name, trim) n += name.cap;
        ZHIP_CTX_DEVBUFS(ZHIP_X)
#undef ZHIP_X
        return n;
    }
    zhip_ctx() = default;
    zhip_ctx(const zhip_ctx&) = delete;
    // what no member owns by itself: streams, the staging slots' events, the phase-timer accumulators. zhip_ctx_destroy has synchronised the device before this runs, so
    // neither these nor the buffers and pinned areas that release themselves after it are in flight
    ~zhip_ctx()
    {
        for (hipStream_t s : slotStream) if (s) (void)hipStreamDestroy(s);
        for (hipStream_t s : sideStream) if (s) (void)hipStreamDestroy(s);
        for (hipStream_t s : {hpH2D, hpCompute, hpD2H}) if (s) (void)hipStreamDestroy(s);
        for (hipEvent_t e : hpStageFree) if (e) (void)hipEventDestroy(e);
        for (unsigned long long* q : {profDecode, profPipe, profEncode}) if (q) (void)hipFree(q);
    }
};

extern "C" zhip_ctx* zhip_ctx_create(void)
{
    zhip_ctx* c = new zhip_ctx();
    if (hipGetDevice(&c->device) != hipSuccess) { g_lastError = "hipGetDevice failed (no GPU?)"; delete c; return nullptr; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) { g_lastError = "hipGetDeviceProperties failed"; delete c; return nullptr; }
    c->numCU = prop.multiProcessorCount;
    {   zhip_ctx::Knobs& k = c->knob;
        // Run-time knobs (round 6: nine, ten with round 7's ZHIP_FAST_PAIRS, each exercised by a GPU test or a resource policy; rounds 1-5's other twenty-two -- chunk shapes, probe counts, waves per CU,
        // bring-up aids -- are the constants of this struct, and what lost its A/B is in DESIGN.md with its measurements): ZHIP_PROF (phase timers), ZHIP_K0_MIN, ZHIP_E1F_PICK,
        // ZHIP_E1LDS_MAX, ZHIP_MBC_MIN, ZHIP_FAST_PAIRS here; ZHIP_DEVICES / ZHIP_DEVICE_MIN_BYTES (the in-call device fan-out), ZHIP_KEEP_GB, ZHIP_PIN_POOL_KEEP_MB (memory kept between
        // calls) where they are used.
        k.prof = getenv("ZHIP_PROF") != nullptr;
        if (const char* e = getenv("ZHIP_K0_MIN")) k.k0Min = (size_t)atol(e);
        if (const char* e = getenv("ZHIP_MBC_MIN")) k.mbcMin = (size_t)atol(e);     // compress: batches of at least this many sources take the flat search for sources of several blocks
        if (const char* e = getenv("ZHIP_E1LDS_MAX")) { const long v = atol(e); if (v >= 0 && v <= 65536) k.e1LdsMax = v; }
        if (const char* e = getenv("ZHIP_E1F_PICK")) k.e1fPick = atol(e) != 0;    // 0: take the tables where the first allocation put them (A/B)
        if (const char* e = getenv("ZHIP_FAST_PAIRS")) { const long v = atol(e); if (v >= 0 && v <= 2) k.fastPairs = (int)v; }      // pairs per trip of the flat fast-strategy search (0: by launch size)
        if (const char* e = getenv("ZHIP_WAVE_HLOG")) { const long v = atol(e); if (v >= 12 && v <= 14) k.waveH = (int)v; }      // MEASUREMENT ONLY (tests/tools/wave_finder_rate.py): table size of the wave match finder -- the frames differ with it
    }
    zh_resolve_rows(&c->rows, 3, nullptr);
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, zhip_decode_frames_kernel, 64, 0) != hipSuccess || nb < 1) nb = 8;
    c->decBlocksPerCU = nb;
    nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, zhip_encode_frames_kernel, 64, 0) != hipSuccess || nb < 1) nb = 4;
    c->encBlocksPerCU = nb;
    nb = 0; if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, zhip_decode_lit_kernel, 64, 0) != hipSuccess || nb < 1) nb = 8;
    c->k1PerCU = nb;
    nb = 0; if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, zhip_decode_exec_kernel, 64, 0) != hipSuccess || nb < 1) nb = 16;
    c->k3PerCU = nb;
    nb = 0; if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, zhip_encode_match_kernel, 64, 0) != hipSuccess || nb < 1) nb = 4;
    c->e1PerCU = nb;
    nb = 0; if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, zhip_encode_entropy_kernel, 64, 0) != hipSuccess || nb < 1) nb = 4;
    c->e2PerCU = nb;
    nb = 0; if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, zhip_encode_match_wave_kernel<12>, 64, 0) != hipSuccess || nb < 1) nb = 8;
    c->wavePerCU[0] = nb;
    nb = 0; if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, zhip_encode_match_wave_kernel<13>, 64, 0) != hipSuccess || nb < 1) nb = 4;
    c->wavePerCU[1] = nb;
    nb = 0; if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, zhip_encode_match_wave_kernel<14>, 64, 0) != hipSuccess || nb < 1) nb = 2;
    c->wavePerCU[2] = nb;
    nb = 0; if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, zhip_encode_classify_kernel, 64, 0) != hipSuccess || nb < 1) nb = 8;
    c->classifyPerCU = nb;
    return c;
}
static void drain_shared(KTimer& t)
{
    for (auto& pr : t.shared) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { t.totalMs += ms; t.launches++; }
    }
    t.shared.clear();
}
static void drain_timer(KTimer& t)
{
    drain_shared(t);
    for (auto& pr : t.pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { t.totalMs += ms > 0 ? ms : 0; t.launches++; }
        (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second);
    }
    t.pending.clear();
}
extern "C" void zhip_ctx_destroy(zhip_ctx* c)
{
    if (!c) return;
    (void)hipDeviceSynchronize();
    for (int i = 0; i < ZHIP_NTIMER; i++) drain_shared(c->timer[i]);
    for (int i = 0; i < ZHIP_NTIMER; i++) drain_timer(c->timer[i]);
    delete c;
}
extern "C" const char* zhip_kernel_name(int k)
{
    static const char* names[ZHIP_NTIMER] = {"zhip_decode_frames_kernel", "zhip_encode_frames_kernel", "zhip_decode_lit_kernel",
                                   "zhip_decode_seq_kernel", "zhip_decode_exec_kernel", "zhip_encode_match_kernel",
                                   "zhip_encode_entropy_kernel", "zhip_decode_huf_kernel", "zhip_encode_match_flat_kernel", "zhip_decode_pipeline_span",
                                   "zhip_encode_match_wave_kernel", "zhip_encode_none_kernel", "zhip_encode_classify_kernel"};
    return k >= 0 && k < ZHIP_NTIMER ? names[k] : "";
}
extern "C" int zhip_ctx_kernel_time(zhip_ctx* c, int direction, double* avgMs, uint64_t* launches)
{
    if (!c || direction < 0 || direction >= ZHIP_NTIMER) return ZHIP_ERR_UNSUPPORTED;
    c->timing = true;                           // from now on the launches of this context are bracketed by events
    HIP_TRY(hipDeviceSynchronize());
    for (int i = 0; i < ZHIP_NTIMER; i++) drain_shared(c->timer[i]);
    KTimer& t = c->timer[direction];
    drain_timer(t);
    if (avgMs) *avgMs = t.launches ? t.totalMs / (double)t.launches : 0.0;
    if (launches) *launches = t.launches;
    t.totalMs = 0; t.launches = 0;
    return 0;
}

extern "C" int zhip_ctx_decode_fallbacks(zhip_ctx* c, uint64_t* frames)
{
    if (!c || !frames) return ZHIP_ERR_UNSUPPORTED;
    *frames = 0;
    if (!c->pipeCounters.p) return 0;             // no decompress call yet
    HIP_TRY(hipDeviceSynchronize());
    uint32_t v = 0;
    HIP_TRY(hipMemcpy(&v, c->pipeCounters.p, sizeof v, hipMemcpyDeviceToHost));      // word 0 of the pipeline's counters: the fallback list's length
    *frames = v;
    return 0;
}

extern "C" int zhip_ctx_table_pick(zhip_ctx* c, float* ms3)
{
    if (!c) return 0;
    if (ms3) for (int k = 0; k < 3; k++) ms3[k] = c->e1fPickMs[k];
    return c->e1fPickKept;
}

static uint64_t dict_fingerprint(const void* p, size_t n, uint64_t salt)
{
    uint64_t h = 0xcbf29ce484222325ull ^ salt;
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
    h ^= (uint64_t)n * 0x9E3779B97F4A7C15ull;
    return h ? h : 1;
}
extern "C" int zhip_ctx_set_ddict(zhip_ctx* c, const void* hostDict, size_t dictSize, int dictType)
{
    if (!c) return ZHIP_ERR_UNSUPPORTED;
    if (dictType != ZHIP_DICT_AUTO && dictType != ZHIP_DICT_RAWCONTENT && dictType != ZHIP_DICT_FULLDICT) { g_lastError = "invalid dictionary type"; return ZHIP_ERR_UNSUPPORTED; }
    if (hostDict && dictSize) {
        const uint64_t key = dict_fingerprint(hostDict, dictSize, 0x100u + (uint64_t)dictType);
        if (c->dictSize == dictSize && c->ddictKey == key) return 0;       // same dictionary as last time: tables are still resident
        c->ddictKey = key;
    } else c->ddictKey = 0;
    c->dictSize = 0; c->dictID = 0; c->dictContentOffset = 0; c->dictHasEntropy = false;
    if (!hostDict || !dictSize) return 0;
    // (the decode kernels pack an offset in 29 bits and keep the values from ZP_OF_LIMIT = 480 MiB up for other purposes: dictionary + one
    // frame's window must stay below that for "offset beyond everything decoded so far" to be decidable from the packed value --
    // zhip_decode_pipeline.hpp, K2. The limit is set at 256 MiB, half of it, leaving the other half to the frames' own windows (up to 2^27
    // here); the reference takes any size: larger dictionaries are refused loudly, INTEGRATION.md section 4 lists the limit)
    if (dictSize >= (256u << 20)) { g_lastError = "dictionary too large"; c->ddictKey = 0; return ZHIP_ERR_UNSUPPORTED; }
    // ZSTD_loadEntropy_intoDDict (zstd.c:42716): raw content when asked for, when shorter than 8 bytes or when the magic is absent --
    // unless a full dictionary was demanded, which is then "Dictionary is corrupted"
    const bool hasMagic = dictSize >= 8 && rd32((const uint8_t*)hostDict) == ZF_DICT_MAGIC;
    if (dictType == ZHIP_DICT_FULLDICT && !hasMagic) { c->ddictKey = 0; return -ZE_DICT_CORRUPTED; }
    // A re-upload waits for everything in flight first (include/zstd_hip.h, "Setters"): the copies below are blocking ones and the digest kernels run on stream 0,
    // neither ordered against the non-blocking slot streams or a non-blocking caller stream on which an earlier call's kernels may still be reading these buffers.
    // Re-uploads are rare and the fingerprint hit above returns without it, so the wait is off the hot path.
    HIP_TRY(hipDeviceSynchronize());
    if (c->dictBlob.reserve(dictSize + 64)) { c->ddictKey = 0; return g_reserveRc; }       // (+ 64: K3 reads whole 32-byte windows)
    if (c->dictEntropy.reserve(sizeof(ZhipDictEntropy))) { c->ddictKey = 0; return g_reserveRc; }
    HIP_TRY(hipMemcpy(c->dictBlob.p, hostDict, dictSize, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(c->dictEntropy.p, 0, sizeof(ZhipDictEntropy)));
    ZhipDictEntropy de; memset(&de, 0, sizeof de);
    if (hasMagic && dictType != ZHIP_DICT_RAWCONTENT) {
        hipLaunchKernelGGL(zhip_parse_dict_kernel, dim3(1), dim3(64), 0, 0, (const uint8_t*)c->dictBlob.p, (uint32_t)dictSize,
                           (ZhipDictEntropy*)c->dictEntropy.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(&de, c->dictEntropy.p, sizeof de, hipMemcpyDeviceToHost));
        if (de.status) { c->ddictKey = 0; return -de.status; }            // negative zstd error code: dictionary corrupted
        if (de.hufCount) {                                                // the decode pipeline's ready-made tables
            if (c->dictTables.reserve(sizeof(ZhipDictTables))) { c->ddictKey = 0; return g_reserveRc; }
            hipLaunchKernelGGL(zhip_dict_tables_kernel, dim3(1), dim3(64), 0, 0, (const ZhipDictEntropy*)c->dictEntropy.p, (ZhipDictTables*)c->dictTables.p);
            HIP_TRY(hipGetLastError());
            int32_t tst = 0;
            HIP_TRY(hipMemcpy(&tst, (const uint8_t*)c->dictTables.p + offsetof(ZhipDictTables, status), 4, hipMemcpyDeviceToHost));
            if (tst) { c->ddictKey = 0; return -ZE_DICT_CORRUPTED; }
        }
    }
    c->dictSize = (uint32_t)dictSize; c->dictID = de.dictID; c->dictContentOffset = de.contentOffset;
    c->dictHasEntropy = de.hufCount != 0;
    return 0;
}
extern "C" int zhip_ctx_set_dformat(zhip_ctx* c, int format, uint64_t maxWindowSize)
{
    if (!c || (format != ZHIP_FORMAT_ZSTD1 && format != ZHIP_FORMAT_ZSTD1_MAGICLESS)) { g_lastError = "invalid frame format"; return ZHIP_ERR_UNSUPPORTED; }
    c->dformat = format;
    c->maxWindowSize = maxWindowSize ? maxWindowSize : ((1ull << 27) + 1);
    return 0;
}
// bring-up probe: launches a 64-lane kernel exercising every wave primitive the codec uses; returns 0 when correct
extern "C" int zhip_selftest(void)
{
    DevBuf buf; uint32_t h[64];
    if (buf.reserve(sizeof h)) return g_reserveRc;
    uint32_t* d = (uint32_t*)buf.p;
    hipLaunchKernelGGL(zhip_selftest_kernel, dim3(1), dim3(64), 0, 0, d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost));
    for (uint32_t l = 0; l < 64; l++) if (h[l] != l * (l + 1) / 2 + 32 + 63 + 7) { g_lastError = "selftest mismatch"; return 1; }
    return 0;
}
extern "C" int zhip_ctx_set_cparams(zhip_ctx* c, const zhip_cparams* p)
{
    if (!c || !p) return ZHIP_ERR_UNSUPPORTED;
    if (p->dictType != ZHIP_DICT_AUTO && p->dictType != ZHIP_DICT_RAWCONTENT && p->dictType != ZHIP_DICT_FULLDICT) { g_lastError = "invalid dictionary type"; return ZHIP_ERR_UNSUPPORTED; }
    if (p->format != ZHIP_FORMAT_ZSTD1 && p->format != ZHIP_FORMAT_ZSTD1_MAGICLESS) { g_lastError = "invalid frame format"; return ZHIP_ERR_UNSUPPORTED; }
    // level + explicit parameters -> one row per source-size class; the kernels implement the fast and double-fast strategies, and greedy where libzstd runs it with the
    // row match finder on 16-entry rows over one block: the row of 16 385 ... 131 072-byte sources, windowLog >= 15, searchLog <= 4 (ze_get_cparams decides per source: the window must cover it, hashLog <= 17)
    ZeRows rows;
    zh_resolve_rows(&rows, p->level, &p->cp);
    bool any = false;
    for (int t = 0; t < 4; t++) {
        if (!zh_check_cparams(rows.r[t])) return -ZE_PARAM_OUTOFBOUND;        // what ZSTD_CCtx_setParametersUsingCCtxParams reports
        any |= rows.r[t][6] == 1 || rows.r[t][6] == 2 || (t == 2 && rows.r[t][6] == 3 && rows.r[t][0] >= 15 && rows.r[t][3] <= 4);
    }
    if (!any) { g_lastError = "HIP backend compresses with the fast and double-fast strategies, and with greedy on inputs of 16 385 ... 131 072 bytes at search_log <= 4 (levels <= 3, negative levels; levels 4 and 5 for inputs above 16 KiB up to 128 KiB; or explicit strategy / parameters that select them)"; return ZHIP_ERR_UNSUPPORTED; }
    // nothing of a dictionary shorter than 8 bytes is loaded (ZSTD_compress_insertDictionary, zstd.c:28167) -- unless a full dictionary
    // was demanded, which is then "Dictionary mismatch"; so is a blob without the magic. The ZSTD_CDict still exists and its
    // parameter row (chosen for a 513-byte source) is what the frames are compressed with, so such a blob is digested like any other
    const bool hasDict = p->dict && p->dictSize;
    const bool hasMagic = hasDict && p->dictSize >= 8 && rd32((const uint8_t*)p->dict) == ZF_DICT_MAGIC;
    // What the caller sees when the dictionary cannot be digested is libzstd's, quirk included: the reference hands the blob to
    // ZSTD_CCtx_loadDictionary_advanced (c-ext/compressor.c:34-37), which only stores it; the ZSTD_CDict is made at the first compression
    // (ZSTD_initLocalDict, zstd.c:24206) and ANY failure there -- dictionary_wrong, dictionary_corrupted -- comes back as a NULL CDict,
    // reported as memory_allocation (zstd.c:24232): "cannot compress: Allocation error : not enough memory".
    if (hasDict && p->dictType == ZHIP_DICT_FULLDICT && !hasMagic) return -ZE_MEMORY;
    const bool useDict = hasDict;
    if (useDict) {
        uint64_t salt = 0x200u + (uint64_t)p->dictType;
        for (int t = 0; t < 4; t++) for (int k = 0; k < 7; k++) salt = salt * 1000003u + (uint64_t)(uint32_t)rows.r[t][k];
        const uint64_t key = dict_fingerprint(p->dict, p->dictSize, salt);
        if (c->hasCDict && c->cdictKey == key) { c->cparams = *p; c->cparams.dict = nullptr; c->cparams.dictSize = 0; c->rows = rows; return 0; }
        c->cdictKey = key;
    }
    c->hasCDict = false;
    if (useDict) {
        // digest the dictionary on the device: parse its entropy section, build the encoding tables, index its content
        // (what ZSTD_createCDict does on the host in the reference, zstd.c:28490-28614)
        if (p->dictSize > 0x7FFFFFFFu) { g_lastError = "dictionary too large"; return ZHIP_ERR_UNSUPPORTED; }
        const size_t cells = (size_t)1 << ZE_CDICT_MAX_HLOG;
        HIP_TRY(hipDeviceSynchronize());      // (as in zhip_ctx_set_ddict: an earlier call's kernels may still be reading the buffers written below)
        if (c->cdictBlob.reserve(p->dictSize + 16) || c->cdictEntropy.reserve(sizeof(ZhipDictEntropy)) ||
            c->cdictDigest.reserve(sizeof(ZeCDict)) || c->cdictTables.reserve(3 * cells * sizeof(uint32_t))) return g_reserveRc;
        HIP_TRY(hipMemcpy(c->cdictBlob.p, p->dict, p->dictSize, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset((uint8_t*)c->cdictBlob.p + p->dictSize, 0, 16));
        HIP_TRY(hipMemset(c->cdictEntropy.p, 0, sizeof(ZhipDictEntropy)));
        HIP_TRY(hipMemset(c->cdictDigest.p, 0, sizeof(ZeCDict)));
        ZhipDictEntropy de; memset(&de, 0, sizeof de);
        if (hasMagic && p->dictType != ZHIP_DICT_RAWCONTENT) {
            hipLaunchKernelGGL(zhip_parse_dict_kernel, dim3(1), dim3(64), 0, 0, (const uint8_t*)c->cdictBlob.p, (uint32_t)p->dictSize,
                               (ZhipDictEntropy*)c->cdictEntropy.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(&de, c->cdictEntropy.p, sizeof de, hipMemcpyDeviceToHost));
            if (de.status) return -ZE_MEMORY;                   // (dictionary_corrupted inside ZSTD_createCDict: see above)
        }
        uint32_t* t = (uint32_t*)c->cdictTables.p;
        hipLaunchKernelGGL(zhip_build_cdict_kernel, dim3(1), dim3(64), 0, 0, (const uint8_t*)c->cdictBlob.p, (uint32_t)p->dictSize,
                           (const ZhipDictEntropy*)c->cdictEntropy.p, rows, (ZeCDict*)c->cdictDigest.p, t, t + cells, t + 2 * cells);
        HIP_TRY(hipGetLastError());
        ZeCDict cd;
        HIP_TRY(hipMemcpy(&cd, c->cdictDigest.p, sizeof cd, hipMemcpyDeviceToHost));
        if (cd.status == ZE_PARAM_UNSUPPORTED) { g_lastError = "dictionary / level combination outside the fast / double-fast attached-dictionary paths of the HIP backend"; return ZHIP_ERR_UNSUPPORTED; }
        if (cd.status) return cd.status == ZE_DICT_CORRUPTED || cd.status == ZE_DICT_WRONG ? -ZE_MEMORY : -cd.status;
        c->hasCDict = true; c->cdictContentOffset = de.hufCount ? de.contentOffset : 0u;
        c->cdictAttachMax = cd.strat == 1 ? ZE_DICT_ATTACH_MAX_FAST : ZE_DICT_ATTACH_MAX;
        c->cdictHlog = cd.hlog; c->cdictClog = cd.clog; c->cdictStrat = cd.strat; c->cdictContentSize = cd.contentSize;
    }
    c->cparams = *p; c->cparams.dict = nullptr; c->cparams.dictSize = 0; c->rows = rows;
    return 0;
}

// ------------------------------------------------------------------------------------------ device-resident decode
// a chunk's timing events. Nothing is created while the context's timers are off, and every call is then a no-op; an event is destroyed with the owner unless a KTimer took it
// (a timer owns both events of its pairs; a pair that a second timer reads as well is LENT to that one, before the give that hands its events over) -- a HIP call that fails
// in the middle of a chunk leaks none
struct ChunkEvents {
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~ChunkEvents() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
    hipError_t create(int count) { for (int i = 0; i < count; i++) { const hipError_t e = hipEventCreate(&ev[i]); if (e != hipSuccess) return e; } return hipSuccess; }
    hipError_t record(int i, hipStream_t stream) { return ev[i] ? hipEventRecord(ev[i], stream) : hipSuccess; }
    void give(KTimer& t, int i, int j) { if (ev[i] && ev[j]) { t.pending.emplace_back(ev[i], ev[j]); ev[i] = ev[j] = nullptr; } }
    void lend(KTimer& t, int i, int j) { if (ev[i] && ev[j]) t.shared.emplace_back(ev[i], ev[j]); }      // (borrowed pairs are always drained before any destroy: drain_shared)
};
// ordering only: every stream of `to` waits for what `from` holds now. The event is made, recorded, waited for and destroyed here: none can outlive a failing call
static hipError_t streams_wait(hipStream_t from, const hipStream_t* to, int count)
{
    hipEvent_t e = nullptr;
    hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (r != hipSuccess) return r;
    r = hipEventRecord(e, from);
    for (int i = 0; i < count && r == hipSuccess; i++) r = hipStreamWaitEvent(to[i], e, 0);
    (void)hipEventDestroy(e);
    return r;
}
// a table of the kernels' phase timers (ZHIP_PROF): a line per phase with its share of `tot` and its wave-cycles per frame (`skipZero`: phases that counted nothing are left out)
static void print_prof_rows(const unsigned long long* h, const char* const* names, int count, unsigned long long tot, double frames, bool skipZero)
{
    for (int q = 0; q < count; q++) if (h[q] || !skipZero) fprintf(stderr, "[zhip-prof]    %-22s %6.2f%% %10.0f cyc/frame\n", names[q], 100.0 * h[q] / (tot ? tot : 1), (double)h[q] / frames);
}
// the dictionary fields that ZhipPipeArgs and ZhipDecodeArgs share
template <class Args> static void set_dict_args(const zhip_ctx* c, Args& a)
{
    if (!c->dictSize) return;
    a.dictID = c->dictID;
    a.dictContent = (const uint8_t*)c->dictBlob.p + c->dictContentOffset;
    a.dictContentSize = c->dictSize - c->dictContentOffset;
    a.dictEntropy = c->dictHasEntropy ? (const ZhipDictEntropy*)c->dictEntropy.p : nullptr;
}
// the launch plan's inputs (zhip_decode_plan.hpp) as this context has them
static ZdPlanIn decode_plan_inputs(const zhip_ctx* c, size_t n, const ZdHints& hint)
{
    ZdPlanIn in;
    in.n = n; in.hint = hint; in.dict = ZdPlanDict{c->dictSize != 0, c->dictHasEntropy}; in.prof = c->knob.prof; in.knob = c->knob;
    in.dev.numCU = c->numCU; in.dev.decBlocksPerCU = c->decBlocksPerCU; in.dev.k1PerCU = c->k1PerCU; in.dev.k3PerCU = c->k3PerCU;
    in.dev.k2LdsPerCU = ZHIP_LDS_BYTES / sizeof(ZpSeqQLDS); in.dev.k1bLdsPerCU = ZHIP_LDS_BYTES / sizeof(ZpHufKernelLDS); in.dev.k2Frames = ZQ_FRAMES;
    return in;
}
// the pipeline's buffers at the plan's sizes
static int reserve_decode(zhip_ctx* c, const ZdPlan& p)
{
    if (c->pipeBases.reserve(p.basesBytes)) return g_reserveRc;
    if (c->pipeMeta.reserve(p.metaBytes) || c->pipeLit.reserve(p.litBytes) || c->pipeCounters.reserve(p.countersBytes) || c->pipeFallback.reserve(p.fallbackBytes) ||
        c->pipeFse.reserve(p.fseBytes) || c->pipeOrder.reserve(p.orderBytes) || c->pipeHuf.reserve(p.hufBytes) || c->pipeOrderLit.reserve(p.orderLitBytes)) return g_reserveRc;
    if (p.pre && c->pipePre.reserve(p.preBytes)) return g_reserveRc;
    if (p.mb && (c->pipeItemFrame.reserve(p.itemFrameBytes) || c->pipeItemReps.reserve(p.itemRepsBytes) || c->pipeFrameRecs.reserve(p.frameRecsBytes))) return g_reserveRc;
    return 0;
}
// the pipeline's arguments that are the same for every chunk of the call
static int pipe_args_init(zhip_ctx* c, ZhipPipeArgs& pa, const ZdPlan& p, const void* d_src, const zhip_segment* d_srcSegs, void* d_dst, const zhip_segment* d_dstSegs,
                          uint64_t* d_outSizes, int32_t* d_status, hipStream_t stream)
{
    memset(&pa, 0, sizeof pa);
    pa.src = (const uint8_t*)d_src; pa.srcSegs = (const uint64_t*)d_srcSegs; pa.dst = (uint8_t*)d_dst; pa.dstSegs = (const uint64_t*)d_dstSegs;
    pa.outSizes = d_outSizes; pa.status = d_status; pa.fallbackList = (uint32_t*)c->pipeFallback.p;
    pa.maxWindowSize = c->maxWindowSize; pa.magicless = c->dformat == ZHIP_FORMAT_ZSTD1_MAGICLESS;
    set_dict_args(c, pa);                               // dictionary frames take the pipeline too (r02v; the generic kernel rebuilt the dictionary's tables per frame)
    pa.dictTables = pa.dictEntropy ? (const ZhipDictTables*)c->dictTables.p : nullptr;
    if (c->knob.prof) {
        if (!c->profPipe && (c->dictSize || p.mb))
            fprintf(stderr, "[zhip-prof] K3's phase timers exist in the dictionary-less single-block kernel only: with a dictionary or frames of several blocks they read zero\n");
        if (!c->profPipe) HIP_TRY(hipMalloc((void**)&c->profPipe, 32 * 8));
        HIP_TRY(hipMemsetAsync(c->profPipe, 0, 32 * 8, stream));
        pa.prof = c->profPipe;
    }
    pa.fallbackCount = (uint32_t*)c->pipeCounters.p;          // [0] = fallback length, then 8 words per slot
    pa.arenaBudget16 = (uint32_t)p.arenaBudget16;
    pa.k1Lanes = p.k1Lanes ? 1u : 0u;
    pa.ckLater = 1;
    return 0;
}
// ... and those of one chunk: frames [first, first + cnt) in the arenas of slot `sidx`
static void pipe_args_chunk(const zhip_ctx* c, ZhipPipeArgs& pa, const ZdPlan& p, const ZdChunkPlan& k, int sidx, size_t first, size_t cnt)
{
    const size_t slots = p.slots;
    pa.first = (uint32_t)first; pa.count = (uint32_t)cnt;
    pa.meta = (ZdMeta*)c->pipeMeta.p + (size_t)sidx * slots;
    pa.litArena = (uint8_t*)c->pipeLit.p + ZP_LIT_FRONT + (size_t)sidx * p.arenaBytes;     // (ZP_LIT_FRONT = 256 bytes in front: K2's parked / first stores of a room at 0 land there)
    pa.seqArena = (uint64_t*)pa.litArena;
    pa.bases = (uint32_t*)c->pipeBases.p + (size_t)sidx * slots * 2;
    pa.fseTables = (uint16_t*)c->pipeFse.p + (size_t)sidx * slots * ZP_FSE_CELLS;
    pa.order = (uint32_t*)c->pipeOrder.p + (size_t)sidx * slots;
    pa.hufTables = (uint16_t*)c->pipeHuf.p + (size_t)sidx * slots * ZP_HUF_CELLS;
    pa.orderLit = (uint32_t*)c->pipeOrderLit.p + (size_t)sidx * slots;
    if (p.mb) {
        pa.itemCap = k.itemCap;
        pa.itemFrame = (uint32_t*)c->pipeItemFrame.p + (size_t)sidx * slots;
        pa.itemReps = (uint32_t*)c->pipeItemReps.p + (size_t)sidx * slots * 4;
        pa.frameRecs = (ZpFrameRec*)c->pipeFrameRecs.p + (size_t)sidx * p.chunk;
    }
    pa.counters = (uint32_t*)c->pipeCounters.p + 8 + ZP_CNT_WORDS * sidx;
    pa.pre = p.pre ? (ZpPre*)c->pipePre.p + (size_t)sidx * slots : nullptr;
}
// K2 and K3 in the form the chunk's plan names (zd_decode_chunk_plan)
static void launch_k2(const ZdChunkPlan& k, hipStream_t ss, const ZhipPipeArgs& pa)
{
    if (k.k2 == ZD_K2_MB) hipLaunchKernelGGL(zhip_decode_seq_mb_kernel, dim3(k.g2), dim3(64), 0, ss, pa);
    else hipLaunchKernelGGL(zhip_decode_seq_kernel, dim3(k.g2), dim3(64), 0, ss, pa);
}
static void launch_k3(const ZdChunkPlan& k, hipStream_t ss, const ZhipPipeArgs& pa)
{
    const dim3 g(k.g3), b(64);
    if (k.k3 == ZD_K3_MB_DICT) hipLaunchKernelGGL(zhip_decode_exec_mb_dict_kernel, g, b, 0, ss, pa);
    else if (k.k3 == ZD_K3_MB) hipLaunchKernelGGL(zhip_decode_exec_mb_kernel, g, b, 0, ss, pa);
    else if (k.k3 == ZD_K3_DICT) hipLaunchKernelGGL(zhip_decode_exec_dict_kernel, g, b, 0, ss, pa);
    else if (k.k3 == ZD_K3_PROF) hipLaunchKernelGGL(zhip_decode_exec_prof_kernel, g, b, 0, ss, pa);
    else hipLaunchKernelGGL(zhip_decode_exec_kernel, g, b, 0, ss, pa);
}
// a chunk's kernels on its slot's stream (K0 / the lane pass, K1, the bins, K1b and K2, K3, KX), and its timers
static int launch_decode_chunk(zhip_ctx* c, const ZdPlan& p, const ZdChunkPlan& k, const ZhipPipeArgs& pa, int sidx)
{
    hipStream_t ss = c->slotStream[sidx];
    // the timing events, in the order they are recorded on the chunk's stream: 0 K1's start; 4 and 5 the bins' end; 1 K1b's end (with the side stream: K2's); 2 K3's start; 3 KX's end.
    // With the side stream two more: 6 at K2's end again, 7 K1b's end on the side stream
    ChunkEvents ev;
    if (c->timing) HIP_TRY(ev.create(p.side ? 8 : 6));
    HIP_TRY(ev.record(0, ss));
    if (k.k1 == ZD_K1_MB) hipLaunchKernelGGL(zhip_decode_lit_mb_kernel, dim3(k.g1), dim3(64), 0, ss, pa);
    else {
        if (k.gPre) hipLaunchKernelGGL(zhip_decode_pre_kernel, dim3(k.gPre), dim3(64), 0, ss, pa);
        if (k.k1 == ZD_K1_LANES) hipLaunchKernelGGL(zhip_decode_lit_lanes_kernel, dim3(k.gLanes), dim3(64), 0, ss, pa);
        hipLaunchKernelGGL(zhip_decode_lit_kernel, dim3(k.g1), dim3(64), 0, ss, pa);
    }
    hipLaunchKernelGGL(zhip_decode_bin_kernel, dim3(k.gBin), dim3(64), 0, ss, pa);      // tiny; timed with K1
    HIP_TRY(ev.record(4, ss)); HIP_TRY(ev.record(5, ss));
    if (p.side) {
        // K1b and K2 need nothing of each other: both follow K1 and the bins, K3 follows both. K2's 15-frame groups are long (~1.9 ms at 128 KiB) and a wave gets 4.27 of
        // them at 65 536 frames, so K2 ends with three quarters of its waves gone for a group's time, and K1b then starts on an empty chip. K1b goes to a side stream BEHIND
        // K2's launch instead: K2's one-wave workgroups are all resident at once, K1b's land where K2's have drained (two K2 waves' LDS make room for one of K1b's).
        // 65 536 x 128 KiB: 24.35 -> 23.3 ms (K1b's 3.35 ms cost 2.4 beyond K2's end), frames of several blocks 150 -> 158 GB/s (r06p). The other order (K1b first)
        // LOSES, 26.2 ms: K1b's short groups keep handing LDS to K2 piecemeal and the mix holds three waves per CU where K2 alone holds four.
        if (!c->sideStream[sidx]) HIP_TRY(hipStreamCreateWithFlags(&c->sideStream[sidx], hipStreamNonBlocking));
        hipStream_t sd = c->sideStream[sidx];
        HIP_TRY(streams_wait(ss, &sd, 1));                      // the bins -> the side stream
        launch_k2(k, ss, pa);
        HIP_TRY(ev.record(1, ss)); HIP_TRY(ev.record(6, ss));       // (two events at K2's end: one closes K2's pair, one opens K1b's)
        hipLaunchKernelGGL(zhip_decode_huf_kernel, dim3(k.gHuf), dim3(64), 0, sd, pa);
        HIP_TRY(ev.record(7, sd));
        HIP_TRY(streams_wait(sd, &ss, 1));                      // the side stream -> the chunk's
    } else {
        hipLaunchKernelGGL(zhip_decode_huf_kernel, dim3(k.gHuf), dim3(64), 0, ss, pa);
        HIP_TRY(ev.record(1, ss));
        launch_k2(k, ss, pa);
    }
    HIP_TRY(ev.record(2, ss));
    launch_k3(k, ss, pa);
    hipLaunchKernelGGL(zhip_decode_check_kernel, dim3(k.gCheck), dim3(64), 0, ss, pa);      // KX (returns at once when no frame carries a checksum; timed with K3)
    HIP_TRY(ev.record(3, ss));
    HIP_TRY(hipGetLastError());
    // consecutive events bracket one kernel each (same stream, nothing in between). Ownership: K1's timer owns
    // (ev[0], ev[4]), K1b's (ev[5], ev[1]), K3's (ev[2], ev[3]); K2's pair (ev[1], ev[2]) is borrowed and always drained
    // before any destroy.
    ev.lend(c->timer[9], 0, 3);                // the chunk's pipeline, K1's start to K3's end: what the step costs now that two of its kernels overlap
    if (!p.side) ev.lend(c->timer[3], 1, 2);
    ev.give(c->timer[2], 0, 4);                // K1 (+ the two bin waves)
    if (p.side) {
        // K2's pair is its own now; K1b's is what it costs the step: from K2's END (on the main stream) to its own end on the side stream -- its first part
        // runs inside K2's tail --, so that the kernels' times still add up to the step (a K1b that ends before K2 counts zero)
        ev.give(c->timer[3], 5, 1);
        ev.give(c->timer[7], 6, 7);
    } else ev.give(c->timer[7], 5, 1);         // K1b
    ev.give(c->timer[4], 2, 3);
    return 0;
}
// the pipeline kernels' phase timers of a call over n frames (ZHIP_PROF)
static int print_pipe_prof(const unsigned long long* d_prof, size_t n)
{
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long h[32];
    HIP_TRY(hipMemcpy(h, d_prof, sizeof h, hipMemcpyDeviceToHost));
    static const char* nm[10] = {"header", "huf-table", "huf-decode", "seq-header+fse", "K3 load+scan", "-", "K3 literal/far fetch", "K3 near rounds", "K3 flush", "tail"};
    for (int k = 0; k < 2; k++) {
        unsigned long long tot = 0; for (int q = 0; q < 10; q++) tot += h[16 * k + q];
        fprintf(stderr, "[zhip-prof] %s: %.0f wave-cycles per frame\n", k ? "K3" : "K1", (double)tot / (double)n);
        print_prof_rows(h + 16 * k, nm, 10, tot, (double)n, true);
    }
    return 0;
}
// the generic kernel over the pipeline's fallback list, on the caller's stream
static int launch_decode_generic(zhip_ctx* c, uint32_t grid, const void* d_src, const zhip_segment* d_srcSegs, size_t n, void* d_dst, const zhip_segment* d_dstSegs,
                                 uint64_t* d_outSizes, int32_t* d_status, hipStream_t stream)
{
    ZhipDecodeArgs a; memset(&a, 0, sizeof a);
    a.src = (const uint8_t*)d_src; a.srcSegs = (const uint64_t*)d_srcSegs; a.dst = (uint8_t*)d_dst;
    a.dstSegs = (const uint64_t*)d_dstSegs; a.outSizes = d_outSizes; a.status = d_status;
    a.scratch = (uint8_t*)c->scratch.p; a.counter = (uint32_t*)c->counter.p; a.n = (uint32_t)n;
    a.maxWindowSize = c->maxWindowSize; a.magicless = c->dformat == ZHIP_FORMAT_ZSTD1_MAGICLESS;
    a.frameList = (const uint32_t*)c->pipeFallback.p; a.listCount = (const uint32_t*)c->pipeCounters.p;
    set_dict_args(c, a);
    const bool prof = c->knob.prof;
    if (prof) {
        if (!c->profDecode) HIP_TRY(hipMalloc((void**)&c->profDecode, ZP_N * 8));
        HIP_TRY(hipMemsetAsync(c->profDecode, 0, ZP_N * 8, stream));
        a.prof = c->profDecode;
    }
    ChunkEvents ev;
    if (c->timing) HIP_TRY(ev.create(2));
    HIP_TRY(ev.record(0, stream));
    hipLaunchKernelGGL(zhip_decode_frames_kernel, dim3(grid), dim3(64), 0, stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(ev.record(1, stream));
    ev.give(c->timer[0], 0, 1);
    if (prof) {
        unsigned long long h[ZP_N];
        HIP_TRY(hipMemcpy(h, c->profDecode, sizeof h, hipMemcpyDeviceToHost));
        static const char* names[ZP_N] = {"header/misc", "huf-table", "huf-decode", "seq-tables", "stage", "seq-decode(lane0)", "exec1(global->lds)", "exec2(lds rounds)", "flush", "raw/lastlit"};
        unsigned long long tot = 0; for (int i = 0; i < ZP_N; i++) tot += h[i];
        fprintf(stderr, "[zhip-prof] grid=%u (CUs %d x %d blocks) frames=%u wave-cycles total=%.3e (%.0f per frame)\n", grid, c->numCU, c->decBlocksPerCU, a.n, (double)tot, (double)tot / a.n);
        print_prof_rows(h, names, ZP_N, tot, (double)a.n, false);
    }
    if (c->timer[0].pending.size() > 1024) { HIP_TRY(hipStreamSynchronize(stream)); for (int i = 0; i < ZHIP_NTIMER; i++) drain_shared(c->timer[i]); for (int i = 0; i < ZHIP_NTIMER; i++) drain_timer(c->timer[i]); }
    return 0;
}
// zhip_decompress_batch_device under what the caller knows about the batch's frames (ZdHints): validate, plan, reserve, fork the slot streams off the caller's, the chunks,
// join, the generic kernel. The phase-split fast path (zhip_decode_pipeline.hpp) takes single-block frames and, under a size hint, frames of several blocks; everything it
// declines lands in the fallback list consumed by the generic kernel behind it. Every decision is the launch plan's (zhip_decode_plan.hpp).
static int decompress_batch(zhip_ctx* c, const ZdHints& hint, const void* d_src, const zhip_segment* d_srcSegs, size_t n, void* d_dst, const zhip_segment* d_dstSegs,
                            uint64_t* d_outSizes, int32_t* d_status, void* streamv)
{
    if (n == 0) return 0;
    if (n > 0x7FFFFFFFu) { g_lastError = "too many frames in one launch"; return ZHIP_ERR_UNSUPPORTED; }
    hipStream_t stream = (hipStream_t)streamv;
    const ZdPlanIn in = decode_plan_inputs(c, n, hint);
    const ZdPlan p = zd_decode_plan(in);
    if (c->scratch.reserve(p.scratchBytes)) return g_reserveRc;
    if (c->counter.reserve(p.counterBytes)) return g_reserveRc;
    HIP_TRY(hipMemsetAsync(c->counter.p, 0, 4, stream));
    if (p.tooLarge) { g_lastError = "frame too large for the block arenas"; return ZHIP_ERR_UNSUPPORTED; }
    if (int rc = reserve_decode(c, p)) return rc;
    for (int sidx = 0; sidx < p.nslot; sidx++) if (!c->slotStream[sidx]) HIP_TRY(hipStreamCreateWithFlags(&c->slotStream[sidx], hipStreamNonBlocking));
    HIP_TRY(hipMemsetAsync(c->pipeCounters.p, 0, p.countersBytes, stream));
    HIP_TRY(streams_wait(stream, c->slotStream, p.nslot));                 // the slots start after everything queued on the caller's stream
    ZhipPipeArgs pa;
    if (int rc = pipe_args_init(c, pa, p, d_src, d_srcSegs, d_dst, d_dstSegs, d_outSizes, d_status, stream)) return rc;
    size_t ci = 0;
    for (size_t first = 0; first < n; first += p.chunk, ci++) {
        const int sidx = (int)(ci % p.nslot);
        const size_t cnt = n - first < p.chunk ? n - first : p.chunk;
        const ZdChunkPlan k = zd_decode_chunk_plan(in, p, cnt);
        pipe_args_chunk(c, pa, p, k, sidx, first, cnt);
        if (ci >= (size_t)p.nslot) HIP_TRY(hipMemsetAsync(pa.counters, 0, ZP_CNT_WORDS * 4, c->slotStream[sidx]));
        if (int rc = launch_decode_chunk(c, p, k, pa, sidx)) return rc;
    }
    if (pa.prof) if (int rc = print_pipe_prof(pa.prof, n)) return rc;
    for (int sidx = 0; sidx < p.nslot; sidx++) HIP_TRY(streams_wait(c->slotStream[sidx], &stream, 1));      // the caller's stream continues after every slot has drained
    return launch_decode_generic(c, p.genericGrid, d_src, d_srcSegs, n, d_dst, d_dstSegs, d_outSizes, d_status, stream);
}
extern "C" int zhip_decompress_batch_device(zhip_ctx* c, const void* d_src, const zhip_segment* d_srcSegs, size_t n,
                                            void* d_dst, const zhip_segment* d_dstSegs, uint64_t* d_outSizes,
                                            int32_t* d_status, void* streamv)
{
    if (!c) return ZHIP_ERR_UNSUPPORTED;
    ZdHints hint; hint.size = c->itemHint;
    return decompress_batch(c, hint, d_src, d_srcSegs, n, d_dst, d_dstSegs, d_outSizes, d_status, streamv);
}
// the LDS-source match kernel at one source size per CU slot -- the fast strategy's (FAST) or the double-fast one's -- of the four sizes the one the plan's shape names
template <uint32_t BYTES, bool FAST> static void launch_lds_at(dim3 g, hipStream_t stream, const ZhipEncodeArgs& a)
{
    if constexpr (FAST) hipLaunchKernelGGL((zhip_encode_match_lds_fast_kernel<BYTES, ZHIP_E1LDS_FAST_PAIRS>), g, dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((zhip_encode_match_lds_kernel<BYTES, ZHIP_E1LDS_PROBES>), g, dim3(64), 0, stream, a);
}
template <bool FAST> static void launch_lds(int shape, dim3 g, hipStream_t stream, const ZhipEncodeArgs& a)
{
    if (shape == 0) launch_lds_at<4096, FAST>(g, stream, a);
    else if (shape == 1) launch_lds_at<16384, FAST>(g, stream, a);
    else if (shape == 2) launch_lds_at<65536, FAST>(g, stream, a);
    else launch_lds_at<ZF_BLOCK_MAX, FAST>(g, stream, a);
}
// the match kernel a chunk's plan names (ze_encode_chunk_plan), on its grid
static void launch_match(const ZeChunkPlan& k, hipStream_t stream, const ZhipEncodeArgs& a)
{
    const dim3 g(k.grid), b(64);
    if (k.kernel == ZE_MATCH_LDS_FAST) launch_lds<true>(k.shape, g, stream, a);
    else if (k.kernel == ZE_MATCH_LDS) launch_lds<false>(k.shape, g, stream, a);
    else if (k.fastPairs == 2) hipLaunchKernelGGL(zhip_encode_match_flat_fast2_kernel, g, b, 0, stream, a);
    else if (k.fastPairs) hipLaunchKernelGGL(zhip_encode_match_flat_fast_kernel, g, b, 0, stream, a);
    else if (k.probes == 4) hipLaunchKernelGGL(zhip_encode_match_flat4_kernel, g, b, 0, stream, a);
    else if (k.probes == 3) hipLaunchKernelGGL(zhip_encode_match_flat3_kernel, g, b, 0, stream, a);
    else hipLaunchKernelGGL(zhip_encode_match_flat_kernel, g, b, 0, stream, a);
}
// ---- what the compress calls share: the counter block's cells, the launch arguments every encode kernel reads from the context's zhip_ctx_set_cparams
// state, the launch plan's inputs, a chunk's timing events, and the entropy + trailer launches behind whatever left the sequences
// the cells of the context's counter block (zhip_ctx::counter) the encode paths use, as byte offsets
enum : size_t {
    ZC_E1_WORK = 8,        // the E1 work counter: the match kernels' sources taken so far (ZhipEncodeArgs.counter)
    ZC_E2_WORK = 12,       // the E2 work counter: the entropy kernel's, which it finds at ZhipEncodeArgs.counter + 1
    ZC_BIG_COUNT = 24,     // bigCount: length of the list of sources left to the generic kernel
    ZC_BIG_WORK = 28,      // the generic kernel's work counter over that list
    ZC_E1_COUNT = 32,      // e1Count: length of the list the flat match kernel leaves to the lane-serial one
    ZC_IDLE = 256,         // the idle pad: 16 readable bytes for the flat searches' lanes without a candidate (ZhipEncodeArgs.idle)
};
static_assert(ZC_E2_WORK == ZC_E1_WORK + 4 && ZC_BIG_WORK == ZC_BIG_COUNT + 4 && ZC_E1_COUNT == ZC_BIG_WORK + 4, "one memset clears neighbouring cells: E1 + E2, bigCount + the generic kernel's (+ e1Count)");
static void enc_args_init(zhip_ctx* c, ZhipEncodeArgs& a, const void* d_src, const zhip_segment* d_srcSegs, size_t n, void* d_dst, const zhip_segment* d_dstSegs,
                          uint64_t* d_outSizes, int32_t* d_status, uint8_t* cbase)
{
    memset(&a, 0, sizeof a);
    a.src = (const uint8_t*)d_src; a.srcSegs = (const uint64_t*)d_srcSegs; a.dst = (uint8_t*)d_dst;
    a.dstSegs = (const uint64_t*)d_dstSegs; a.outSizes = d_outSizes; a.status = d_status;
    a.workspace = (uint8_t*)c->encWorkspace.p; a.counter = (uint32_t*)(cbase + ZC_E1_WORK); a.n = (uint32_t)n;
    a.idle = cbase + ZC_IDLE;                                                   // (the context's own counter block: ADVICE r04 -- the caller's arena base need not be readable)
    a.level = c->cparams.level == 0 ? 3 : c->cparams.level;
    a.rows = c->rows; a.magicless = c->cparams.format == ZHIP_FORMAT_ZSTD1_MAGICLESS;
    a.contentSizeFlag = c->cparams.contentSizeFlag != 0; a.checksumFlag = c->cparams.checksumFlag != 0; a.dictIDFlag = c->cparams.dictIDFlag != 0;
    if (c->hasCDict) {
        const size_t cells = (size_t)1 << ZE_CDICT_MAX_HLOG;
        a.cdict = (const ZeCDict*)c->cdictDigest.p;
        a.cdictContent = (const uint8_t*)c->cdictBlob.p + c->cdictContentOffset;
        a.cdictHashLong = (const uint32_t*)c->cdictTables.p;
        a.cdictHashSmall = (const uint32_t*)c->cdictTables.p + cells;
    }
}
// the launch plan's inputs (zhip_encode_plan.hpp) as this context has them
static ZePlanIn plan_inputs(const zhip_ctx* c, size_t n)
{
    ZePlanIn in;
    in.rows = c->rows; in.n = n; in.sizeHint = c->srcMaxHint ? c->srcMaxHint : c->itemHint; in.srcMaxHint = c->srcMaxHint;
    in.dict = ZePlanDict{c->hasCDict, c->cdictHlog, c->cdictClog, c->cdictStrat, c->cdictAttachMax, c->cdictContentSize};
    in.dev = ZePlanDevice{c->numCU, c->encBlocksPerCU, c->e1PerCU, c->e2PerCU};
    in.knob = c->knob;
    return in;
}
// EX over the chunk where the frame kernel in front of it left the checksum trailers to it (ZhipEncodeArgs.xxLater): a lane per frame
static void launch_trailer(const zhip_ctx* c, const ZhipEncodeArgs& a, size_t cnt, hipStream_t stream)
{
    if (!a.xxLater) return;
    const size_t w = (cnt + 63) / 64, gm = (size_t)c->numCU * 8;
    hipLaunchKernelGGL(zhip_encode_trailer_kernel, dim3((uint32_t)(w < gm ? w : gm)), dim3(64), 0, stream, a);
}
// E2 over the chunk, g2 waves, and EX behind it for checksummed frames (timed with E2)
static void launch_entropy(const zhip_ctx* c, ZhipEncodeArgs& a, uint32_t g2, size_t cnt, hipStream_t stream)
{
    a.xxLater = ZHIP_TRAILER_LATER && a.checksumFlag ? 1u : 0u;
    hipLaunchKernelGGL(zhip_encode_entropy_kernel, dim3(g2), dim3(64), 0, stream, a);
    launch_trailer(c, a, cnt, stream);
    a.xxLater = 0;
}
// the arena of the calls that run no match search of the library's (ZeSlotPlan): no room for a whole chunk's slots: half as many sources per launch, down to 64, before the call fails
static int reserve_slots(zhip_ctx* c, const ZePlanDevice& dev, ZeSlotPlan& s, ZhipEncodeArgs& a, uint32_t* g2)
{
    a.arenaStride = s.arenaStride; a.arenaLit = s.arenaLit; a.slotSrcMax = s.slotSrcMax;
    while (c->encArena.reserve(s.chunk * (size_t)s.arenaStride)) {
        if (g_reserveRc != ZHIP_ERR_NO_MEMORY || s.chunk <= 64) return g_reserveRc;
        s.chunk = (s.chunk + 1) / 2;
    }
    *g2 = ze_entropy_grid(dev, s.chunk);
    if (c->encMeta.reserve(s.chunk * sizeof(ZeMeta)) || c->encWorkspace.reserve((size_t)*g2 * ZE_E2_STRIDE + ZHIP_ENC_STRIDE)) return g_reserveRc;
    a.workspace = (uint8_t*)c->encWorkspace.p; a.meta = (ZeMeta*)c->encMeta.p; a.arena = (uint8_t*)c->encArena.p;
    return 0;
}
extern "C" int zhip_ctx_set_match_finder(zhip_ctx* c, int finder)
{
    if (!c || (finder != ZHIP_FINDER_LIBZSTD && finder != ZHIP_FINDER_WAVE && finder != ZHIP_FINDER_NONE && finder != ZHIP_FINDER_AUTO)) { g_lastError = "zhip_ctx_set_match_finder: unknown match finder"; return ZHIP_ERR_UNSUPPORTED; }
    c->matchFinder = finder;
    return 0;
}
// zhip_compress_batch_device under ZHIP_FINDER_WAVE: per chunk the wave match kernel in place of every other match kernel, then the entropy and trailer kernels as ever.
// No flat tables, no table-placement pick, no generic kernel: a source of several blocks is refused at its own index (status 40, by the entropy kernel's ze_frame).
static int compress_batch_wave(zhip_ctx* c, ZhipEncodeArgs& a, uint8_t* cbase, size_t n, hipStream_t stream)
{
    // the one-block row (sources of 16 385 ... 131 072 bytes) must be fast or double-fast -- the entropy side codes those; where only the row of smaller sources is
    // something else (level 4), those sources are refused one by one
    if (c->hasCDict) { g_lastError = "the wave match finder (ZHIP_FINDER_WAVE) does not take a dictionary"; return ZHIP_ERR_UNSUPPORTED; }
    if (a.rows.r[2][6] != 1 && a.rows.r[2][6] != 2) { g_lastError = "the wave match finder (ZHIP_FINDER_WAVE) serves the levels whose one-block row is fast or double-fast (levels <= 4, negative levels, explicit strategy 1 / 2)"; return ZHIP_ERR_UNSUPPORTED; }
    const ZePlanIn in = plan_inputs(c, n);
    ZeSlotPlan s = ze_wave_plan(in);
    uint32_t g2 = 0;
    if (int rc = reserve_slots(c, in.dev, s, a, &g2)) return rc;
    const size_t chunk = s.chunk, gwmax = (size_t)c->numCU * (size_t)c->wavePerCU[c->knob.waveH - 12];
    for (size_t first = 0; first < n; first += chunk) {
        const size_t cnt = n - first < chunk ? n - first : chunk;
        a.first = (uint32_t)first; a.count = (uint32_t)cnt;
        HIP_TRY(hipMemsetAsync(cbase + ZC_E1_WORK, 0, 8, stream));
        ChunkEvents ev;      // wave kernel: 0 .. 1, entropy + trailer: 2 .. 3
        if (c->timing) HIP_TRY(ev.create(4));
        HIP_TRY(ev.record(0, stream));
        const dim3 g((uint32_t)(cnt < gwmax ? cnt : gwmax)), b(64);
        if (c->knob.waveH == 12) hipLaunchKernelGGL(zhip_encode_match_wave_kernel<12>, g, b, 0, stream, a);
        else if (c->knob.waveH == 14) hipLaunchKernelGGL(zhip_encode_match_wave_kernel<14>, g, b, 0, stream, a);
        else hipLaunchKernelGGL(zhip_encode_match_wave_kernel<13>, g, b, 0, stream, a);
        HIP_TRY(ev.record(1, stream)); HIP_TRY(ev.record(2, stream));
        launch_entropy(c, a, g2, cnt, stream);
        HIP_TRY(ev.record(3, stream));
        ev.give(c->timer[10], 0, 1); ev.give(c->timer[6], 2, 3);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
// zhip_compress_batch_device under ZHIP_FINDER_NONE: per chunk the literals-only kernel in place of the match kernels AND the entropy kernel, then the trailer kernel where
// checksums are on. It reserves the chunk's ZeMeta records and nothing else -- no arena, no tables, no entropy workspace -- and touches none of the default finder's state
// (flat tables and their launch numbers, the placement pick, the arenas), so a context may alternate finders between calls.
static int compress_batch_none(zhip_ctx* c, ZhipEncodeArgs& a, uint8_t* cbase, size_t n, hipStream_t stream)
{
    if (const char* why = ze_none_refusal(a.rows, c->hasCDict)) { g_lastError = why; return ZHIP_ERR_UNSUPPORTED; }
    const ZeNonePlan s = ze_none_plan(plan_inputs(c, n));
    if (c->encMeta.reserve(s.metaBytes)) return g_reserveRc;
    a.meta = (ZeMeta*)c->encMeta.p; a.workspace = nullptr;
    for (size_t first = 0; first < n; first += s.chunk) {
        const size_t cnt = n - first < s.chunk ? n - first : s.chunk;
        a.first = (uint32_t)first; a.count = (uint32_t)cnt;
        HIP_TRY(hipMemsetAsync(cbase + ZC_E1_WORK, 0, 8, stream));
        ChunkEvents ev;      // the literals-only kernel + trailer: 0 .. 1
        if (c->timing) HIP_TRY(ev.create(2));
        HIP_TRY(ev.record(0, stream));
        a.xxLater = ZHIP_TRAILER_LATER && a.checksumFlag ? 1u : 0u;
        hipLaunchKernelGGL(zhip_encode_none_kernel, dim3(s.grid), dim3(64), 0, stream, a);
        launch_trailer(c, a, cnt, stream);
        a.xxLater = 0;
        HIP_TRY(ev.record(1, stream));
        ev.give(c->timer[11], 0, 1);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
// frames per launch of the flat match kernel for a batch above 65 536 (ZePlan::flatMaxOpen): 131 072 where the device has `need` bytes free, asked once per context
// (hipMemGetInfo is not a launch-path call)
static size_t flat_max_decided(zhip_ctx* c, size_t need)
{
    if (!c->flatMaxCached) {
        size_t freeB = 0, totalB = 0;
        c->flatMaxCached = 65536;
        if (hipMemGetInfo(&freeB, &totalB) == hipSuccess && freeB + c->encFlatTables.cap + c->encArena.cap >= need) c->flatMaxCached = 131072;
    }
    return c->flatMaxCached;
}
// A launch of a flat search on `tables`: the next launch number for its cells (ZhipEncodeArgs.tabEpoch), the tables zeroed where the numbers start again. `zeroed` comes
// back false when the plan's tables carry no launch numbers (ZePlan::epochShift) and the caller zeroes them as before. Changes the context's encEpoch* fields and `args` only.
static int next_epoch(zhip_ctx* c, const ZePlan& p, ZhipEncodeArgs& args, uint8_t* tables, uint64_t gen, size_t bytes, hipStream_t stream, bool* zeroed)
{
    args.tabEpoch = 0; args.tabEpochShift = 31; *zeroed = false;
    if (!p.epochShift) return 0;
    *zeroed = true;
    const uint32_t es = p.epochShift, maxE = (1u << (32 - es)) - 1;
    const uint64_t key = (p.flatDict ? c->cdictKey : 0x9E3779B97F4A7C15ull) ^ p.epochKeyLayout;
    if (tables != c->encEpochPtr || gen != c->encEpochGen || es != c->encEpochShift || key != c->encEpochKey || c->encEpoch >= maxE || bytes > c->encEpochBytes) {
        HIP_TRY(hipMemsetAsync(tables, 0, bytes, stream));
        c->encEpoch = 0; c->encEpochPtr = tables; c->encEpochGen = gen; c->encEpochShift = es; c->encEpochKey = key; c->encEpochBytes = bytes;
    }
    args.tabEpoch = ++c->encEpoch; args.tabEpochShift = es;
    return 0;
}
// Picking the tables' placement (round 5). The flat match kernel's time for one and the same launch differs by ~14 % with WHERE the driver put
// this 25 GiB allocation (397-415 ms or 455-488 per 65 536 frames; sticky for the life of the allocation, not controllable
// through the allocator) -- and two allocations held at the same time are different memory. So the first large launch of a context times the
// real kernel on its tables, reserves a second set beside them, times that, and keeps the faster (tests/tools/e1f_pick_best.py, r05g: in every
// trial at least one of three candidates was the fast kind, and the best stayed the best). Costs two extra launches of the kernel and a transient
// second table allocation, once per context; skipped where the second set does not fit. ZHIP_E1F_PICK=0 turns it off.
// Leaves the kept tables in c->encFlatTables and a.flatTables.
static int pick_table_placement(zhip_ctx* c, const ZePlan& p, ZhipEncodeArgs& a, hipStream_t stream)
{
    if (!p.flat || p.mbc || !c->knob.e1fPick || p.chunk < ZHIP_PICK_MIN || (c->e1fPicked && c->e1fPickedPtr == c->encFlatTables.p)) return 0;      // (again when a larger batch made the context reallocate its tables)
    c->e1fPicked = true; c->e1fPickKept = 0; c->e1fPickMs[1] = c->e1fPickMs[2] = 0;
    uint8_t* const cbase = (uint8_t*)c->counter.p;
    uint8_t* const flatTables = a.flatTables;
    const size_t cnt0 = p.chunk, bytes = p.flatTablesBytes;
    DevBuf cand;      // (releases itself however the pick ends)
    ChunkEvents ev;
    if (ev.create(2) == hipSuccess) {
        const hipEvent_t e0 = ev.ev[0], e1 = ev.ev[1];
        ZhipEncodeArgs pa = a; pa.first = 0; pa.count = (uint32_t)cnt0;
        // (round 6, last session: a probe searches the first 8 KiB of every source only. What makes an allocation the slow kind shows in any stretch of the launch -- eight
        // candidates in each of six processes, whole launch / first 8 KiB: 405-412 ms / 30.1-30.5 or 468-485 / 35.7-36.4, never out of order (profiles/r06zzr_pick_study.txt) --
        // so a candidate costs ~35 ms instead of ~450, the first large launch of a context 0.1-0.2 s instead of 1.3, and three slow candidates in a row (one time in eleven
        // at this box's 4 in 9) get three more tries by the rule below instead of a slow context)
        pa.probeCap = p.flatDict ? 0u : 8192u;
        auto timeOn = [&](uint8_t* t, float* ms) -> int {
            pa.flatTables = t;
            HIP_TRY(hipMemsetAsync(cbase + ZC_E1_WORK, 0, 8, stream)); HIP_TRY(hipMemsetAsync(cbase + ZC_BIG_COUNT, 0, 12, stream));
            {   bool z = false;                                                    // (launch numbers in the cells: a candidate allocation is zeroed once, by next_epoch)
                if (int rc = next_epoch(c, p, pa, t, t == (uint8_t*)cand.p ? cand.gen : c->encFlatTables.gen, bytes, stream, &z)) return rc;
                if (!z && !p.flatDict) { HIP_TRY(hipMemsetAsync(t, 0, bytes, stream)); c->encEpochPtr = nullptr; } }
            HIP_TRY(hipEventRecord(e0, stream));
            launch_match(p.pick, stream, pa);
            HIP_TRY(hipEventRecord(e1, stream));
            HIP_TRY(hipEventSynchronize(e1));
            HIP_TRY(hipEventElapsedTime(ms, e0, e1));
            return 0;
        };
        // three candidates: the context's own tables, then two further sets, each reserved beside the best so far (r05g / r05h: 397-415 or 455-488 ms per
        // 65 536 frames; 746-764, 805, 855, 928 per 131 072); the fastest is kept
#if ZHIP_PICK_STUDY
        // DIAGNOSTIC build: eight candidate allocations, each timed whole and over the sources' first 8 KiB; the probe's waves leave their durations (wall clock, 10 ns units), printed
        // as the mean of each sixteenth of the allocation -- is a slow allocation slow everywhere?
        {   const uint32_t cap0 = pa.probeCap;
            const size_t nw = (cnt0 + 63) / 64;
            DevBuf clockBuf; if (clockBuf.reserve(nw * 8)) return g_reserveRc;
            unsigned long long* dClock = (unsigned long long*)clockBuf.p;
            std::vector<unsigned long long> hClock(nw);
            for (int k = 0; k < (ZHIP_PICK_STUDY > 1 ? ZHIP_PICK_STUDY : 8); k++) {            // (-DZHIP_PICK_STUDY=n, n > 1: n candidates, whole launches for the first eight only)
                uint8_t* t = flatTables;
                if (k) { if (cand.reserve(bytes)) { (void)hipGetLastError(); break; } t = (uint8_t*)cand.p; }
                float whole = 0, probe = 0;
                pa.probeCap = 0; if (k < 8) if (int rc = timeOn(t, &whole)) return rc;
                HIP_TRY(hipMemsetAsync(dClock, 0, nw * 8, stream));
                pa.probeCap = 8192; pa.waveClock = dClock; if (int rc = timeOn(t, &probe)) return rc;
                pa.waveClock = nullptr; pa.probeCap = cap0;
                HIP_TRY(hipMemcpy(hClock.data(), dClock, nw * 8, hipMemcpyDeviceToHost));
                char line[512]; int o = 0; unsigned long long mn = ~0ull, mx = 0;
                for (int q = 0; q < 16; q++) { double sum = 0; size_t lo = nw * q / 16, hi = nw * (q + 1) / 16; for (size_t w = lo; w < hi; w++) { sum += (double)hClock[w]; if (hClock[w] < mn) mn = hClock[w]; if (hClock[w] > mx) mx = hClock[w]; }
                                               o += snprintf(line + o, sizeof line - o, " %.2f", sum / (double)(hi - lo ? hi - lo : 1) / 1e5); }
                fprintf(stderr, "[zhip-pick-study] candidate %d %p whole %.1f ms, first 8 KiB %.1f; waves' ms by sixteenth of the allocation:%s (min %.2f max %.2f)\n", k, (void*)t, whole, probe, line, mn / 1e5, mx / 1e5);
                if (k) cand.release();
            }
        }
#endif
        float best = 0;
        if (int rc = timeOn(flatTables, &best)) return rc;
        c->e1fPickMs[0] = best;
        // (round 6: where a probe is cheap -- dictionary batches: ~40 ms and 12 GiB a candidate -- and the first three came out ALIKE, which says they are one kind but not
        // which, up to three more are tried until one is clearly faster: a dictionary batch's candidates are the fast kind one time in three, 35.4 ms against 41-42
        // (r06u: [35.6, 42.1, 42.1], [42.3, 35.3, 42.1]; r06z: [41.1, 40.9, 41.2] -- all slow, 23.2 GB/s instead of 26.5), so three of them are all slow three runs in ten)
        // (round 6, last session: EIGHT candidates, always. With probes at ~35 ms there is no reason to stop at the first fast one, and there is a third kind: the wave-clock study
        // (profiles/r06zzv_wave_clocks.txt) found allocations at 388-392 ms per 65 536 sources beside the 406-417 and 467-473 ones -- one candidate in eight, the eighth in each of
        // three processes; an allocation's kind is the same over all of its sixteenths, so there is nothing to pick INSIDE one)
        // (a released candidate's memory does not come back at once: the EIGHTH 28 GiB reservation of a 65 536-source context, with ~70 GiB of the process's own in use, waited
        // 4.7 s for the driver to reclaim what the earlier candidates had left -- profiles/r06zzz6_pick_candidates_cost.txt -- where every other one took 0.3 ms. So the candidates'
        // reservations together stay inside what was free when the pick began, less one more set and 8 GiB: seven candidates there, two at 131 072 sources per launch)
        float worst = best;
        size_t free0 = 0, total0 = 0;
        if (hipMemGetInfo(&free0, &total0) != hipSuccess) { (void)hipGetLastError(); free0 = 0; }
        const size_t want = bytes + (bytes >> 3) + 4096;
        for (int k = 1; k < ZHIP_PICK_CANDIDATES; k++) {
            if ((size_t)k * want + want + ((size_t)8 << 30) > free0) break;
            const auto tc0 = std::chrono::steady_clock::now();
            if (cand.reserve(bytes)) { (void)hipGetLastError(); break; }                 // no room for another set: keep what we have
            const auto tc1 = std::chrono::steady_clock::now();
            float ms = 0;
            if (int rc = timeOn((uint8_t*)cand.p, &ms)) return rc;
            if (c->knob.prof) fprintf(stderr, "[zhip-prof] pick candidate %d: reserve %.1f ms, zero + probe %.1f ms (the probe launch %.1f)\n", k,
                                      std::chrono::duration<double, std::milli>(tc1 - tc0).count(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc1).count(), ms);
            if (k < 3) c->e1fPickMs[k] = ms;
            if (ms > worst) worst = ms;
            if (ms < 0.97f * best) { std::swap(c->encFlatTables.p, cand.p); std::swap(c->encFlatTables.cap, cand.cap); std::swap(c->encFlatTables.gen, cand.gen); best = ms; c->e1fPickKept = k; }
            cand.release();
            // (no early stop among the first three: at 131 072 frames per launch the kinds are not two but a spread -- 750, 805, 855, 928 ms, r05n / r05u -- so all three are timed)
        }
        a.flatTables = (uint8_t*)c->encFlatTables.p;
    } else (void)hipGetLastError();
    c->e1fPickedPtr = c->encFlatTables.p;
    return 0;
}
// a chunk's flat match stage: fresh tables, then what the chunk's plan names -- with the split kernel in front and the several-block search behind it where the plan has
// sources of several blocks in the flat kernel. Events 0 .. 1 of the chunk around the kernels.
static int launch_flat_stage(zhip_ctx* c, const ZePlan& p, const ZeChunkPlan& k, ZhipEncodeArgs& a, size_t cnt, ChunkEvents& ev, hipStream_t stream)
{
    // every launch its own number in the tables' cells (the tables serve other sources now), or -- where the cells carry none -- zeroed tables
    bool z = false;
    if (int rc = next_epoch(c, p, a, a.flatTables, c->encFlatTables.gen, p.flatTablesBytes, stream, &z)) return rc;
    if (!z && !p.flatDict) { HIP_TRY(hipMemsetAsync(a.flatTables, 0, cnt * (size_t)a.tableStride, stream)); c->encEpochPtr = nullptr; }      // (cells without numbers in the tables now: the next numbered launch starts from zeroed tables)
    HIP_TRY(ev.record(0, stream));
    a.mbProbes = k.mbProbes;
    if (p.mbc) hipLaunchKernelGGL(zhip_encode_split_kernel, dim3((uint32_t)(cnt < (size_t)c->numCU * 8 ? cnt : (size_t)c->numCU * 8)), dim3(64), 0, stream, a);
    launch_match(k, stream, a);
    if (p.mbc) hipLaunchKernelGGL(zhip_encode_match_flat_mb_kernel, dim3((uint32_t)((cnt + a.mbLanes - 1) / a.mbLanes)), dim3(64), 0, stream, a);
    HIP_TRY(ev.record(1, stream));
    return 0;
}
// the generic one-wave-per-frame kernel over the list the match kernels made, on a workspace and a work counter of its own
static void launch_big_list(const zhip_ctx* c, const ZePlan& p, const ZhipEncodeArgs& a, hipStream_t stream)
{
    ZhipEncodeArgs b = a;
    b.workspace = (uint8_t*)c->encBigWs.p; b.counter = (uint32_t*)((uint8_t*)c->counter.p + ZC_BIG_WORK);
    b.frameList = a.bigList; b.listCount = a.bigCount;
    hipLaunchKernelGGL(zhip_encode_frames_kernel, dim3(p.gBig), dim3(64), 0, stream, b);
}
static int compress_batch_auto(zhip_ctx* c, const void* d_src, const zhip_segment* d_srcSegs, size_t n, void* d_dst, const zhip_segment* d_dstSegs, uint64_t* d_outSizes,
                               int32_t* d_status, hipStream_t stream);
// zhip_compress_batch_device under match finder `finder` (the context's, or one of the two that ZHIP_FINDER_AUTO hands its parts to)
static int compress_batch_with(zhip_ctx* c, int finder, const void* d_src, const zhip_segment* d_srcSegs, size_t n,
                               void* d_dst, const zhip_segment* d_dstSegs, uint64_t* d_outSizes,
                               int32_t* d_status, void* streamv)
{
    if (!c) return ZHIP_ERR_UNSUPPORTED;
    if (n == 0) return 0;
    if (n > 0x7FFFFFFFu) { g_lastError = "too many frames in one launch"; return ZHIP_ERR_UNSUPPORTED; }
    hipStream_t stream = (hipStream_t)streamv;
    if (finder == ZHIP_FINDER_AUTO) return compress_batch_auto(c, d_src, d_srcSegs, n, d_dst, d_dstSegs, d_outSizes, d_status, stream);
    if (c->counter.reserve(64 * 8)) return g_reserveRc;
    uint8_t* const cbase = (uint8_t*)c->counter.p;
    HIP_TRY(hipMemsetAsync(cbase + ZC_E1_WORK, 0, 4, stream));
    ZhipEncodeArgs a; enc_args_init(c, a, d_src, d_srcSegs, n, d_dst, d_dstSegs, d_outSizes, d_status, cbase);
    if (finder == ZHIP_FINDER_WAVE) return compress_batch_wave(c, a, cbase, n, stream);
    if (finder == ZHIP_FINDER_NONE) return compress_batch_none(c, a, cbase, n, stream);
    // the plan: which kernels, how many sources per launch, how much memory (zhip_encode_plan.hpp)
    ZePlanIn in = plan_inputs(c, n);
    ZePlan p = ze_encode_plan(in);
    // the reservations. One that fails at 131 072 sources per launch after all, because another context took the memory in between, is planned again at 65 536
    for (int pass = 0; ; pass++) {
        if (p.flatMaxOpen) { in.flatMax = flat_max_decided(c, p.flatMaxNeed); p = ze_encode_plan(in); }
        if (!(c->encMeta.reserve(p.metaBytes) || c->encArena.reserve(p.arenaBytes) || c->encTables.reserve(p.tablesBytes) || c->encWorkspace.reserve(p.workspaceBytes) ||
              c->encBigList.reserve(p.bigListBytes) || c->encE1List.reserve(p.e1ListBytes) || (p.flat && c->encFlatTables.reserve(p.flatTablesBytes)))) break;
        if (pass || g_reserveRc != ZHIP_ERR_NO_MEMORY || c->knob.echunkMax || c->flatMaxCached <= 65536) return g_reserveRc;
        c->flatMaxCached = 65536; c->encArena.release(); c->encFlatTables.release();      // no room for 131 072 per launch after all: 65 536
    }
    if (p.mbc) {
        if (c->encMbBlocks.reserve(p.mbBlocksBytes) || c->encMbCount.reserve(p.mbCountBytes) || c->encMbSeqs.reserve(p.mbSeqsBytes) || c->encBigWs.reserve(p.bigWsBytes)) return g_reserveRc;
        a.mbBlocks = (ZeMbBlock*)c->encMbBlocks.p; a.mbCount = (uint32_t*)c->encMbCount.p; a.mbSeqs = (uint64_t*)c->encMbSeqs.p;
        a.mbMaxBlocks = p.mbMaxBlocks; a.mbSeqCap = p.mbSeqCap; a.mbLanes = p.mbLanes;
    }
    a.tableStride = p.tableStride; a.arenaStride = p.arenaStride; a.arenaLit = p.arenaLit; a.slotSrcMax = p.slotSrcMax; a.e1Lanes = p.e1Lanes;
    a.workspace = (uint8_t*)c->encWorkspace.p;
    a.meta = (ZeMeta*)c->encMeta.p; a.arena = (uint8_t*)c->encArena.p; a.laneTables = (uint8_t*)c->encTables.p;
    a.flatTables = p.flat ? (uint8_t*)c->encFlatTables.p : nullptr; a.useE1List = p.flat ? 1u : 0u;
    a.e1List = (uint32_t*)c->encE1List.p; a.e1Count = (uint32_t*)(cbase + ZC_E1_COUNT);
    a.bigList = (uint32_t*)c->encBigList.p; a.bigCount = (uint32_t*)(cbase + ZC_BIG_COUNT);
    if (int rc = pick_table_placement(c, p, a, stream)) return rc;
    HIP_TRY(hipMemsetAsync(cbase + ZC_BIG_COUNT, 0, 8, stream));
    if (c->knob.prof) {                                                         // tuning aid: per-phase cycle totals of the entropy kernel
        if (!c->profEncode) HIP_TRY(hipMalloc((void**)&c->profEncode, 16 * 8));
        HIP_TRY(hipMemsetAsync(c->profEncode, 0, 16 * 8, stream));
        a.prof = c->profEncode;
    }
    for (size_t first = 0; first < n; first += p.chunk) {
        const size_t cnt = n - first < p.chunk ? n - first : p.chunk;
        a.first = (uint32_t)first; a.count = (uint32_t)cnt;
        HIP_TRY(hipMemsetAsync(cbase + ZC_E1_WORK, 0, 8, stream));
        HIP_TRY(hipMemsetAsync(cbase + ZC_E1_COUNT, 0, 4, stream));
        ChunkEvents ev;      // the flat match stage: 0 .. 1, the lane-serial match kernel: 2 .. 3, entropy + trailer: 4 .. 5
        if (c->timing) HIP_TRY(ev.create(6));
        if (p.flat) if (int rc = launch_flat_stage(c, p, ze_encode_chunk_plan(in, p, cnt), a, cnt, ev, stream)) return rc;
        HIP_TRY(ev.record(2, stream));
        if (p.greedy) hipLaunchKernelGGL(zhip_encode_match_greedy_kernel, dim3(p.g1), dim3(64), 0, stream, a);      // (takes the chunk's fast / double-fast sources, tiny ones and errors as the kernel below does)
        else hipLaunchKernelGGL(zhip_encode_match_kernel, dim3(p.g1), dim3(64), 0, stream, a);
        HIP_TRY(ev.record(3, stream)); HIP_TRY(ev.record(4, stream));
        launch_entropy(c, a, p.g2, cnt, stream);
        HIP_TRY(ev.record(5, stream));
        if (p.mbc) {      // this chunk's sources of several blocks: the generic kernel over the list the flat kernel just made (it reads the chunk's arenas)
            launch_big_list(c, p, a, stream);
            HIP_TRY(hipMemsetAsync(cbase + ZC_BIG_COUNT, 0, 8, stream));          // list length and the kernel's work counter: fresh for the next chunk
        }
        HIP_TRY(hipGetLastError());
        if (p.flat) ev.give(c->timer[8], 0, 1);
        ev.give(c->timer[5], 2, 3); ev.give(c->timer[6], 4, 5);
    }
    if (a.prof) {
        HIP_TRY(hipStreamSynchronize(stream));
        unsigned long long h[16];
        HIP_TRY(hipMemcpy(h, a.prof, sizeof h, hipMemcpyDeviceToHost));
        static const char* nm[12] = {"gather literals", "literal stats+decide", "huffman build+table", "huffman encode", "sequence stats", "sequence tables", "sequence stream", "frame assembly",
                                      "  stream: constants", "  stream: state chains", "  stream: pack + OR", "  stream: flush"};      // (the last four: -DZE_PROF_STREAM builds only)
        unsigned long long tot = 0; for (int q = 0; q <= ZEP_REST; q++) tot += h[q];
        fprintf(stderr, "[zhip-prof] E2: %.0f wave-cycles per frame\n", (double)tot / (double)n);
        print_prof_rows(h, nm, ZEP_N, tot, (double)n, false);
        a.prof = nullptr;
    }
    if (!p.mbc) {   // inputs above 128 KiB (multi-block frames): the generic one-wave-per-frame kernel over the list E1 made (usually empty)
        if (c->encBigWs.reserve(p.bigWsBytes)) return g_reserveRc;
        launch_big_list(c, p, a, stream);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" int zhip_compress_batch_device(zhip_ctx* c, const void* d_src, const zhip_segment* d_srcSegs, size_t n,
                                          void* d_dst, const zhip_segment* d_dstSegs, uint64_t* d_outSizes,
                                          int32_t* d_status, void* streamv)
{
    if (!c) return ZHIP_ERR_UNSUPPORTED;
    return compress_batch_with(c, c->matchFinder, d_src, d_srcSegs, n, d_dst, d_dstSegs, d_outSizes, d_status, streamv);
}

// ---- ZHIP_FINDER_AUTO (zhip_encode_auto.hpp)
// the classify kernel over a batch, in launches of the plan's chunk: choice bytes (and statistics) at the sources' own indices. The work counter is the first cell of the
// context's encAuto buffer, which the caller has reserved.
static int launch_classify(zhip_ctx* c, const ZeAutoPlan& s, const void* d_src, const zhip_segment* d_srcSegs, size_t n, uint8_t* d_choice, uint32_t* d_stats, hipStream_t stream)
{
    ZhipClassifyArgs k; k.src = (const uint8_t*)d_src; k.srcSegs = (const uint64_t*)d_srcSegs; k.choice = d_choice; k.stats = d_stats; k.counter = (uint32_t*)c->encAuto.p;
    for (size_t first = 0; first < n; first += s.chunk) {
        const size_t cnt = n - first < s.chunk ? n - first : s.chunk;
        k.first = (uint32_t)first; k.count = (uint32_t)cnt;
        HIP_TRY(hipMemsetAsync(k.counter, 0, 4, stream));
        ChunkEvents ev;
        if (c->timing) HIP_TRY(ev.create(2));
        HIP_TRY(ev.record(0, stream));
        hipLaunchKernelGGL(zhip_encode_classify_kernel, dim3((uint32_t)(cnt < s.grid ? cnt : s.grid)), dim3(64), 0, stream, k);
        HIP_TRY(ev.record(1, stream));
        ev.give(c->timer[12], 0, 1);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
extern "C" int zhip_classify_batch_device(zhip_ctx* c, const void* d_src, const zhip_segment* d_srcSegs, size_t n, uint8_t* d_choice, uint32_t* d_stats, void* streamv)
{
    if (!c) return ZHIP_ERR_UNSUPPORTED;
    if (n == 0) return 0;
    if (!d_choice || !d_srcSegs) { g_lastError = "zhip_classify_batch_device: null choice or segment pointer"; return ZHIP_ERR_UNSUPPORTED; }
    if (n > 0x7FFFFFFFu) { g_lastError = "too many frames in one launch"; return ZHIP_ERR_UNSUPPORTED; }
    ZePlanIn in = plan_inputs(c, n); in.n = 0;                    // (no split: the counter's cell only)
    ZeAutoPlan s = ze_auto_plan(in, c->classifyPerCU);
    if (c->encAuto.reserve(s.bytes)) return g_reserveRc;
    in.n = n; s = ze_auto_plan(in, c->classifyPerCU);
    return launch_classify(c, s, d_src, d_srcSegs, n, d_choice, d_stats, (hipStream_t)streamv);
}
// zhip_compress_batch_device under ZHIP_FINDER_AUTO: classify, partition the indices, gather the segment tables, run the two parts through the default finder and the
// literals-only finder as they are -- on the gathered tables and into gathered sizes and statuses -- and scatter those back to the sources' own indices. The two paths'
// launch arguments carry the count by value, so the call WAITS ONCE on the stream, for the two counts (8 bytes); a part that is empty launches nothing.
static int compress_batch_auto(zhip_ctx* c, const void* d_src, const zhip_segment* d_srcSegs, size_t n, void* d_dst, const zhip_segment* d_dstSegs, uint64_t* d_outSizes,
                               int32_t* d_status, hipStream_t stream)
{
    if (const char* why = ze_auto_refusal(c->rows, c->hasCDict)) { g_lastError = why; return ZHIP_ERR_UNSUPPORTED; }
    const ZeAutoPlan s = ze_auto_plan(plan_inputs(c, n), c->classifyPerCU);
    if (c->encAuto.reserve(s.bytes)) return g_reserveRc;
    uint8_t* const base = (uint8_t*)c->encAuto.p;
    ZhipSplitArgs k; memset(&k, 0, sizeof k);
    k.choice = base + s.offChoice; k.n = (uint32_t)n; k.perm = (uint32_t*)(base + s.offPerm); k.counts = (uint32_t*)(base + 4);
    k.srcSegs = (const uint64_t*)d_srcSegs; k.dstSegs = (const uint64_t*)d_dstSegs; k.gSrcSegs = (uint64_t*)(base + s.offSrcSegs); k.gDstSegs = (uint64_t*)(base + s.offDstSegs);
    k.outSizes = d_outSizes; k.status = d_status; k.gOutSizes = (const uint64_t*)(base + s.offOutSizes); k.gStatus = (const int32_t*)(base + s.offStatus);
    if (int rc = launch_classify(c, s, d_src, d_srcSegs, n, base + s.offChoice, nullptr, stream)) return rc;
    hipLaunchKernelGGL(zhip_encode_auto_partition_kernel, dim3(1), dim3(64), 0, stream, k);
    hipLaunchKernelGGL(zhip_encode_auto_gather_kernel, dim3(s.gridMove), dim3(64), 0, stream, k);
    HIP_TRY(hipGetLastError());
    uint32_t counts[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(counts, k.counts, sizeof counts, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));                                  // the one host wait
    if ((size_t)counts[0] + counts[1] != n) { g_lastError = "match finder \"auto\": the split does not cover the batch"; return ZHIP_ERR_HIP; }
    const size_t n0 = counts[0], n1 = counts[1];
    if (n0) if (int rc = compress_batch_with(c, ZHIP_FINDER_LIBZSTD, d_src, (const zhip_segment*)k.gSrcSegs, n0, d_dst, (const zhip_segment*)k.gDstSegs,
                                             (uint64_t*)k.gOutSizes, (int32_t*)k.gStatus, stream)) return rc;
    if (n1) if (int rc = compress_batch_with(c, ZHIP_FINDER_NONE, d_src, (const zhip_segment*)(k.gSrcSegs + 2 * n0), n1, d_dst, (const zhip_segment*)(k.gDstSegs + 2 * n0),
                                             (uint64_t*)k.gOutSizes + n0, (int32_t*)k.gStatus + n0, stream)) return rc;
    hipLaunchKernelGGL(zhip_encode_auto_scatter_kernel, dim3(s.gridMove), dim3(64), 0, stream, k);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Compression from the CALLER's sequences: zhip_compress_batch_device with the match search replaced by a loader (ze_load_sequences_body, a lane per source: checks the
// list, fills the source's arena slot and ZeMeta as a match kernel would) -- the entropy kernel and the trailer kernel behind it are the batch call's, launched the same way.
// Sources of one block only; the arena slots are the full one-block shape (dictionary batches: the dictionary shape, ze_dict_slots), whatever the level's strategy.
extern "C" int zhip_compress_sequences_device(zhip_ctx* c, const void* d_src, const zhip_segment* d_srcSegs, size_t n,
                                              const uint64_t* d_seqs, const zhip_segment* d_seqSegs,
                                              void* d_dst, const zhip_segment* d_dstSegs, uint64_t* d_outSizes,
                                              int32_t* d_status, void* streamv, uint32_t flags)
{
    if (!c) return ZHIP_ERR_UNSUPPORTED;
    if (flags & ~1u) { g_lastError = "zhip_compress_sequences_device: unknown flags"; return ZHIP_ERR_UNSUPPORTED; }
    if (n == 0) return 0;
    if (n > 0x7FFFFFFFu) { g_lastError = "too many frames in one launch"; return ZHIP_ERR_UNSUPPORTED; }
    hipStream_t stream = (hipStream_t)streamv;
    if (c->counter.reserve(64 * 8)) return g_reserveRc;
    uint8_t* const cbase = (uint8_t*)c->counter.p;
    ZhipEncodeArgs a; enc_args_init(c, a, d_src, d_srcSegs, n, d_dst, d_dstSegs, d_outSizes, d_status, cbase);
    const ZePlanIn pin = plan_inputs(c, n);
    ZeSlotPlan s = ze_sequences_plan(pin);
    uint32_t g2 = 0;
    if (int rc = reserve_slots(c, pin.dev, s, a, &g2)) return rc;
    const size_t chunk = s.chunk;
    ZeSeqLoad in; in.seqs = d_seqs; in.table = (const uint64_t*)d_seqSegs; in.copyLits = flags & 1u;
    for (size_t first = 0; first < n; first += chunk) {
        const size_t cnt = n - first < chunk ? n - first : chunk;
        a.first = (uint32_t)first; a.count = (uint32_t)cnt;
        HIP_TRY(hipMemsetAsync(cbase + ZC_E1_WORK, 0, 8, stream));
        hipLaunchKernelGGL(zhip_encode_load_sequences_kernel, dim3((uint32_t)((cnt + 63) / 64)), dim3(64), 0, stream, a, in);
        launch_entropy(c, a, g2, cnt, stream);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
// waves the entropy kernel holds resident on this device (the occupancy query of zhip_ctx_create): batches above it take several frames per wave
extern "C" size_t zhip_ctx_entropy_grid(zhip_ctx* c) { return c ? (size_t)c->numCU * (size_t)c->e2PerCU : 0; }

extern "C" int zhip_ctx_sync(zhip_ctx* c, void* streamv, const int32_t* d_status, size_t n, zhip_error* err)
{
    HIP_TRY(hipStreamSynchronize((hipStream_t)streamv));
    if (err) memset(err, 0, sizeof *err);
    if (!d_status || !n) return 0;
    std::vector<int32_t> st(n);
    HIP_TRY(hipMemcpy(st.data(), d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) if (st[i]) {
        if (err) { err->kind = ZHIP_ERR_ZSTD; err->zstdErr = st[i]; err->index = i; }
        return ZHIP_ERR_ZSTD;
    }
    (void)c;
    return 0;
}

// ------------------------------------------------------------------------------------------ host-buffer batch API
// zhip_compress_batch / zhip_decompress_batch: the reference's multi_*_to_buffer hands over host buffers and gets host buffers back
// (c-ext/compressor.c:1340-1503, c-ext/decompressor.c:1459-1710), so this path is bounded by PCIe (Gen5 x16, ~55 GB/s each way) --
// provided nothing on the host is slower than the link. Round 1 was: one thread packs every item into a pinned buffer, ONE H2D copy,
// kernels, ONE D2H copy into pageable memory (10.5 / 2.6 GB/s). Now the batch is cut into chunks that flow through three streams:
//
//     host threads pack chunk k+1 into pinned staging  |  H2D(k+1)  |  kernels(k)  |  D2H(k-1) straight into the result payload
//
// * staging: two pinned slots, filled by ZHIP_PACK_THREADS host threads (a pageable->pinned memcpy is ~8 GB/s per thread);
// * results: one zhip_outbuf per chunk (the reference returns one buffer per worker as well, the grouping is not contractual), its
//   payload PINNED so that the D2H copy runs at link speed and needs no second host copy. Pinning costs ~0.3 ms per MiB, far more than
//   the copy itself, so payload blocks come from a process-wide pool and return to it when the caller frees them
//   (zhip_free_payload; the CPython extension's BufferWithSegments does that in its deallocator);
// * compress: the compressBound-sized slots are compacted ON THE DEVICE (scan of the frame sizes + one wave per frame) so that only
//   the frames cross the link, into a payload allocated once the chunk's total is known (the host learns it one chunk behind).
#ifndef ZHIP_PACK_THREADS
#define ZHIP_PACK_THREADS 8
#endif
#define ZHIP_HOST_CHUNK_ITEMS 32768u                  // most items of one pipeline chunk (the scan kernel's bound)
// idle pinned bytes kept for reuse; beyond that blocks are unpinned on free. 24 GiB covers a full-size batch's payloads (pinning costs more than
// the copy it speeds up); ZHIP_PIN_POOL_KEEP_MB (read once) lowers or raises it, 0 = keep nothing (no way to trim it before)
static size_t pin_pool_keep()
{
    static const size_t keep = [] { const char* e = getenv("ZHIP_PIN_POOL_KEEP_MB"); return e ? (size_t)strtoull(e, nullptr, 10) << 20 : (size_t)24 << 30; }();
    return keep;
}

static std::atomic<bool> g_pinPortable{false};      // set when the host-buffer calls have more than one device slot to fan out over (dev_pool)
// the process's payload pool (PinPool, zhip_host_pool.hpp) over hipHostMalloc / hipHostFree; leaked on purpose: payloads may outlive static destruction
static PinPool& pin_pool()
{
    static PinPool* pool = new PinPool(
        [](size_t cap) -> void* {
            // (portable -- pinned for every device's copy engines -- only where the in-call fan-out can hand a block to another device: dev_pool sets the flag)
            void* p = nullptr;
            if (hipHostMalloc(&p, cap, g_pinPortable.load() ? hipHostMallocPortable : hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
            return p;
        },
        [](void* p) { (void)hipHostFree(p); }, pin_pool_keep());
    return *pool;
}

extern "C" void zhip_free_payload(void* p) { pin_pool().give(p); }

// sizes -> exclusive offsets (bytes) of the frames of one chunk, total to *total. One workgroup; n <= ZHIP_HOST_CHUNK_ITEMS.
__global__ __launch_bounds__(1024) void zhip_scan_sizes_kernel(const uint64_t* sizes, const int32_t* status, uint32_t n, uint64_t* offs, uint64_t* total)
{
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x, per = (n + 1023) / 1024, lo = t * per, hi = lo + per < n ? lo + per : n;
    uint64_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += status[i] ? 0 : sizes[i];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t run = part[t] - sum;
    for (uint32_t i = lo; i < hi; i++) { offs[i] = run; run += status[i] ? 0 : sizes[i]; }
    if (t == 1023) *total = part[1023];
}
// one wave per frame: the valid prefix of its compressBound-sized slot -> its place in the dense payload
__global__ __launch_bounds__(64) void zhip_compact_kernel(const uint8_t* slots, const zhip_segment* dstSegs, const uint64_t* sizes, const int32_t* status,
                                                           const uint64_t* offs, uint32_t n, uint8_t* dense)
{
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        if (status[i]) continue;
        const uint8_t* s = slots + dstSegs[i].offset; uint8_t* d = dense + offs[i];
        const uint32_t size = (uint32_t)sizes[i], whole = size & ~15u;
        for (uint32_t j = threadIdx.x * 16; j < whole; j += 1024) { const zh_v16 v = zh_ld128(s + j); zh_st64(d + j, v.lo); zh_st64(d + j + 8, v.hi); }
        if (threadIdx.x < size - whole) d[whole + threadIdx.x] = s[whole + threadIdx.x];
    }
}

extern "C" void zhip_ctx_set_size_hint(zhip_ctx* c, uint64_t maxItemBytes) { if (c) c->itemHint = (size_t)maxItemBytes; }

extern "C" int zhip_compact_device(const void* d_slots, const zhip_segment* d_slotSegs, const uint64_t* d_outSizes, const int32_t* d_status,
                                   const uint64_t* d_offsets, size_t n, void* d_dense, void* streamv)
{
    if (n == 0) return 0;
    if (n > 0x7FFFFFFFu) { g_lastError = "too many frames in one launch"; return ZHIP_ERR_UNSUPPORTED; }
    // (the CU count per device is looked up once: hipGetDeviceProperties is slow and this sits on the sharded compress path)
    static thread_local int cuOf[64] = {0};
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    int cus = dev >= 0 && dev < 64 ? cuOf[dev] : 0;
    if (!cus) { HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)); if (dev >= 0 && dev < 64) cuOf[dev] = cus; }
    const size_t gmax = (size_t)cus * 16;
    hipLaunchKernelGGL(zhip_compact_kernel, dim3((uint32_t)(n < gmax ? n : gmax)), dim3(64), 0, (hipStream_t)streamv, (const uint8_t*)d_slots, d_slotSegs, d_outSizes,
                       d_status, d_offsets, (uint32_t)n, (uint8_t*)d_dense);
    HIP_TRY(hipGetLastError());
    return 0;
}

// per-context host pipeline state (streams, staging, small pinned metadata)
static int host_pipe_init(zhip_ctx* c)
{
    if (c->hpReady) return 0;
    HIP_TRY(hipStreamCreateWithFlags(&c->hpH2D, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&c->hpCompute, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&c->hpD2H, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) HIP_TRY(hipEventCreateWithFlags(&c->hpStageFree[i], hipEventDisableTiming));
    c->hpReady = true;
    return 0;
}
// one lazily created context per calling thread, destroyed when the thread exits; re-created when the thread switched devices
struct TlsCtx { zhip_ctx* c = nullptr; ~TlsCtx() { if (c) zhip_ctx_destroy(c); } };
static thread_local TlsCtx g_tls;
static zhip_ctx* tls_ctx()
{
    int dev = -1;
    if (g_tls.c && hipGetDevice(&dev) == hipSuccess && dev != g_tls.c->device) { zhip_ctx_destroy(g_tls.c); g_tls.c = nullptr; }
    if (!g_tls.c) g_tls.c = zhip_ctx_create();
    return g_tls.c;
}
// the host-buffer API keeps its scratch between calls (allocation is slow), but not the tens of GiB a 65 536-frame batch needs
// what memory_size() reports. The reference's contexts exist from the constructor on (ZSTD_sizeof_CCtx > 0 right away, its tests expect that):
// the calling thread's device context is created here if it is not there yet, with the launch counters every call needs.
static std::atomic<size_t> g_slotBytes[64];         // device bytes the device slots' contexts hold (each slot's thread updates its own after a job: fan_out)
extern "C" size_t zhip_thread_memory_size(void)
{
    zhip_ctx* c = tls_ctx();
    if (c) (void)c->counter.reserve(64 * 8);
    size_t n = c ? c->device_bytes() : 0;
    for (int i = 0; i < 64; i++) n += g_slotBytes[i].load();     // (what the in-call fan-out keeps on the node's devices belongs to the caller's picture too)
    return n;
}
// Round 6: a context KEEPS its working set between calls -- the flat search's tables (12 GiB for a 32 768-source chunk), the arenas, the
// device-side staging -- as long as the whole stays within ZHIP_KEEP_GB (default 64: a BASELINE-sized call of 65 536 x 128 KiB holds ~50 GiB of the GPU's
// 288), the way the reference keeps one ZSTD_CCtx per worker between calls (c-ext/compressor.c:1129-1168). Rounds 1-5 released every buffer above 2 GiB after
// every call: the next call re-reserved ~13 GiB of tables (and re-drew their placement). Above the limit the largest buffers go first.
static size_t tls_keep_bytes()
{
    static const size_t keep = [] { const char* e = getenv("ZHIP_KEEP_GB"); return (e ? (size_t)strtoull(e, nullptr, 10) : (size_t)64) << 30; }();
    return keep;
}
static void tls_trim(zhip_ctx* c)      // (which buffers go, and in what order: host_trim_order over the context's one list, its 14 trimmable ones the candidates)
{
#define ZHIP_X(name, trim) &c->name,
    DevBuf* const bufs[] = { ZHIP_CTX_DEVBUFS(ZHIP_X) };
#undef ZHIP_X
#define ZHIP_X(name, trim) trim != 0,
    static const bool trimmable[] = { ZHIP_CTX_DEVBUFS(ZHIP_X) };
#undef ZHIP_X
    const size_t n = sizeof bufs / sizeof bufs[0];
    size_t caps[n];
    for (size_t i = 0; i < n; i++) caps[i] = bufs[i]->cap;
    for (size_t i : host_trim_order(caps, trimmable, n, tls_keep_bytes())) bufs[i]->release();
}
static int set_err(zhip_error* err, int kind, size_t index, int zerr, uint64_t d0 = 0, uint64_t d1 = 0)
{
    if (err) { err->kind = kind; err->index = index; err->zstdErr = zerr; err->detail[0] = d0; err->detail[1] = d1; }
    return kind;
}

extern "C" void zhip_free_outbufs(zhip_outbuf* bufs, size_t n, int freePayload)
{
    if (!bufs) return;
    if (freePayload) for (size_t i = 0; i < n; i++) { zhip_free_payload(bufs[i].data); free(bufs[i].segs); }
    free(bufs);
}

// items [lo, hi) -> their place in the device source arena, in steps of <= ZHIP_STAGE_BYTES (host_upload_step) through the two pinned staging slots: the
// packing of step s+1 (host threads, from ZHIP_PACK_BYTES on) overlaps the H2D copy of step s. Every copy is only ENQUEUED on hpH2D; `done` is recorded behind
// the last one. A slot is reused once the copy that last read it has finished (its event).
#define ZHIP_STAGE_BYTES ((uint64_t)512 << 20)
#define ZHIP_PACK_BYTES ((uint64_t)32 << 20)
static int upload_items(zhip_ctx* c, const zhip_item* items, const zhip_segment* segs, size_t lo, size_t hi, hipEvent_t done)
{
    for (size_t a = lo; a < hi;) {
        const HostStep st = host_upload_step(segs, a, hi, ZHIP_STAGE_BYTES);
        const int slot = c->hpNextSlot; c->hpNextSlot ^= 1;
        if (hipEventSynchronize(c->hpStageFree[slot]) != hipSuccess) return ZHIP_ERR_HIP;
        if (c->hpStage[slot].reserve(st.bytes + 16, 3) != hipSuccess) return ZHIP_ERR_HIP;
        pack_items((uint8_t*)c->hpStage[slot].p, items, segs, st.a, st.b, ZHIP_PACK_BYTES, c->knob.packThreads ? c->knob.packThreads : ZHIP_PACK_THREADS);
        if (st.bytes && hipMemcpyAsync((uint8_t*)c->hSrc.p + segs[a].offset, c->hpStage[slot].p, st.bytes, hipMemcpyHostToDevice, c->hpH2D) != hipSuccess) return ZHIP_ERR_HIP;
        if (hipEventRecord(c->hpStageFree[slot], c->hpH2D) != hipSuccess) return ZHIP_ERR_HIP;
        a = st.b;
    }
    return hipEventRecord(done, c->hpH2D) == hipSuccess ? 0 : ZHIP_ERR_HIP;
}
static void empty_outbuf(zhip_outbuf* ob) { ob->data = malloc(1); ob->segs = (zhip_segment*)malloc(sizeof(zhip_segment)); ob->dataSize = 0; ob->nSegs = 0; }

// One host-buffer call on ONE device (the calling thread's current one): what the two directions share around their chunk loops. It owns the call's events and its
// output array: however the call ends the events are destroyed, and the outputs freed unless finish() handed them to the caller. The plan -- segments, cuts, meta
// layouts, verdicts -- is zhip_host_calls.hpp's.
struct HostCall {
    const bool compress;
    zhip_ctx* c; zhip_error* err;
    zhip_outbuf* ob = nullptr; size_t nOb = 0;      // one output per chunk (one empty one for no chunk)
    hipEvent_t evUp = nullptr, evK = nullptr;       // behind a chunk's upload; decompress: behind its kernels
    std::vector<hipEvent_t> evMeta;                 // compress: behind a chunk's sizes, status and total on their way back
    HostCall(bool compress_, zhip_outbuf** out, size_t* nOut, zhip_error* err_) : compress(compress_), err(err_)
    {
        if (err) memset(err, 0, sizeof *err);
        *out = nullptr; *nOut = 0;
        c = tls_ctx();
    }
    ~HostCall() { release(); }
    HostCall(const HostCall&) = delete;
    void drop_events()
    {
        for (auto& e : evMeta) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        if (evUp) (void)hipEventDestroy(evUp);
        if (evK) (void)hipEventDestroy(evK);
        evUp = evK = nullptr;
    }
    void release() { drop_events(); if (ob) zhip_free_outbufs(ob, nOb, 1); ob = nullptr; }
    int fail(int kind, size_t index = 0, int zerr = 0, uint64_t d0 = 0, uint64_t d1 = 0)
    {
        if (kind == ZHIP_ERR_HIP) hip_fail(hipGetLastError(), compress ? "host compress pipeline" : "host decompress pipeline");
        (void)hipDeviceSynchronize();          // nothing of the call still runs when its events and its outputs go
        release();
        return set_err(err, kind, index, zerr, d0, d1);
    }
    // the prologue behind pass 1 and the cuts: streams, arenas (compress: the dense frames too), the meta areas of the direction's layout, an output per chunk, the
    // events, and the segment table on the device
    int begin(const std::vector<zhip_segment>& segs, size_t n, size_t nChunks, uint64_t srcTotal, uint64_t dstTotal, size_t dBytes, size_t hBytes)
    {
        if (host_pipe_init(c)) return set_err(err, ZHIP_ERR_HIP, 0, 0);
        if (c->hSrc.reserve(srcTotal + 16) || c->hDst.reserve(dstTotal + 16) || (compress && c->hDense.reserve(dstTotal + 16)) ||
            c->hSegs.reserve(2 * n * sizeof(zhip_segment) + 16) || c->hStatus.reserve(dBytes)) return set_err(err, g_reserveRc, 0, 0);
        if (const hipError_t e = c->pinned.reserve(hBytes, 2)) return set_err(err, hip_fail(e, "hipHostMalloc"), 0, 0);
        ob = (zhip_outbuf*)calloc(nChunks ? nChunks : 1, sizeof(zhip_outbuf));
        if (!ob) return set_err(err, ZHIP_ERR_NO_MEMORY, 0, 0);
        nOb = nChunks ? nChunks : 1;
        if (compress) evMeta.assign(nChunks, nullptr);
        if (hipEventCreateWithFlags(&evUp, hipEventDisableTiming) != hipSuccess || (!compress && hipEventCreateWithFlags(&evK, hipEventDisableTiming) != hipSuccess)) return fail(ZHIP_ERR_HIP);
        if (hipMemcpyAsync(c->hSegs.p, segs.data(), 2 * n * sizeof(zhip_segment), hipMemcpyHostToDevice, c->hpH2D) != hipSuccess ||
            hipStreamSynchronize(c->hpH2D) != hipSuccess) return fail(ZHIP_ERR_HIP);      // segs is pageable: wait before anything reads the table
        return 0;
    }
    // the epilogue: everything has arrived ..
    int drain() { return hipStreamSynchronize(c->hpD2H) != hipSuccess || hipStreamSynchronize(c->hpCompute) != hipSuccess ? fail(ZHIP_ERR_HIP) : 0; }
    // .. and the outputs are the caller's
    int finish(zhip_outbuf** out, size_t* nOut, size_t nChunks)
    {
        drop_events();
        if (nChunks == 0) empty_outbuf(&ob[0]);
        *out = ob; *nOut = nOb; ob = nullptr;
        tls_trim(c);
        return ZHIP_ERR_NONE;
    }
};

// decompress: the chunked three-stream pipeline
static int decompress_batch_one(const zhip_dparams* params, const zhip_item* items, size_t n, int requireSizes,
                                zhip_outbuf** out, size_t* nOut, zhip_error* err)
{
    const bool allowShort = (requireSizes & 2) != 0;   // dstSize is a capacity (one-shot decompress with max_output_size)
    HostCall call(false, out, nOut, err);
    zhip_ctx* c = call.c;
    if (!c) return set_err(err, ZHIP_ERR_HIP, 0, 0);
    std::vector<zhip_segment> segs(2 * n);           // [0,n) source, [n,2n) destination
    std::vector<uint32_t> nBlocks(n);                // blocks per frame (0: unknown), from the block headers (host_count_blocks)
    const int format = params ? params->format : ZHIP_FORMAT_ZSTD1;
    uint64_t srcTotal = 0, dstTotal = 0;
    const HostRefusal no = host_decompress_segments(items, n, format, segs.data(), nBlocks.data(), &srcTotal, &dstTotal);
    if (no.kind) return set_err(err, no.kind, no.index, 0);
    int r = zhip_ctx_set_dformat(c, format, params ? params->maxWindowSize : 0);
    if (r) return set_err(err, r, 0, 0);
    r = zhip_ctx_set_ddict(c, params ? params->dict : nullptr, params ? params->dictSize : 0, params ? params->dictType : ZHIP_DICT_AUTO);
    if (r < 0) return set_err(err, ZHIP_ERR_ZSTD, 0, -r);
    if (r) return set_err(err, r, 0, 0);
    // the kernels are several times faster than the link here: chunks of ~1 GiB of output keep all three streams busy
    // (a small FIRST chunk -- ZHIP_HCHUNK_D0 items, default 2 048 for batches above 8 192 -- starts the copy back, which is what the call waits for, a few ms after
    // the call instead of after a whole chunk's packing, upload and kernels)
    const std::vector<size_t> cut = host_chunks(segs.data(), n, (uint64_t)1 << 30, 32768, n > 8192 ? c->knob.hchunkD0 : 0);
    const size_t nChunks = cut.size() - 1;
    const HostDecompressLayout l = host_decompress_layout(n);
    if (const int e = call.begin(segs, n, nChunks, srcTotal, dstTotal, l.dBytes, l.hBytes)) return e;
    uint64_t* dSizes = (uint64_t*)((uint8_t*)c->hStatus.p + l.dSizes);
    int32_t* dStatus = (int32_t*)((uint8_t*)c->hStatus.p + l.dStatus);
    uint64_t* hSizes = (uint64_t*)((uint8_t*)c->pinned.p + l.hSizes);
    int32_t* hStatus = (int32_t*)((uint8_t*)c->pinned.p + l.hStatus);
    const zhip_segment* dSegs = (const zhip_segment*)c->hSegs.p;
    zhip_outbuf* ob = call.ob;
    // payloads, sizes and statuses all go back on the third stream, and every item is judged once everything has arrived
    for (size_t k = 0; k < nChunks; k++) {
        const size_t lo = cut[k], hi = cut[k + 1], cnt = hi - lo;
        const uint64_t outBytes = segs[n + hi - 1].offset + segs[n + hi - 1].length - segs[n + lo].offset;
        if (upload_items(c, items, segs.data(), lo, hi, call.evUp)) return call.fail(ZHIP_ERR_HIP);
        if (hipStreamWaitEvent(c->hpCompute, call.evUp, 0) != hipSuccess) return call.fail(ZHIP_ERR_HIP);
        ZdHints hint = zd_host_hint(&segs[n + lo].length, 2, nBlocks.data() + lo, cnt);      // (the frames' content sizes: the length of every destination segment)
        if (!hint.size) hint.size = c->itemHint;
        r = decompress_batch(c, hint, c->hSrc.p, dSegs + lo, cnt, c->hDst.p, dSegs + n + lo, dSizes + lo, dStatus + lo, c->hpCompute);
        if (r) return call.fail(r);
        if (hipEventRecord(call.evK, c->hpCompute) != hipSuccess || hipStreamWaitEvent(c->hpD2H, call.evK, 0) != hipSuccess) return call.fail(ZHIP_ERR_HIP);
        // the chunk's output goes straight into its (pinned) result payload
        ob[k].data = pin_pool().take((size_t)outBytes);
        ob[k].segs = (zhip_segment*)malloc((cnt ? cnt : 1) * sizeof(zhip_segment));
        if (!ob[k].data || !ob[k].segs) return call.fail(ZHIP_ERR_NO_MEMORY, lo);
        ob[k].dataSize = (size_t)outBytes; ob[k].nSegs = cnt;
        if ((outBytes && hipMemcpyAsync(ob[k].data, (uint8_t*)c->hDst.p + segs[n + lo].offset, outBytes, hipMemcpyDeviceToHost, c->hpD2H) != hipSuccess) ||
            hipMemcpyAsync(hSizes + lo, dSizes + lo, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost, c->hpD2H) != hipSuccess ||
            hipMemcpyAsync(hStatus + lo, dStatus + lo, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, c->hpD2H) != hipSuccess) return call.fail(ZHIP_ERR_HIP);
    }
    if (const int e = call.drain()) return e;
    for (size_t k = 0; k < nChunks; k++) {
        const HostVerdict v = host_decompress_verdict(segs.data() + n, hSizes, hStatus, cut[k], cut[k + 1], allowShort, ob[k].segs);
        if (v.kind) return call.fail(v.kind, v.index, v.zerr, v.d0, v.d1);
    }
    return call.finish(out, nOut, nChunks);
}

static int compress_batch_one(const zhip_cparams* params, const zhip_item* items, size_t n, zhip_outbuf** out, size_t* nOut, zhip_error* err)
{
    HostCall call(true, out, nOut, err);
    zhip_ctx* c = call.c;
    if (!c) return set_err(err, ZHIP_ERR_HIP, 0, 0);
    zhip_cparams defaults; memset(&defaults, 0, sizeof defaults);
    defaults.level = 3; defaults.contentSizeFlag = 1; defaults.dictIDFlag = 1;
    int r = zhip_ctx_set_cparams(c, params ? params : &defaults);
    if (r < 0) return set_err(err, ZHIP_ERR_ZSTD, 0, -r);
    if (r) return set_err(err, r, 0, 0);
    if (n == 0) {                                     // nothing to compress: the parameters / dictionary have been digested (what precompute_compress asks for)
        zhip_outbuf* e = (zhip_outbuf*)calloc(1, sizeof(zhip_outbuf));
        if (!e) return set_err(err, ZHIP_ERR_NO_MEMORY, 0, 0);
        empty_outbuf(e); *out = e; *nOut = 1;
        return ZHIP_ERR_NONE;
    }
    std::vector<zhip_segment> segs(2 * n);
    uint64_t srcTotal = 0, dstTotal = 0;
    const HostRefusal no = host_compress_segments(items, n, segs.data(), &srcTotal, &dstTotal);
    if (no.kind) { g_lastError = no.text; return set_err(err, no.kind, no.index, 0); }
    // the match kernel is a per-frame latency chain (its time barely depends on the batch below ~16 K frames), so compress chunks are
    // large: two of them overlap one's upload with the other's kernels, more would only add chains end to end
    // (round 4 ran these chunks side by side on their own streams, each in its own part of the encode arenas -- +8 % at best and an unexplained 5 x
    // slow mode in three of eight configurations; removed in round 5, git tag r04-experiments has it. The ceiling of this shape is the search:
    // 65 536 frames are 410-480 ms of transaction-bound work however they are cut, with the first chunk's upload in front and entropy coding,
    // compaction and the copy back behind: DESIGN.md section 3.)
    const std::vector<size_t> cut = host_chunks(segs.data(), n, (uint64_t)4 << 30, c->knob.hchunkE, n > c->knob.hchunkE ? c->knob.hchunkE0 : 0);
    const size_t nChunks = cut.size() - 1;
    // device: sources, slots, dense frames, segment table, [sizes | offsets | chunk totals | status]
    const HostCompressLayout l = host_compress_layout(n, nChunks);
    if (const int e = call.begin(segs, n, nChunks, srcTotal, dstTotal, l.dBytes, l.hBytes)) return e;
    uint8_t* dMeta = (uint8_t*)c->hStatus.p; uint8_t* hMeta = (uint8_t*)c->pinned.p;
    uint64_t* dSizes = (uint64_t*)(dMeta + l.dSizes); uint64_t* dOffs = (uint64_t*)(dMeta + l.dOffs); uint64_t* dTotals = (uint64_t*)(dMeta + l.dTotals); int32_t* dStatus = (int32_t*)(dMeta + l.dStatus);
    uint64_t* hSizes = (uint64_t*)(hMeta + l.hSizes); uint64_t* hTotals = (uint64_t*)(hMeta + l.hTotals); int32_t* hStatus = (int32_t*)(hMeta + l.hStatus);
    const zhip_segment* dSegs = (const zhip_segment*)c->hSegs.p;
    zhip_outbuf* ob = call.ob;
    // the host learns a chunk's total one chunk behind: while chunk k is being packed / copied / compressed, chunk k-1's sizes have
    // arrived, its payload is allocated (exact size) and its frames travel back on the third stream
    auto collect = [&](size_t k) -> int {
        const size_t lo = cut[k], hi = cut[k + 1], cnt = hi - lo;
        if (hipEventSynchronize(call.evMeta[k]) != hipSuccess) return call.fail(ZHIP_ERR_HIP);
        (void)hipEventDestroy(call.evMeta[k]); call.evMeta[k] = nullptr;
        const HostVerdict v = host_compress_verdict(hStatus, lo, hi);
        if (v.kind) return call.fail(v.kind, v.index, v.zerr);
        const uint64_t total = hTotals[k];
        ob[k].data = pin_pool().take((size_t)total);
        ob[k].segs = (zhip_segment*)malloc((cnt ? cnt : 1) * sizeof(zhip_segment));
        if (!ob[k].data || !ob[k].segs) return call.fail(ZHIP_ERR_NO_MEMORY, lo);
        ob[k].dataSize = (size_t)total; ob[k].nSegs = cnt;
        (void)host_compress_out_segments(hSizes, lo, hi, ob[k].segs);
        // the compaction finished before evMeta (same stream), so the copy needs no further dependency
        if (total && hipMemcpyAsync(ob[k].data, (uint8_t*)c->hDense.p + segs[n + lo].offset, total, hipMemcpyDeviceToHost, c->hpD2H) != hipSuccess) return call.fail(ZHIP_ERR_HIP);
        return 0;
    };
    for (size_t k = 0; k < nChunks; k++) {
        const size_t lo = cut[k], hi = cut[k + 1], cnt = hi - lo;
        hipStream_t sk = c->hpCompute;
        if (upload_items(c, items, segs.data(), lo, hi, call.evUp)) return call.fail(ZHIP_ERR_HIP);
        if (hipStreamWaitEvent(sk, call.evUp, 0) != hipSuccess) return call.fail(ZHIP_ERR_HIP);
        { size_t mx = 0; for (size_t i = lo; i < hi; i++) if (items[i].srcSize > mx) mx = items[i].srcSize; c->srcMaxHint = mx; }
        r = zhip_compress_batch_device(c, c->hSrc.p, dSegs + lo, cnt, c->hDst.p, dSegs + n + lo, dSizes + lo, dStatus + lo, sk);
        c->srcMaxHint = 0;
        if (r) return call.fail(r);
        hipLaunchKernelGGL(zhip_scan_sizes_kernel, dim3(1), dim3(1024), 0, sk, dSizes + lo, dStatus + lo, (uint32_t)cnt, dOffs + lo, dTotals + k);
        const uint32_t gridC = (uint32_t)(cnt < (size_t)c->numCU * 16 ? cnt : (size_t)c->numCU * 16);
        hipLaunchKernelGGL(zhip_compact_kernel, dim3(gridC ? gridC : 1), dim3(64), 0, sk, (const uint8_t*)c->hDst.p, dSegs + n + lo, dSizes + lo, dStatus + lo,
                           dOffs + lo, (uint32_t)cnt, (uint8_t*)c->hDense.p + segs[n + lo].offset);
        // sizes, status and the chunk total ride the compute stream (a few hundred KiB) so that nothing queues behind a later chunk's kernels
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(hSizes + lo, dSizes + lo, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost, sk) != hipSuccess ||
            hipMemcpyAsync(hStatus + lo, dStatus + lo, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, sk) != hipSuccess ||
            hipMemcpyAsync(hTotals + k, dTotals + k, sizeof(uint64_t), hipMemcpyDeviceToHost, sk) != hipSuccess ||
            hipEventCreateWithFlags(&call.evMeta[k], hipEventDisableTiming) != hipSuccess || hipEventRecord(call.evMeta[k], sk) != hipSuccess) return call.fail(ZHIP_ERR_HIP);
        if (k >= 1) { const int e = collect(k - 1); if (e) return e; }
    }
    if (nChunks) { const int e = collect(nChunks - 1); if (e) return e; }
    if (const int e = call.drain()) return e;
    return call.finish(out, nOut, nChunks);
}


// ------------------------------------------------------------------------------------------ one call, every device (round 6)
// The reference fans a batch out INSIDE multi_compress_to_buffer / multi_decompress_to_buffer: bytesPerWorker = total / workers, a contiguous run of
// items per worker, one destination buffer set per worker, the collection in worker order, the first failing item reported (c-ext/compressor.c:1127-1298,
// c-ext/decompressor.c:1237-1455). Here a worker is a DEVICE: zhip_compress_batch / zhip_decompress_batch cut the item list by the same rule, hand every
// run to a host thread bound to its device (one persistent thread + one context + its own staging per device slot; the pinned payload pool is the process's),
// and return the devices' zhip_outbufs in device order -- which is item order. No collective: the collection holds one BufferWithSegments per chunk of each
// device. ZHIP_DEVICES=0,1,... selects the device slots (a device may be listed twice: two contexts on one GPU -- how the split is tested on a
// one-GPU box); unset = every visible device, but never more devices than ZHIP_DEVICE_MIN_BYTES (default 256 MiB) of input each -- small batches stay on the
// calling thread's current device, exactly as before.
// The rules -- the partition, the device list, the slot count, the merge -- are zhip_host_calls.hpp's; the threads and the contexts are here.
extern "C" size_t zhip_partition_by_bytes(const uint64_t* sizes, size_t n, size_t workers, size_t* bounds) { return host_partition_by_bytes(sizes, n, workers, bounds); }

// the process's device slots (DevPool, zhip_host_pool.hpp): the environment and the device count are read once, on the first call that asks; leaked on purpose like its threads
static DevPool& dev_pool()
{
    static DevPool* pool = [] {
        DevPool* p = new DevPool([](int device) { (void)hipSetDevice(device); });
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess) { (void)hipGetLastError(); count = 0; }
        p->parse(count, getenv("ZHIP_DEVICES"), getenv("ZHIP_DEVICE_MIN_BYTES"));
        if (p->slots.size() > 1) g_pinPortable.store(true);       // payload blocks serve any device's copy engines from the first one on
        return p;
    }();
    return *pool;
}
// one call over d slots (host_fan_out). What stays here is what a slot's thread does after its run: it keeps its thread's error text for the merge and publishes what its
// context holds for memory_size()
template <typename F>
static int fan_out(size_t d, const zhip_item* items, size_t n, F&& one, zhip_outbuf** out, size_t* nOut, zhip_error* err)
{
    if (err) memset(err, 0, sizeof *err);
    *out = nullptr; *nOut = 0;
    std::vector<uint64_t> sizes(n);
    for (size_t i = 0; i < n; i++) sizes[i] = items[i].srcSize;
    auto after = [](size_t w, int rc) {
        if (w < 64 && g_tls.c) g_slotBytes[w].store(g_tls.c->device_bytes());
        return rc ? g_lastError : std::string();
    };
    return host_fan_out(dev_pool(), d, sizes.data(), n, one, after, [](zhip_outbuf* b, size_t k) { zhip_free_outbufs(b, k, 1); }, out, nOut, err, &g_lastError);
}

extern "C" int zhip_batch_devices(int* devices, int cap)
{
    const DevPool& p = dev_pool();
    for (int i = 0; i < cap && i < (int)p.slots.size(); i++) devices[i] = p.slots[i];
    return (int)p.slots.size();
}

extern "C" int zhip_compress_batch(const zhip_cparams* params, const zhip_item* items, size_t n, zhip_outbuf** out, size_t* nOut, zhip_error* err)
{
    uint64_t bytes = 0;
    for (size_t i = 0; i < n; i++) bytes += items[i].srcSize;
    const size_t d = dev_pool().slotsFor(n, bytes);
    if (d == 0) return compress_batch_one(params, items, n, out, nOut, err);
    return fan_out(d, items, n, [=](size_t lo, size_t hi, zhip_outbuf** o, size_t* no, zhip_error* e) { return compress_batch_one(params, items + lo, hi - lo, o, no, e); }, out, nOut, err);
}

extern "C" int zhip_decompress_batch(const zhip_dparams* params, const zhip_item* items, size_t n, int requireSizes,
                                     zhip_outbuf** out, size_t* nOut, zhip_error* err)
{
    // the reference's decompress dispatcher balances by COMPRESSED bytes (decompressor.c:1237-1320: framePointers' sourceSize)
    uint64_t bytes = 0, outBytes = 0;
    for (size_t i = 0; i < n; i++) { bytes += items[i].srcSize; outBytes += items[i].dstSize; }
    const size_t d = dev_pool().slotsFor(n, outBytes > bytes ? outBytes : bytes);
    if (d == 0) return decompress_batch_one(params, items, n, requireSizes, out, nOut, err);
    return fan_out(d, items, n, [=](size_t lo, size_t hi, zhip_outbuf** o, size_t* no, zhip_error* e) { return decompress_batch_one(params, items + lo, hi - lo, requireSizes, o, no, e); }, out, nOut, err);
}

// ------------------------------------------------------------------------------------------ seekable streams (zhip_seekable.hpp)
// One large buffer as the batch the kernels are fast at: chunks of frameSize bytes -> zhip_compress_batch_device -> frames back to back + the seek table;
// a range read is zhip_decompress_batch_device over the frames that cover it. Everything between the batch calls is the small kernels of zhip_seekable.hpp,
// queued on the caller's stream: no call here waits on the host except where scratch grows, and zhip_seekable_open_device, which reads the table's shape.
struct zhip_seekable : ZskTypedOpened {
    // the pinned slots the many-ranges call's tables are uploaded from (a slot is written again only after the event behind its upload has completed). Declared first, so they
    // go last: behind the device buffers, whose hipFree waits for the device like the synchronise in zhip_seekable_close
    std::deque<ZskPinSlot> slots;
    DevBuf prefix;                       // the table's scans (ZskOpened::pre points into it)
    DevBuf meta, edge;                   // a range call's segments / sizes / statuses, and where its partly covered frames are decoded
    // the many-ranges call: its plan's tables on the device, its item arrays and per-range words, its scratch frames
    DevBuf gTables, gMeta, gScratch;
    DevBuf tPlanar, tTables, tStatus;     // a typed read: the planar buffer the many-ranges call fills (at exactly its bytes), the jobs and owners, the passes' status arrays
    DevBuf tTileSums;                     // a read of a delta-filtered stream: a uint64 per tile of its largest pass
};

// a pinned slot of at least `bytes` that no upload still reads: one whose event has completed (grown where too small), else a new one
static int zsk_take_slot(std::deque<ZskPinSlot>& slots, size_t bytes, ZskPinSlot** out)
{
    ZskPinSlot* s = nullptr;
    for (ZskPinSlot& x : slots) if (hipEventQuery(x.done) == hipSuccess) { s = &x; break; }
    (void)hipGetLastError();                                               // (hipErrorNotReady of a slot still in flight is no failure)
    if (!s) {
        hipEvent_t done = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        slots.emplace_back(); s = &slots.back(); s->done = done;
    }
    if (s->pin.reserve(bytes, 2) != hipSuccess) { (void)hipGetLastError(); g_lastError = "seekable: no pinned memory for the call's tables"; return ZHIP_ERR_NO_MEMORY; }
    *out = s;
    return 0;
}

// The backend the sequences of zhip_seekable_calls.hpp run over: the context's and the handle's areas, the kernels on the caller's stream
struct ZskHipBackend {
    zhip_ctx* c; zhip_seekable* h; hipStream_t stream;
    int numCU; std::string& err;
    ZskPinSlot* slot = nullptr;
    ZskHipBackend(zhip_ctx* c_, zhip_seekable* h_, void* streamv) : c(c_), h(h_), stream((hipStream_t)streamv), numCU(c_ ? c_->numCU : 0), err(g_lastError) {}
    int reserve(ZskArea area, size_t bytes, uint8_t** base)
    {
        if (area == ZSK_A_PIN) {
            if (int rc = zsk_take_slot(h ? h->slots : c->skPins, bytes, &slot)) return rc;
            *base = (uint8_t*)slot->pin.p;
            return 0;
        }
        if (area == ZSK_A_G_SCRATCH) {      // at exactly its bytes
            if (int rc = h->gScratch.reserve_exact(bytes)) return rc;
            *base = (uint8_t*)h->gScratch.p;
            return 0;
        }
        DevBuf& d = area == ZSK_A_SK_META ? c->skMeta : area == ZSK_A_SK_SLOTS ? c->skSlots : area == ZSK_A_PREFIX ? h->prefix : area == ZSK_A_META ? h->meta : area == ZSK_A_EDGE ? h->edge :
                    area == ZSK_A_G_TABLES ? h->gTables : h->gMeta;
        if (d.reserve(bytes)) return g_reserveRc;
        *base = (uint8_t*)d.p;
        return 0;
    }
    void launch(ZskKernel k, uint32_t grid, const void* args)
    {
#define ZSK_X(id, name, A) case ZSK_K_##id: hipLaunchKernelGGL(zhip_seekable_##name##_kernel, dim3(grid), dim3(64), 0, stream, *(const A*)args); break;
        switch (k) { ZSK_KERNELS(ZSK_X) default: break; }
#undef ZSK_X
    }
    int check() { HIP_TRY(hipGetLastError()); return 0; }
    int compress(const uint8_t* src, const uint64_t* srcSegs, size_t n, uint8_t* slots, const uint64_t* slotSegs, uint64_t* outSizes, int32_t* status, size_t srcMax)
    {
        const size_t hintWas = c->srcMaxHint;
        c->srcMaxHint = srcMax;
        const int rc = zhip_compress_batch_device(c, src, (const zhip_segment*)srcSegs, n, slots, (const zhip_segment*)slotSegs, outSizes, status, stream);
        c->srcMaxHint = hintWas;
        return rc;
    }
    int decompress(const ZskOpened& o, const uint64_t* srcSegs, size_t n, uint8_t* dstBase, const uint64_t* dstSegs, uint64_t* outSizes, int32_t* status)
    {
        // what the readers tell the batch decode about their frames. Frames above one block: the several-block mode, for these launches only
        ZdHints hint; hint.size = o.maxFrameContent > ZF_BLOCK_MAX ? (uint64_t)o.maxFrameContent : (uint64_t)c->itemHint;
        return decompress_batch(c, hint, o.stream, (const zhip_segment*)srcSegs, n, dstBase, (const zhip_segment*)dstSegs, outSizes, status, stream);
    }
    void compact(uint32_t grid, const uint8_t* slots, const uint64_t* slotSegs, const uint64_t* sizes, const int32_t* status, const uint64_t* offs, uint32_t n, uint8_t* dst)
    {
        hipLaunchKernelGGL(zhip_compact_kernel, dim3(grid), dim3(64), 0, stream, slots, (const zhip_segment*)slotSegs, sizes, status, offs, n, dst);
    }
    int zero(void* p, size_t bytes) { HIP_TRY(hipMemsetAsync(p, 0, bytes, stream)); return 0; }
    int copy(void* dst, const void* src, size_t bytes, ZskCopy kind)
    {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind == ZSK_COPY_TO_HOST ? hipMemcpyDeviceToHost : kind == ZSK_COPY_FROM_PIN ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, stream));
        if (kind == ZSK_COPY_FROM_PIN) HIP_TRY(hipEventRecord(slot->done, stream));
        return 0;
    }
    int wait() { HIP_TRY(hipStreamSynchronize(stream)); return 0; }
};
// and what the typed calls of zhip_seekable_typed_calls.hpp need on top: their areas, their kernels
struct ZskHipTypedBackend : ZskHipBackend {
    using ZskHipBackend::ZskHipBackend;
    int reserve_typed(ZskTypedArea area, size_t bytes, uint8_t** base)
    {
        if (area == ZSKT_A_PLANAR) {        // at exactly its bytes, as the many-ranges scratch
            if (int rc = h->tPlanar.reserve_exact(bytes)) return rc;
            *base = (uint8_t*)h->tPlanar.p;
            return 0;
        }
        DevBuf& d = area == ZSKT_A_STAGING ? c->skStaging : area == ZSKT_A_RECORDS ? c->skRecords : area == ZSKT_A_STASH ? c->skStash : area == ZSKT_A_TABLES ? h->tTables :
                    area == ZSKT_A_TILESUMS ? (h ? h->tTileSums : c->skTileSums) : h->tStatus;
        if (d.reserve(bytes)) return g_reserveRc;
        *base = (uint8_t*)d.p;
        return 0;
    }
    void launch_typed(ZskTypedKernel k, uint32_t grid, const void* args)
    {
#define ZSKT_X(id, name, A) case ZSKT_K_##id: hipLaunchKernelGGL(zhip_seekable_##name##_kernel, dim3(grid), dim3(64), 0, stream, *(const A*)args); break;
        switch (k) { ZSKT_KERNELS(ZSKT_X) default: break; }
#undef ZSKT_X
    }
};

extern "C" uint64_t zhip_seekable_frame_count(uint64_t srcSize, uint32_t frameSize) { return zsk_frame_count(srcSize, frameSize); }
extern "C" uint64_t zhip_seekable_bound(uint64_t srcSize, uint32_t frameSize, int flags)
{
    if (flags & ~ZHIP_SEEKABLE_CHECKSUM) return 0;
    return zsk_bound(srcSize, frameSize, flags & ZHIP_SEEKABLE_CHECKSUM);
}

extern "C" int zhip_seekable_compress_device(zhip_ctx* c, const void* d_src, uint64_t srcSize, uint32_t frameSize, int flags,
                                             void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status, void* streamv)
{
    ZskHipBackend b(c, nullptr, streamv);
    return zsk_compress(b, c != nullptr, d_src, srcSize, frameSize, flags, d_dst, dstCapacity, d_streamSize, d_status);
}

extern "C" uint64_t zhip_seekable_records_bound(uint64_t maxContentBytes, uint64_t nRecords, int flags)
{
    if (flags & ~ZHIP_SEEKABLE_CHECKSUM) return 0;
    return zsk_records_bound(maxContentBytes, nRecords, flags & ZHIP_SEEKABLE_CHECKSUM);
}

extern "C" int zhip_seekable_compress_records_device(zhip_ctx* c, const void* d_src, uint64_t srcSize, const zhip_segment* d_records, size_t nRecords,
                                                     uint64_t maxContentBytes, uint64_t maxRecordBytes, int flags,
                                                     void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status, void* streamv)
{
    ZskHipBackend b(c, nullptr, streamv);
    return zsk_compress_records(b, c != nullptr, d_src, srcSize, d_records, nRecords, maxContentBytes, maxRecordBytes, flags, d_dst, dstCapacity, d_streamSize, d_status);
}

extern "C" void zhip_seekable_close(zhip_seekable* h)
{
    if (!h) return;
    (void)hipDeviceSynchronize();      // no upload from a slot, no kernel over a buffer is in flight when the handle's members release themselves
    delete h;
}

extern "C" int zhip_seekable_open_device(zhip_ctx* c, const void* d_stream, uint64_t streamSize, void* streamv, zhip_seekable** out, zhip_seekable_info* info, zhip_error* err)
{
    if (err) memset(err, 0, sizeof *err);
    if (out) *out = nullptr;
    if (!c || !d_stream || !out) { g_lastError = "seekable open: bad arguments"; return set_err(err, ZHIP_ERR_UNSUPPORTED, 0, 0); }
    zhip_seekable* h = new zhip_seekable();
    ZskHipTypedBackend b(c, h, streamv);
    int zerr = 0; size_t index = 0;
    if (const int kind = zsk_open(b, d_stream, streamSize, h, &zerr, &index)) { zhip_seekable_close(h); return set_err(err, kind, index, zerr); }
    if (const int kind = zsk_typed_probe(b, h, &zerr, &index)) { zhip_seekable_close(h); return set_err(err, kind, index, zerr); }
    if (info) { info->streamSize = streamSize; info->contentSize = h->contentSize; info->nFrames = h->lay.n; info->maxFrameContent = h->maxFrameContent; info->checksumFlag = h->lay.checksum; }
    *out = h;
    return 0;
}

extern "C" int zhip_seekable_decompress_device(zhip_ctx* c, zhip_seekable* h, uint64_t offset, uint64_t length, void* d_dst, int32_t* d_status, void* streamv)
{
    ZskHipBackend b(c, h, streamv);
    return zsk_range(b, c != nullptr, h, offset, length, d_dst, d_status);
}

extern "C" void zhip_seekable_set_scratch_limit(zhip_seekable* h, uint64_t bytes) { if (h) h->scratchLimit = bytes; }

extern "C" int zhip_seekable_decompress_ranges_device(zhip_ctx* c, zhip_seekable* h, const zhip_seekable_range* ranges, size_t nRanges, void* d_dst, uint64_t dstCapacity,
                                                      int32_t* d_status, zhip_seekable_gather_stats* stats, void* streamv)
{
    static_assert(sizeof(zhip_seekable_range) == 24, "the plan reads the ranges as [R][3]");
    ZskHipBackend b(c, h, streamv);
    size_t bad = 0;
    return zsk_ranges(b, c != nullptr, h, (const uint64_t*)ranges, nRanges, d_dst, dstCapacity, d_status, stats, &bad);
}

extern "C" int zhip_seekable_frame_offsets(const zhip_seekable* h, uint32_t first, uint32_t count, uint64_t* out)
{
    if (!h || !out) { g_lastError = "seekable frame offsets: bad arguments"; return ZHIP_ERR_UNSUPPORTED; }
    if (!zsk_frame_offsets(h->dOff.data(), h->lay.n, first, count, out)) {
        char buf[160]; snprintf(buf, sizeof buf, "seekable frame offsets: frames %u + %u, the table has %u", first, count, h->lay.n);
        g_lastError = buf;
        return ZHIP_ERR_SIZE_MISMATCH;
    }
    return 0;
}

// whole frames by index: every index becomes the range of its frame's content, and the many-ranges call does the rest
extern "C" int zhip_seekable_decompress_frames_device(zhip_ctx* c, zhip_seekable* h, const uint32_t* frames, size_t nFrames, const uint64_t* dstOffsets, void* d_dst, uint64_t dstCapacity,
                                                      int32_t* d_status, zhip_seekable_gather_stats* stats, void* streamv)
{
    if (!c || !h || !d_status || (nFrames && !frames) || nFrames > ZSK_MAX_RANGES) { g_lastError = "seekable frames: bad arguments (NULL, or more than 2^27 indices)"; return ZHIP_ERR_UNSUPPORTED; }
    std::vector<zhip_seekable_range> rg(nFrames ? nFrames : 1);
    const size_t bad = zsk_frames_to_ranges(h->dOff.data(), h->lay.n, frames, nFrames, dstOffsets, (uint64_t*)rg.data());
    if (bad != nFrames) {
        char buf[160]; snprintf(buf, sizeof buf, "seekable frames: position %zu names frame %u, the table has %u", bad, frames[bad], h->lay.n);
        g_lastError = buf;
        return ZHIP_ERR_SIZE_MISMATCH;
    }
    return zhip_seekable_decompress_ranges_device(c, h, rg.data(), nFrames, d_dst, dstCapacity, d_status, stats, streamv);
}

// ------------------------------------------------------------------------------------------ seekable streams: edit
extern "C" uint64_t zhip_seekable_edit_bound(const zhip_seekable* old, const zhip_seekable_pick* picks, size_t nPicks, uint64_t maxRecordBytes, int flags)
{
    static_assert(sizeof(zhip_seekable_pick) == sizeof(ZskEditPick) && ZHIP_PICK_FRAME == ZSK_PICK_FRAME && ZHIP_PICK_RECORD == ZSK_PICK_RECORD, "the kernels read the caller's picks as they are");
    if ((flags & ~ZHIP_SEEKABLE_CHECKSUM) || (nPicks && !picks) || nPicks > ZSK_MAX_FRAMES || maxRecordBytes > ZSK_MAX_CONTENT) return 0;
    const int checksum = flags & ZHIP_SEEKABLE_CHECKSUM ? 1 : 0;
    if (old && old->lay.checksum != checksum) return 0;
    size_t bad = 0;
    if (zsk_edit_check((const ZskEditPick*)picks, nPicks, old != nullptr, old ? old->lay.n : 0, ZSK_MAX_FRAMES, &bad)) return 0;
    return zsk_edit_bound((const ZskEditPick*)picks, nPicks, old ? old->cOff.data() : nullptr, maxRecordBytes, checksum);
}

extern "C" int zhip_seekable_edit_device(zhip_ctx* c, zhip_seekable* old, const zhip_seekable_pick* picks, size_t nPicks,
                                         const void* d_src, uint64_t srcSize, const zhip_segment* d_records, size_t nRecords,
                                         uint64_t maxContentBytes, uint64_t maxRecordBytes, int flags,
                                         void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status, void* streamv)
{
    ZskHipBackend b(c, old, streamv);
    return zsk_edit(b, c != nullptr, old, (const ZskEditPick*)picks, nPicks, d_src, srcSize, d_records, nRecords, maxContentBytes, maxRecordBytes, flags, d_dst, dstCapacity, d_streamSize, d_status);
}

// ------------------------------------------------------------------------------------------ seekable streams: typed (zhip_seekable_typed.hpp)
extern "C" int zhip_planes_split_device(zhip_ctx* c, const void* d_src, uint64_t size, uint32_t elementSize, uint32_t frameSize, void* d_dst, void* streamv)
{
    ZskHipTypedBackend b(c, nullptr, streamv);
    return zsk_planes_split(b, c != nullptr, d_src, size, elementSize, frameSize, d_dst);
}
extern "C" int zhip_planes_join_device(zhip_ctx* c, const void* d_src, uint64_t size, uint32_t elementSize, uint32_t frameSize, void* d_dst, void* streamv)
{
    ZskHipTypedBackend b(c, nullptr, streamv);
    return zsk_planes_join(b, c != nullptr, d_src, size, elementSize, frameSize, d_dst);
}
extern "C" int zhip_planes_split_filter_device(zhip_ctx* c, const void* d_src, uint64_t size, uint32_t elementSize, uint32_t frameSize, uint32_t filter, void* d_dst, void* streamv)
{
    ZskHipTypedBackend b(c, nullptr, streamv);
    return zsk_planes_split(b, c != nullptr, d_src, size, elementSize, frameSize, d_dst, filter);
}
extern "C" int zhip_planes_join_filter_device(zhip_ctx* c, const void* d_src, uint64_t size, uint32_t elementSize, uint32_t frameSize, uint32_t filter, void* d_dst, void* streamv)
{
    ZskHipTypedBackend b(c, nullptr, streamv);
    return zsk_planes_join(b, c != nullptr, d_src, size, elementSize, frameSize, d_dst, filter);
}
extern "C" uint64_t zhip_seekable_typed_bound(uint64_t srcSize, uint32_t frameSize, uint32_t elementSize, int flags)
{
    if (flags & ~ZHIP_SEEKABLE_CHECKSUM) return 0;
    if (elementSize == 1) return zsk_bound(srcSize, frameSize, flags & ZHIP_SEEKABLE_CHECKSUM);
    return zsk_typed_bound(srcSize, frameSize, elementSize, flags & ZHIP_SEEKABLE_CHECKSUM);
}
extern "C" int zhip_seekable_compress_typed_device(zhip_ctx* c, const void* d_src, uint64_t srcSize, uint32_t frameSize, uint32_t elementSize, int flags,
                                                   void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status, void* streamv)
{
    ZskHipTypedBackend b(c, nullptr, streamv);
    return zsk_typed_compress(b, c != nullptr, d_src, srcSize, frameSize, elementSize, flags, d_dst, dstCapacity, d_streamSize, d_status);
}
extern "C" int zhip_seekable_compress_typed_filter_device(zhip_ctx* c, const void* d_src, uint64_t srcSize, uint32_t frameSize, uint32_t elementSize, uint32_t filter, int flags,
                                                          void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status, void* streamv)
{
    ZskHipTypedBackend b(c, nullptr, streamv);
    return zsk_typed_compress(b, c != nullptr, d_src, srcSize, frameSize, elementSize, flags, d_dst, dstCapacity, d_streamSize, d_status, filter);
}
// the xor-with-base filter (ZHIP_FILTER_XOR_BASE): the calls that take the base
extern "C" int zhip_planes_split_base_device(zhip_ctx* c, const void* d_src, uint64_t size, uint32_t elementSize, uint32_t frameSize, const void* d_base, void* d_dst, void* streamv)
{
    ZskHipTypedBackend b(c, nullptr, streamv);
    return zsk_planes_split_base(b, c != nullptr, d_src, size, elementSize, frameSize, d_base, d_dst);
}
extern "C" int zhip_planes_join_base_device(zhip_ctx* c, const void* d_planar, uint64_t size, uint32_t elementSize, uint32_t frameSize, const void* d_base, void* d_dst, void* streamv)
{
    ZskHipTypedBackend b(c, nullptr, streamv);
    return zsk_planes_join_base(b, c != nullptr, d_planar, size, elementSize, frameSize, d_base, d_dst);
}
extern "C" int zhip_seekable_compress_typed_base_device(zhip_ctx* c, const void* d_src, uint64_t srcSize, uint32_t frameSize, uint32_t elementSize, const void* d_base, int flags,
                                                        void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status, void* streamv)
{
    ZskHipTypedBackend b(c, nullptr, streamv);
    return zsk_typed_compress_base(b, c != nullptr, d_src, srcSize, frameSize, elementSize, d_base, flags, d_dst, dstCapacity, d_streamSize, d_status);
}
extern "C" int zhip_seekable_decompress_typed_ranges_base_device(zhip_ctx* c, zhip_seekable* h, const void* d_base, uint64_t baseSize, const zhip_seekable_range* ranges, size_t nRanges,
                                                                 void* d_dst, uint64_t dstCapacity, int32_t* d_status, zhip_seekable_gather_stats* stats, void* streamv)
{
    ZskHipTypedBackend b(c, h, streamv);
    size_t bad = 0;
    return zsk_typed_ranges_base(b, c != nullptr, h, d_base, baseSize, (const uint64_t*)ranges, nRanges, d_dst, dstCapacity, d_status, stats, &bad);
}
extern "C" uint32_t zhip_seekable_filter(const zhip_seekable* h) { return h ? h->filter : 0; }
extern "C" uint32_t zhip_seekable_element_size(const zhip_seekable* h) { return h ? h->elementSize : 0; }
extern "C" uint32_t zhip_seekable_group_elements(const zhip_seekable* h) { return h ? h->groupElements : 0; }
extern "C" int zhip_seekable_decompress_typed_ranges_device(zhip_ctx* c, zhip_seekable* h, const zhip_seekable_range* ranges, size_t nRanges, void* d_dst, uint64_t dstCapacity,
                                                            int32_t* d_status, zhip_seekable_gather_stats* stats, void* streamv)
{
    ZskHipTypedBackend b(c, h, streamv);
    size_t bad = 0;
    return zsk_typed_ranges(b, c != nullptr, h, (const uint64_t*)ranges, nRanges, d_dst, dstCapacity, d_status, stats, &bad);
}
// chains of xor-with-base links: the chain join on its own, and the typed read through [full stream or base, delta 1, ..., delta n]
extern "C" int zhip_planes_join_chain_device(zhip_ctx* c, const void* const* d_planar, size_t nLinks, uint64_t size, uint32_t elementSize, uint32_t frameSize, const void* d_base,
                                             void* d_dst, void* streamv)
{
    ZskHipTypedBackend b(c, nullptr, streamv);
    return zsk_planes_join_chain(b, c != nullptr, d_planar, nLinks, size, elementSize, frameSize, d_base, d_dst);
}
extern "C" int zhip_seekable_decompress_typed_ranges_chain_device(zhip_ctx* c, zhip_seekable* const* links, size_t nLinks, const void* d_base, uint64_t baseSize,
                                                                  const zhip_seekable_range* ranges, size_t nRanges, void* d_dst, uint64_t dstCapacity, int32_t* d_status, int32_t* d_link,
                                                                  zhip_seekable_gather_stats* stats, void* streamv)
{
    // a backend per link, over that link's handle: its many-ranges call, its planar and status areas (the sequence checks the chain before it touches one)
    std::vector<ZskHipTypedBackend> backends;
    std::vector<ZskHipTypedBackend*> bs;
    std::vector<const ZskTypedOpened*> hs;
    if (links && nLinks <= ZSK_CHAIN_MAX) {
        backends.reserve(nLinks);
        for (size_t i = 0; i < nLinks; i++) { backends.emplace_back(c, links[i], streamv); hs.push_back(links[i]); }
        for (size_t i = 0; i < nLinks; i++) bs.push_back(&backends[i]);
    }
    size_t bad = 0;
    return zsk_typed_ranges_chain(bs.data(), g_lastError, c != nullptr, links ? hs.data() : nullptr, nLinks, d_base, baseSize, (const uint64_t*)ranges, nRanges, d_dst, dstCapacity, d_status,
                                  d_link, stats, &bad);
}
