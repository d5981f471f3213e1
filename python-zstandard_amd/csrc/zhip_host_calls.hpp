// zhip_host_calls.hpp -- HOST side, free of HIP: the plan of the host-buffer batch calls (zhip_compress_batch / zhip_decompress_batch: multi_compress_to_buffer and
// multi_decompress_to_buffer). What a call refuses before it touches the device, where every item lies in the device arenas, how the batch is cut into chunks, upload steps and
// packing runs, where every array lies in the meta areas, what the sizes and statuses that come back mean, and how a batch is cut over the node's devices is decided HERE, by
// pure functions of plain data. zhip_lib.hip keeps the streams, the events and the copies -- one implementation, it needs no second -- and reads these functions; the CPU tests
// (tests/emu/emu_host_calls.cpp, tests/emu/host_calls_main.cpp) read the same ones.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>
#include "../../include/zstd_hip.h"
#include "zhip_format.hpp"

// ------------------------------------------------------------------------------------------ frame inspection
static inline uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
static inline uint32_t rd24(const uint8_t* p) { return rd16(p) | ((uint32_t)p[2] << 16); }
static inline uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
static inline uint64_t rd64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }

struct HostFrameHeader { uint64_t contentSize; uint32_t headerSize; uint32_t hasChecksum; uint32_t skippable, skipSize; };
// RFC 8878 3.1.1.1; restates ZSTD_getFrameHeader_advanced (zstd.c:43668) for the fields the dispatcher needs.
static inline int host_frame_header(HostFrameHeader* h, const uint8_t* src, size_t n, int format)
{
    const size_t mg = format == ZHIP_FORMAT_ZSTD1_MAGICLESS ? 0 : 4;
    h->skippable = 0; h->skipSize = 0;
    if (n < mg + 1) {
        // too short to say -- unless the bytes that are there already begin neither magic (ZSTD_getFrameHeader_advanced's look at a partial magic, zstd.c:43689)
        uint32_t m = ZF_MAGIC, s = ZF_MAGIC_SKIPPABLE;
        if (mg && n) { memcpy(&m, src, n < 4 ? n : 4); memcpy(&s, src, n < 4 ? n : 4); }
        return m != ZF_MAGIC && (s & 0xFFFFFFF0u) != ZF_MAGIC_SKIPPABLE ? -ZE_PREFIX_UNKNOWN : -ZE_SRC_SIZE_WRONG;
    }
    if (mg && (rd32(src) & 0xFFFFFFF0u) == ZF_MAGIC_SKIPPABLE) {          // skippable frame: content size 0 (ZSTD_getFrameContentSize, zstd.c:43773)
        if (n < 8) return -ZE_SRC_SIZE_WRONG;
        h->skippable = 1; h->skipSize = rd32(src + 4); h->contentSize = 0; h->headerSize = 8; h->hasChecksum = 0;
        return 0;
    }
    if (mg && rd32(src) != ZF_MAGIC) return -ZE_PREFIX_UNKNOWN;
    src += mg; n -= mg;
    uint32_t fhd = src[0], dictCode = fhd & 3, single = (fhd >> 5) & 1, fcsCode = fhd >> 6;
    uint32_t dictBytes = dictCode == 3 ? 4 : dictCode, fcsBytes = fcsCode == 0 ? single : (1u << fcsCode);
    uint32_t hs = 1 + (single ? 0 : 1) + dictBytes + fcsBytes;
    if (fhd & 8) return -ZE_FRAMEPARAM_UNSUPPORTED;
    if (n < hs) return -ZE_SRC_SIZE_WRONG;
    const uint8_t* p = src + 1 + (single ? 0 : 1) + dictBytes;
    h->contentSize = ZHIP_CONTENTSIZE_UNKNOWN;
    if (fcsCode == 0) { if (single) h->contentSize = p[0]; }
    else if (fcsCode == 1) h->contentSize = (uint64_t)rd16(p) + 256;
    else if (fcsCode == 2) h->contentSize = rd32(p);
    else h->contentSize = rd64(p);
    h->headerSize = (uint32_t)mg + hs; h->hasChecksum = (fhd >> 2) & 1;
    return 0;
}
static inline uint64_t host_frame_content_size(const uint8_t* src, size_t n, int format)
{
    HostFrameHeader h;
    return host_frame_header(&h, src, n, format) < 0 ? ZHIP_CONTENTSIZE_ERROR : h.contentSize;
}
// the block headers of a frame from `pos` (behind the frame header) to its last block: how many blocks it passed, where it stood when it stopped, and why it stopped
enum HostWalkStop { HOST_WALK_LAST = 0, HOST_WALK_TRUNCATED, HOST_WALK_RESERVED };      // behind the last block; a header or a body beyond the input; a block of the reserved type 3
struct HostBlockWalk { uint64_t nBlocks; size_t end; int stop; };
static inline HostBlockWalk host_walk_blocks(const uint8_t* src, size_t n, size_t pos)
{
    uint64_t nb = 0;
    for (;;) {
        if (pos + 3 > n) return {nb, pos, HOST_WALK_TRUNCATED};
        const uint32_t bh = rd24(src + pos), type = (bh >> 1) & 3, bs = bh >> 3;
        if (type == 3) return {nb, pos, HOST_WALK_RESERVED};
        const size_t body = type == 1 ? 1 : bs;
        if (pos + 3 + body > n) return {nb, pos, HOST_WALK_TRUNCATED};
        pos += 3 + body; nb++;
        if (bh & 1) return {nb, pos, HOST_WALK_LAST};
    }
}
// how many blocks a frame has (0: not a frame this walk can follow -- the kernels will say what is wrong with it). The host-buffer decompress call uses it to tell frames of
// SEVERAL blocks from frames of one: libzstd's block splitter (levels 16 and up) cuts even a 128 KiB source into many, and those belong to the pipeline's several-block mode,
// not -- one wave each -- to the generic kernel (round 6: 2 048 level-19 frames of 128 KiB took 44 ms there, 6 GB/s). A frame whose first 65 536 blocks are not its last: 0
static inline uint32_t host_count_blocks(const uint8_t* src, size_t n, int format)
{
    HostFrameHeader h;
    if (host_frame_header(&h, src, n, format) < 0 || h.skippable) return 0;
    const HostBlockWalk w = host_walk_blocks(src, n, h.headerSize);
    return w.stop == HOST_WALK_LAST && w.nBlocks <= 65536 ? (uint32_t)w.nBlocks : 0;
}
// ZSTD_findFrameCompressedSize: the bytes of the first frame of src, or minus a zstd error code
static inline int64_t host_frame_compressed_size(const uint8_t* src, size_t n, int format)
{
    HostFrameHeader h; int e = host_frame_header(&h, src, n, format); if (e < 0) return e;
    if (h.skippable) return (uint64_t)h.skipSize + 8 > n ? -ZE_SRC_SIZE_WRONG : (int64_t)h.skipSize + 8;      // readSkippableFrameSize (zstd.c:43795)
    const HostBlockWalk w = host_walk_blocks(src, n, h.headerSize);
    if (w.stop != HOST_WALK_LAST) return w.stop == HOST_WALK_RESERVED ? -ZE_CORRUPTION : -ZE_SRC_SIZE_WRONG;
    if (h.hasChecksum && w.end + 4 > n) return -ZE_SRC_SIZE_WRONG;
    return (int64_t)(w.end + (h.hasChecksum ? 4 : 0));
}

// ------------------------------------------------------------------------------------------ pass 1: the two segment layouts
static inline size_t host_compress_bound(size_t n) { return n + (n >> 8) + (n < (128u << 10) ? (((128u << 10) - n) >> 11) : 0); }

// why a call refuses its items before it touches the device: kind 0 = it does not. text (compress): what zhip_last_error() then says
struct HostRefusal { int kind = ZHIP_ERR_NONE; size_t index = 0; const char* text = nullptr; };
#define ZHIP_HOST_TOTAL_MAX ((uint64_t)1 << 46)
// decompress (decompress_worker pass 1, decompressor.c:981-1014): every frame needs a known decompressed size. segs: [0,n) source, [n,2n) destination, both back to back;
// nBlocks: blocks per frame (0: unknown), from the block headers
static inline HostRefusal host_decompress_segments(const zhip_item* items, size_t n, int format, zhip_segment* segs, uint32_t* nBlocks, uint64_t* srcTotal, uint64_t* dstTotal)
{
    uint64_t st = 0, dt = 0;
    for (size_t i = 0; i < n; i++) {
        uint64_t ds = items[i].dstSize;
        if (ds == 0) {
            const uint64_t fcs = host_frame_content_size((const uint8_t*)items[i].src, items[i].srcSize, format);
            if (fcs == ZHIP_CONTENTSIZE_ERROR || fcs == ZHIP_CONTENTSIZE_UNKNOWN) return {ZHIP_ERR_UNKNOWN_SIZE, i, nullptr};
            ds = fcs;
        }
        // the sizes come from untrusted frame headers: a claimed size that cannot be allocated is "out of memory" (what the reference's
        // malloc of the destination reports, decompressor.c:1085-1090), never a wrapped sum
        if (ds > ZHIP_HOST_TOTAL_MAX || dt + ds > ZHIP_HOST_TOTAL_MAX) return {ZHIP_ERR_NO_MEMORY, i, nullptr};
        segs[i].offset = st; segs[i].length = items[i].srcSize; st += items[i].srcSize;
        segs[n + i].offset = dt; segs[n + i].length = ds; dt += ds;
        nBlocks[i] = host_count_blocks((const uint8_t*)items[i].src, items[i].srcSize, format);
    }
    *srcTotal = st; *dstTotal = dt;
    return {};
}
// compress: like compress_worker (compressor.c:913-947) every item gets a ZSTD_compressBound-sized slot (rounded up to 16); the frames are compacted on the
// device, chunk by chunk, and only they travel back
static inline HostRefusal host_compress_segments(const zhip_item* items, size_t n, zhip_segment* segs, uint64_t* srcTotal, uint64_t* dstTotal)
{
    uint64_t st = 0, dt = 0;
    for (size_t i = 0; i < n; i++) {
        if (items[i].srcSize >= (1ull << 31)) return {ZHIP_ERR_UNSUPPORTED, i, "inputs of 2 GiB and more are not implemented in the HIP backend"};
        segs[i].offset = st; segs[i].length = items[i].srcSize; st += items[i].srcSize;
        const uint64_t b = ((uint64_t)host_compress_bound(items[i].srcSize) + 15) & ~(uint64_t)15;
        segs[n + i].offset = dt; segs[n + i].length = b; dt += b;
    }
    *srcTotal = st; *dstTotal = dt;
    return {};
}

// ------------------------------------------------------------------------------------------ cuts and splits
// chunk boundaries [cut[k], cut[k+1]) over n items: a chunk closes when its input or output bytes reach maxBytes or it holds maxItems
// items. segs: [0,n) source, [n,2n) destination.
// firstItems (0: like the others): a smaller first chunk shortens the pipeline's fill -- the time before the first kernel can start
static inline std::vector<size_t> host_chunks(const zhip_segment* segs, size_t n, uint64_t maxBytes, size_t maxItems, size_t firstItems = 0)
{
    std::vector<size_t> cut(1, 0);
    uint64_t in = 0, out = 0; size_t cnt = 0;
    for (size_t i = 0; i < n; i++) {
        in += segs[i].length; out += segs[n + i].length; cnt++;
        const size_t lim = cut.size() == 1 && firstItems ? firstItems : maxItems;
        if (in >= maxBytes || out >= maxBytes || cnt >= lim) { cut.push_back(i + 1); in = out = 0; cnt = 0; }
    }
    if (cut.back() != n) cut.push_back(n);
    return cut;
}
// the upload step that begins at item a < hi: items [a, b) and their bytes -- as many as fit stageBytes, and one item however large it is
struct HostStep { size_t a, b; uint64_t bytes; };
static inline HostStep host_upload_step(const zhip_segment* segs, size_t a, size_t hi, uint64_t stageBytes)
{
    size_t b = a; uint64_t bytes = 0;
    while (b < hi && (b == a || bytes + segs[b].length <= stageBytes)) { bytes += segs[b].length; b++; }
    return {a, b, bytes};
}
// the runs [cut[t], cut[t+1]) in which `threads` host threads pack the items [lo, hi) of one step: by bytes, and one run below `threshold` bytes or 2 items a thread
static inline std::vector<size_t> host_pack_split(const zhip_segment* segs, size_t lo, size_t hi, uint64_t threshold, unsigned threads)
{
    std::vector<size_t> cut(1, lo);
    if (hi <= lo) return cut;
    const uint64_t base = segs[lo].offset, bytes = segs[hi - 1].offset + segs[hi - 1].length - base;
    const unsigned nt = bytes >= threshold ? threads : 1;
    if (nt <= 1 || hi - lo < 2 * (size_t)nt) { cut.push_back(hi); return cut; }
    size_t a = lo;
    for (unsigned t = 0; t < nt && a < hi; t++) {
        const uint64_t target = base + bytes * (t + 1) / nt;
        size_t b = a;
        while (b < hi && (t + 1 == nt || segs[b].offset + segs[b].length <= target)) b++;
        if (b == a) b = a + 1;
        cut.push_back(b);
        a = b;
    }
    return cut;
}
// items [lo, hi) -> stage, item i at offset segs[i].offset - segs[lo].offset. Big steps are split over host threads by bytes.
static inline void pack_items(uint8_t* stage, const zhip_item* items, const zhip_segment* segs, size_t lo, size_t hi, uint64_t threshold, unsigned threads)
{
    if (hi <= lo) return;
    const uint64_t base = segs[lo].offset;
    auto run = [&](size_t a, size_t b) { for (size_t i = a; i < b; i++) if (items[i].srcSize) memcpy(stage + (segs[i].offset - base), items[i].src, items[i].srcSize); };
    const std::vector<size_t> cut = host_pack_split(segs, lo, hi, threshold, threads);
    if (cut.size() <= 2) { run(lo, hi); return; }
    std::vector<std::thread> th;
    for (size_t t = 0; t + 1 < cut.size(); t++) th.emplace_back(run, cut[t], cut[t + 1]);
    for (auto& t : th) t.join();
}

// ------------------------------------------------------------------------------------------ meta layouts
// where a call keeps its per-item words: d* in the context's device meta area (dBytes to reserve), h* in its small pinned area (hBytes), byte offsets
struct HostDecompressLayout { size_t dSizes, dStatus, dBytes, hSizes, hStatus, hBytes; };
static inline HostDecompressLayout host_decompress_layout(size_t n)
{
    HostDecompressLayout l;
    l.dSizes = 0; l.dStatus = n * sizeof(uint64_t); l.dBytes = l.dStatus + n * sizeof(int32_t) + 16;
    l.hSizes = l.dSizes; l.hStatus = l.dStatus; l.hBytes = l.dBytes;
    return l;
}
// compress: the device also holds the frames' offsets in the dense payload and both sides the chunks' totals (nChunks + 1 words)
struct HostCompressLayout { size_t dSizes, dOffs, dTotals, dStatus, dBytes, hSizes, hTotals, hStatus, hBytes; };
static inline HostCompressLayout host_compress_layout(size_t n, size_t nChunks)
{
    HostCompressLayout l;
    const size_t totals = (nChunks + 1) * sizeof(uint64_t);
    l.dSizes = 0; l.dOffs = l.dSizes + n * sizeof(uint64_t); l.dTotals = l.dOffs + n * sizeof(uint64_t); l.dStatus = l.dTotals + totals; l.dBytes = l.dStatus + n * sizeof(int32_t) + 32;
    l.hSizes = 0; l.hTotals = l.hSizes + n * sizeof(uint64_t); l.hStatus = l.hTotals + totals; l.hBytes = l.hStatus + n * sizeof(int32_t) + 32;
    return l;
}

// ------------------------------------------------------------------------------------------ verdicts
struct HostVerdict { int kind = ZHIP_ERR_NONE; size_t index = 0; int zerr = 0; uint64_t d0 = 0, d1 = 0; };
// decompress, items [lo, hi) of one chunk: out[i - lo] = where item i lies in the chunk's payload and what it produced. The first failing item is reported: its status, else
// its size -- what it produced against dstSegs[i].length (detail: produced, expected); allowShort: the length is a capacity, less is fine. dstSegs = segs + n
static inline HostVerdict host_decompress_verdict(const zhip_segment* dstSegs, const uint64_t* sizes, const int32_t* status, size_t lo, size_t hi, bool allowShort, zhip_segment* out)
{
    const uint64_t base = hi > lo ? dstSegs[lo].offset : 0;
    for (size_t i = lo; i < hi; i++) {
        if (status[i]) return {ZHIP_ERR_ZSTD, i, status[i], 0, 0};
        if (sizes[i] != dstSegs[i].length && !(allowShort && sizes[i] < dstSegs[i].length)) return {ZHIP_ERR_SIZE_MISMATCH, i, 0, sizes[i], dstSegs[i].length};
        out[i - lo].offset = dstSegs[i].offset - base; out[i - lo].length = sizes[i];
    }
    return {};
}
// compress, items [lo, hi) of one chunk: the first item with a status, before anything is allocated for the chunk
static inline HostVerdict host_compress_verdict(const int32_t* status, size_t lo, size_t hi)
{
    for (size_t i = lo; i < hi; i++) if (status[i]) return {ZHIP_ERR_ZSTD, i, status[i], 0, 0};
    return {};
}
// .. and the frames back to back in the chunk's dense payload; returns their bytes
static inline uint64_t host_compress_out_segments(const uint64_t* sizes, size_t lo, size_t hi, zhip_segment* out)
{
    uint64_t o = 0;
    for (size_t i = lo; i < hi; i++) { out[i - lo].offset = o; out[i - lo].length = sizes[i]; o += sizes[i]; }
    return o;
}

// ------------------------------------------------------------------------------------------ what a context gives back after a call
// a context keeps its device buffers between calls as long as they total at most `keep` bytes. Above that: release the largest trimmable buffer whose capacity is above 64 MiB
// (of equals the earlier one), again and again, until the total fits or no such buffer is left. caps: every buffer of the context (all of them count towards the total),
// trimmable: which of them may go. Returns the indices to release, in order
static inline std::vector<size_t> host_trim_order(const size_t* caps, const bool* trimmable, size_t n, size_t keep)
{
    std::vector<size_t> cap(caps, caps + n), order;
    size_t total = 0;
    for (size_t i = 0; i < n; i++) total += cap[i];
    while (total > keep) {
        size_t big = n;
        for (size_t i = 0; i < n; i++) if (trimmable[i] && cap[i] > ((size_t)64 << 20) && (big == n || cap[i] > cap[big])) big = i;
        if (big == n) break;
        order.push_back(big); total -= cap[big]; cap[big] = 0;
    }
    return order;
}

// ------------------------------------------------------------------------------------------ one call, every device: the decisions of the fan-out
// compressor.c:1127-1216: never more workers than items (:1151); walk the items, close a worker's run once its bytes reach total / workers; the
// last worker takes the rest. bounds[2w], bounds[2w+1] = [start, end) of worker w; returns the workers that got a run.
static inline size_t host_partition_by_bytes(const uint64_t* sizes, size_t n, size_t workers, size_t* bounds)
{
    if (workers < 1) workers = 1;
    if (n && workers > n) workers = n;
    if (!n) return 0;
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) total += sizes[i];
    const uint64_t per = total / workers;
    size_t w = 0, start = 0; uint64_t acc = 0;
    for (size_t i = 0; i < n; i++) {
        acc += sizes[i];
        if (w == workers - 1) continue;
        if (acc >= per) { bounds[2 * w] = start; bounds[2 * w + 1] = i + 1; w++; start = i + 1; acc = 0; }
    }
    if (start < n) { bounds[2 * w] = start; bounds[2 * w + 1] = n; w++; }
    return w;
}
// ZHIP_DEVICES: device ordinals separated by commas, each a slot (a device may be listed twice); ordinals outside [0, count) are dropped, the list ends at what is no number
static inline std::vector<int> host_parse_devices(const char* list, int count)
{
    std::vector<int> slots;
    for (const char* p = list; *p;) {
        char* end = nullptr;
        const long v = strtol(p, &end, 10);
        if (end == p) break;
        if (v >= 0 && v < count) slots.push_back((int)v);
        p = *end == ',' ? end + 1 : end;
    }
    return slots;
}
// device slots a batch of `n` items / `bytes` input bytes is cut over (0: the calling thread's current device, inline). Without an explicit list never more
// slots than minBytes of input each
static inline size_t host_slots_for(size_t slots, bool explicitList, uint64_t minBytes, size_t n, uint64_t bytes)
{
    size_t d = slots;
    if (!explicitList) {
        if (d <= 1) return 0;
        const uint64_t byBytes = minBytes ? bytes / minBytes : d;
        if (byBytes < d) d = (size_t)byBytes;
        if (d <= 1) return 0;
    }
    if (d > n) d = n;
    return d;
}
// the merge at the end of a fan-out. A run is the items [lo, ..) one device took and what its call returned
struct HostRun { size_t lo = 0; int rc = 0; zhip_error err; zhip_outbuf* out = nullptr; size_t nOut = 0; };
// the first failing item (the lowest index: runs are in item order), as the reference reports it (compressor.c:1225-1253): the lowest failing run, or `used`;
// *err is that run's, its index counted from the call's first item
static inline size_t host_merge_failing(const HostRun* runs, size_t used, zhip_error* err)
{
    for (size_t w = 0; w < used; w++) if (runs[w].rc) {
        if (err) { *err = runs[w].err; err->index += runs[w].lo; }
        return w;
    }
    return used;
}
// the runs' buffers concatenated in run order (which is item order); the runs' own arrays are freed. nullptr: no memory, nothing freed
static inline zhip_outbuf* host_merge_concat(HostRun* runs, size_t used, size_t* total)
{
    size_t t = 0;
    for (size_t w = 0; w < used; w++) t += runs[w].nOut;
    zhip_outbuf* all = (zhip_outbuf*)calloc(t ? t : 1, sizeof(zhip_outbuf));
    if (!all) return nullptr;
    size_t k = 0;
    for (size_t w = 0; w < used; w++) { for (size_t j = 0; j < runs[w].nOut; j++) all[k++] = runs[w].out[j]; free(runs[w].out); runs[w].out = nullptr; }
    *total = t;
    return all;
}
