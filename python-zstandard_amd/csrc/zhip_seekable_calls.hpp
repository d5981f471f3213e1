// zhip_seekable_calls.hpp -- HOST side, free of HIP: everything the seekable calls decide before and between their kernels, once. Per call: the layout of its
// meta area, the host checks with their ZHIP_ERR_* code and message, the grids, and the sequence of reservations, launches, batch calls and copies as a function
// template over a backend B. zhip_lib.hip runs the templates over the HIP runtime (ZskHipBackend); the emulator harness (tests/emu/emu_seekable_backend.hpp)
// runs the same templates over heap areas and zhemu::run_grid, so the CPU tests and their sanitizer programs exercise these layouts, this wiring and this order.
//
// The backend is a plain struct passed by reference:
//     int numCU;  std::string& err;                                                      what the grids scale with; where a refusal's text goes
//     int  reserve(ZskArea, size_t bytes, uint8_t** base)                                0 or the ZHIP_ERR_* code (growing an area frees the old one, which waits for the
//                                                                                        device: the one wait the stream-order rules allow besides the open call's)
//     void launch(ZskKernel, uint32_t grid, const void* args)                            one-wave workgroups; args is the kernel's Zsk*Args
//     int  check()                                                                       the launches so far were accepted (hipGetLastError)
//     int  compress(src, srcSegs, n, slots, slotSegs, outSizes, status, srcMax)          zhip_compress_batch_device under the size hint srcMax
//     int  decompress(opened, srcSegs, n, dstBase, dstSegs, outSizes, status)            the decode batch under the stream's hints
//     void compact(grid, slots, slotSegs, sizes, status, offs, n, dst)                   zhip_compact_kernel
//     int  zero(p, bytes)   int copy(dst, src, bytes, ZskCopy)   int wait()              on the caller's stream; only the open call copies to the host and waits
#pragma once
#include "zhip_seekable.hpp"
#include "../../include/zstd_hip.h"
#include <stdio.h>
#include <string>

// the 18 kernels as X(id, name, args): zhip_seekable_<name>_kernel(args) runs zsk_<name>_body. The enum, the library's launch switch and the emulator's lane
// table are all written from this one list
#define ZSK_KERNELS(X) \
    X(SCAN_REDUCE, scan_reduce, ZskScanArgs) X(SCAN_WRITE, scan_write, ZskScanArgs) X(CHUNK_SEGS, chunk_segs, ZskCompressArgs) X(VERDICT, verdict, ZskCompressArgs) \
    X(TABLE, table, ZskCompressArgs) X(RECORDS_VERDICT, records_verdict, ZskRecordsArgs) X(RECORDS_SEGS, records_segs, ZskRecordsArgs) X(RECORDS_TABLE, records_table, ZskRecordsArgs) \
    X(RANGE_SEGS, range_segs, ZskRangeArgs) X(RANGE_VERIFY, range_verify, ZskRangeArgs) X(RANGE_FINISH, range_finish, ZskRangeArgs) X(GATHER_SEGS, gather_segs, ZskGatherArgs) \
    X(GATHER_VERIFY, gather_verify, ZskGatherArgs) X(GATHER_FINISH, gather_finish, ZskGatherArgs) X(EDIT_SIZES, edit_sizes, ZskEditArgs) X(EDIT_VERDICT, edit_verdict, ZskEditArgs) \
    X(EDIT_COPY, edit_copy, ZskEditArgs) X(EDIT_TABLE, edit_table, ZskEditArgs)
#define ZSK_X(id, name, args) ZSK_K_##id,
enum ZskKernel { ZSK_KERNELS(ZSK_X) ZSK_K_COUNT };
#undef ZSK_X
// the context's meta area and slots; the handle's scan columns, range areas, many-ranges areas (the scratch is allocated at exactly its bytes); a pinned slot
// no upload still reads (the handle's where there is one, else the context's)
enum ZskArea { ZSK_A_SK_META, ZSK_A_SK_SLOTS, ZSK_A_PREFIX, ZSK_A_META, ZSK_A_EDGE, ZSK_A_G_TABLES, ZSK_A_G_META, ZSK_A_G_SCRATCH, ZSK_A_PIN, ZSK_A_COUNT };
enum ZskCopy { ZSK_COPY_TO_HOST, ZSK_COPY_FROM_PIN, ZSK_COPY_ON_DEVICE };      // FROM_PIN: the upload from the slot last reserved, and the event behind it

// what the open call leaves for the readers and the edit call: the stream, its table's shape, the scans' columns on the device (pre) and their host copies
struct ZskOpened {
    const uint8_t* stream = nullptr; uint64_t streamSize = 0;
    ZskLayout lay = {0, 8, 0, 0};
    uint64_t contentSize = 0; uint32_t maxFrameContent = 0;
    const uint8_t* pre = nullptr;        // compressed offsets, decompressed offsets, place among the frames with content -- [n + 1] each, zsk_open_layout(n).col apart
    std::vector<uint64_t> dOff, place;   // the host's copies: which frames cover a range, and how many of them go to the decoder
    std::vector<uint64_t> cOff;          // and where a frame's bytes lie: what an edit keeps of the stream (zhip_seekable_edit_bound)
    uint64_t scratchLimit = 0;           // 0 = ZSK_SCRATCH_DEFAULT
};

// ------------------------------------------------------------------------------------------------ grids
static inline uint32_t zsk_lane_grid(int numCU, uint64_t lanes)
{
    const uint64_t w = (lanes + 63) / 64, gm = (uint64_t)(numCU > 0 ? numCU : 1) * 8;
    return (uint32_t)(w < 1 ? 1 : w < gm ? w : gm);
}
static inline uint32_t zsk_compact_grid(int numCU, size_t n) { const size_t gmax = (size_t)numCU * 16; return (uint32_t)(n < gmax ? n : gmax); }
// the edit copy's grid is fixed (the host knows only bounds): the tiles of dstCapacity bytes and one more per pick cover every stream that fits
static inline uint32_t zsk_edit_copy_grid(int numCU, uint64_t dstCapacity, size_t nPicks)
{
    const uint64_t tilesMost = dstCapacity / ZSK_COPY_TILE + nPicks + 1, gmax = (uint64_t)(numCU > 0 ? numCU : 1) * 32;
    return (uint32_t)(tilesMost < gmax ? tilesMost : gmax);
}

// ------------------------------------------------------------------------------------------------ the meta layouts
static inline size_t zsk_up16(size_t v) { return (v + 15) & ~(size_t)15; }

struct ZskCompressLayout { size_t oSrcSegs, oSlotSegs, oSizes, oOffs, oPartSum, oPartBad, oGo, oStatus, metaBytes; };
static inline ZskCompressLayout zsk_compress_layout(size_t n)
{
    ZskCompressLayout l;
    l.oSrcSegs = 0; l.oSlotSegs = l.oSrcSegs + zsk_up16(n * 16); l.oSizes = l.oSlotSegs + zsk_up16(n * 16); l.oOffs = l.oSizes + zsk_up16(n * 8);
    l.oPartSum = l.oOffs + zsk_up16((n + 1) * 8); l.oPartBad = l.oPartSum + ZSK_SCAN_GRID * 8; l.oGo = l.oPartBad + ZSK_SCAN_GRID * 8; l.oStatus = l.oGo + 16;
    l.metaBytes = l.oStatus + zsk_up16(n * 4);
    return l;
}
// where the records call keeps its arrays in the context's meta area; a caller with arrays of its own (the edit call) puts them behind metaBytes
struct ZskRecordsLayout { size_t oSrcSegs, oSlotSegs, oSizes, oOffs, oLenOffs, oSlotOffs, oPartSum, oPartBad, oPreBad, oGo, oStatus, metaBytes; };
static inline ZskRecordsLayout zsk_records_layout(size_t n)
{
    ZskRecordsLayout l;
    l.oSrcSegs = 0; l.oSlotSegs = l.oSrcSegs + zsk_up16(n * 16); l.oSizes = l.oSlotSegs + zsk_up16(n * 16); l.oOffs = l.oSizes + zsk_up16(n * 8);
    l.oLenOffs = l.oOffs + zsk_up16((n + 1) * 8); l.oSlotOffs = l.oLenOffs + zsk_up16((n + 1) * 8); l.oPartSum = l.oSlotOffs + zsk_up16((n + 1) * 8);
    l.oPartBad = l.oPartSum + ZSK_SCAN_GRID * 8; l.oPreBad = l.oPartBad + ZSK_SCAN_GRID * 8; l.oGo = l.oPreBad + ZSK_SCAN_GRID * 8; l.oStatus = l.oGo + 16;
    l.metaBytes = zsk_up16(l.oStatus + zsk_up16(n * 4));
    return l;
}
// the open call: three columns of [n + 1] in the prefix area, a (sums, lowest bad) pair of ZSK_SCAN_GRID cells per scan in the meta area
struct ZskOpenLayout { size_t col, part, prefixBytes, metaBytes; };
static inline ZskOpenLayout zsk_open_layout(size_t n)
{
    ZskOpenLayout l;
    l.col = zsk_up16((n + 1) * 8); l.part = ZSK_SCAN_GRID * 8; l.prefixBytes = 3 * l.col; l.metaBytes = 6 * l.part;
    return l;
}
// a decode batch's item arrays and the readers' `worst` words (worstBytes): 16 bytes for the single range, a word per range for many
struct ZskItemsLayout { size_t oSrcSegs, oDstSegs, oSizes, oFrameOf, oStatus, oWorst, metaBytes; };
static inline ZskItemsLayout zsk_items_layout(size_t count, size_t worstBytes)
{
    ZskItemsLayout l;
    l.oSrcSegs = 0; l.oDstSegs = l.oSrcSegs + zsk_up16(count * 16); l.oSizes = l.oDstSegs + zsk_up16(count * 16); l.oFrameOf = l.oSizes + zsk_up16(count * 8);
    l.oStatus = l.oFrameOf + zsk_up16(count * 4); l.oWorst = l.oStatus + zsk_up16(count * 4); l.metaBytes = l.oWorst + worstBytes;
    return l;
}
// many ranges: the plan's tables (ranges, segments, jobs: 32 bytes an entry each) as they are uploaded, and the items
struct ZskGatherLayout { size_t oRanges, oSegs, oJobs, tableBytes; ZskItemsLayout m; };
static inline ZskGatherLayout zsk_gather_layout(size_t R, size_t S, size_t J, size_t count)
{
    ZskGatherLayout l;
    l.oRanges = 0; l.oSegs = l.oRanges + R * sizeof(ZskGatherRange); l.oJobs = l.oSegs + S * sizeof(ZskGatherSeg); l.tableBytes = l.oJobs + J * sizeof(ZskGatherJob);
    l.m = zsk_items_layout(count, zsk_up16(R * 4));
    return l;
}
// the edit call's per-pick arrays: behind the records layout where there are records, else from 0; in place the old table's entries are stashed at the end
struct ZskEditLayout { size_t oPicks, oPickSize, oOffs, oTileOffs, oPartSum, oPartBad, oTileBad, oGo, oPickStatus, oStash, end; };
static inline ZskEditLayout zsk_edit_layout(size_t n, size_t nRecords, size_t nOld, bool inPlace, size_t entry)
{
    ZskEditLayout l;
    l.oPicks = nRecords ? zsk_records_layout(nRecords).metaBytes : 0; l.oPickSize = l.oPicks + zsk_up16(n * 8); l.oOffs = l.oPickSize + zsk_up16(n * 8);
    l.oTileOffs = l.oOffs + zsk_up16((n + 1) * 8); l.oPartSum = l.oTileOffs + zsk_up16((n + 1) * 8); l.oPartBad = l.oPartSum + ZSK_SCAN_GRID * 8;
    l.oTileBad = l.oPartBad + ZSK_SCAN_GRID * 8; l.oGo = l.oTileBad + ZSK_SCAN_GRID * 8; l.oPickStatus = l.oGo + 16; l.oStash = l.oPickStatus + zsk_up16(n * 4);
    l.end = l.oStash + (inPlace ? zsk_up16(nOld * entry) : 0);
    return l;
}

// ------------------------------------------------------------------------------------------------ the host checks: the code, and the text zhip_last_error returns
static inline int zsk_refuse(std::string& err, int code, const char* text) { err = text; return code; }

static inline int zsk_compress_check(bool pointers, uint64_t srcSize, uint32_t frameSize, int flags, std::string& err)
{
    if (!pointers || (flags & ~ZHIP_SEEKABLE_CHECKSUM)) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "seekable compress: bad arguments");
    if (!zsk_args_ok(srcSize, frameSize)) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "seekable compress: frameSize must be 1 ... 2^30 and the frame count at most 2^27");
    return 0;
}
static inline int zsk_records_check(bool pointers, const void* d_records, size_t nRecords, uint64_t maxRecordBytes, int flags, std::string& err)
{
    if (!pointers || (nRecords && !d_records) || (flags & ~ZHIP_SEEKABLE_CHECKSUM)) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "seekable compress: bad arguments");
    if (nRecords > ZSK_MAX_FRAMES || maxRecordBytes > ZSK_MAX_CONTENT) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "seekable compress: at most 2^27 records of at most 2^30 bytes");
    return 0;
}
static inline int zsk_range_check(uint64_t offset, uint64_t length, uint64_t contentSize, std::string& err)
{
    const uint64_t end = offset + length;
    if (end < offset || end > contentSize) {
        char buf[160]; snprintf(buf, sizeof buf, "seekable decompress: the range ends at %llu, the content at %llu", (unsigned long long)end, (unsigned long long)contentSize);
        return zsk_refuse(err, ZHIP_ERR_SIZE_MISMATCH, buf);
    }
    return 0;
}
// rg = [R][3] (offset, length, dstOffset). *bad: the range a refusal names; *any: whether a range has bytes
static inline int zsk_ranges_check(bool pointers, const uint64_t* rg, size_t R, uint64_t contentSize, const void* d_dst, uint64_t dstCapacity, size_t* bad, bool* any, std::string& err)
{
    if (!pointers || (R && !rg) || R > ZSK_MAX_RANGES) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "seekable ranges: bad arguments (NULL, or more than 2^27 ranges)");
    size_t other = 0;
    if (const int why = zsk_gather_check(rg, R, contentSize, dstCapacity, bad, &other)) {
        char buf[224];
        const unsigned long long off = rg[3 * *bad], len = rg[3 * *bad + 1], at = rg[3 * *bad + 2];
        if (why == 1) snprintf(buf, sizeof buf, "seekable ranges: range %zu ends at %llu + %llu, the content at %llu", *bad, off, len, (unsigned long long)contentSize);
        else if (why == 2) snprintf(buf, sizeof buf, "seekable ranges: range %zu goes to %llu + %llu, the capacity is %llu", *bad, at, len, (unsigned long long)dstCapacity);
        else snprintf(buf, sizeof buf, "seekable ranges: the destinations of ranges %zu and %zu overlap", other, *bad);
        return zsk_refuse(err, why == 3 ? ZHIP_ERR_UNSUPPORTED : ZHIP_ERR_SIZE_MISMATCH, buf);
    }
    *any = false;
    for (size_t r = 0; r < R; r++) *any = *any || rg[3 * r + 1];
    if (*any && !d_dst) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "seekable ranges: bad arguments (no destination)");
    return 0;
}
// the edit call's refusals, the checksum-flag match and the in-place / overlap decision. *bad: the position a refusal names
static inline int zsk_edit_call_check(bool pointers, const ZskOpened* old, const ZskEditPick* pk, size_t nPicks, const void* d_records, size_t nRecords, uint64_t maxRecordBytes, int flags,
                                      const void* d_dst, uint64_t dstCapacity, bool* inPlace, size_t* bad, std::string& err)
{
    if (!pointers || !d_dst || (nPicks && !pk) || (nRecords && !d_records) || (flags & ~ZHIP_SEEKABLE_CHECKSUM)) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "seekable edit: bad arguments");
    if (nPicks > ZSK_MAX_FRAMES) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "seekable edit: at most 2^27 picks");
    if (nRecords > ZSK_MAX_FRAMES || maxRecordBytes > ZSK_MAX_CONTENT) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "seekable edit: at most 2^27 records of at most 2^30 bytes");
    const uint32_t checksum = flags & ZHIP_SEEKABLE_CHECKSUM ? 1u : 0u;
    if (old && (uint32_t)old->lay.checksum != checksum) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "seekable edit: ZHIP_SEEKABLE_CHECKSUM must be set exactly when the opened stream's table has checksums");
    const uint32_t nOld = old ? old->lay.n : 0;
    *bad = 0;
    size_t at = 0;
    if (const int why = zsk_edit_check(pk, nPicks, old != nullptr, nOld, nRecords, &at)) {
        *bad = at;
        char buf[200];
        if (why == 1) snprintf(buf, sizeof buf, "seekable edit: position %zu is %s", *bad, pk[*bad].from > ZSK_PICK_RECORD ? "neither a frame nor a record pick" : "a frame pick, and no stream is opened");
        else snprintf(buf, sizeof buf, "seekable edit: position %zu names %s %u, there are %llu", *bad, pk[*bad].from == ZSK_PICK_FRAME ? "frame" : "record", pk[*bad].index,
                      (unsigned long long)(pk[*bad].from == ZSK_PICK_FRAME ? (uint64_t)nOld : (uint64_t)nRecords));
        return zsk_refuse(err, why == 1 ? ZHIP_ERR_UNSUPPORTED : ZHIP_ERR_SIZE_MISMATCH, buf);
    }
    *inPlace = false;
    if (old) {
        const uint8_t* const d0 = (const uint8_t*)d_dst; const uint8_t* const o0 = old->stream;
        if (d0 < o0 + old->streamSize && o0 < d0 + dstCapacity) {
            *inPlace = d0 == o0 && zsk_edit_is_append(pk, nPicks, nOld);
            if (!*inPlace) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "seekable edit: the destination overlaps the opened stream (allowed only at its base, with picks that begin with every frame in order)");
        }
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ the sequences
template <class B> int zsk_launch_scan(B& b, ZskScanArgs a)
{
    const uint32_t grid = zsk_scan_shape(a.n, &a.span);
    b.launch(ZSK_K_SCAN_REDUCE, grid, &a);
    b.launch(ZSK_K_SCAN_WRITE, grid, &a);
    return b.check();
}

// The tail of a compress call behind the batch: the scan of the sizes, its verdict, the table writer (the fixed cut's or the records'), the compaction
template <class B> int zsk_compress_tail(B& b, const ZskCompressArgs& a, uint64_t* partSum, const uint8_t* slots, const uint64_t* slotSegs, ZskKernel tableKernel, const void* tableArgs)
{
    ZskScanArgs s; memset(&s, 0, sizeof s);
    s.in = (const uint8_t*)a.outSizes; s.status = a.status; s.mode = 0; s.n = a.n; s.offs = (uint64_t*)a.offs; s.partSum = partSum; s.partBad = (uint64_t*)a.partBad;
    if (int rc = zsk_launch_scan(b, s)) return rc;
    b.launch(ZSK_K_VERDICT, 1, &a);
    b.launch(tableKernel, zsk_lane_grid(b.numCU, a.n), tableArgs);
    if (int rc = b.check()) return rc;
    if (a.n) {
        b.compact(zsk_compact_grid(b.numCU, a.n), slots, slotSegs, a.outSizes, a.status, a.offs, a.n, a.dst);
        if (int rc = b.check()) return rc;
    }
    return 0;
}

// One large buffer as the batch the kernels are fast at: chunks of frameSize bytes -> the batch -> frames back to back + the seek table
template <class B> int zsk_compress(B& b, bool ctx, const void* d_src, uint64_t srcSize, uint32_t frameSize, int flags, void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status)
{
    if (int rc = zsk_compress_check(ctx && d_streamSize && d_status, srcSize, frameSize, flags, b.err)) return rc;
    const size_t n = (size_t)zsk_frame_count(srcSize, frameSize);
    const ZskCompressLayout l = zsk_compress_layout(n);
    uint8_t* m = nullptr; uint8_t* slots = nullptr;
    if (int rc = b.reserve(ZSK_A_SK_META, l.metaBytes, &m)) return rc;
    if (n) if (int rc = b.reserve(ZSK_A_SK_SLOTS, (size_t)(n * zsk_slot_stride(frameSize)), &slots)) return rc;
    ZskCompressArgs a; memset(&a, 0, sizeof a);
    a.src = (const uint8_t*)d_src; a.srcSize = srcSize; a.frameSize = frameSize; a.n = (uint32_t)n; a.checksum = flags & ZHIP_SEEKABLE_CHECKSUM ? 1u : 0u;
    a.srcSegs = (uint64_t*)(m + l.oSrcSegs); a.slotSegs = (uint64_t*)(m + l.oSlotSegs); a.outSizes = (const uint64_t*)(m + l.oSizes); a.status = (int32_t*)(m + l.oStatus);
    a.offs = (const uint64_t*)(m + l.oOffs); a.partBad = (const uint64_t*)(m + l.oPartBad);
    a.dst = (uint8_t*)d_dst; a.dstCapacity = dstCapacity; a.streamSize = d_streamSize; a.outStatus = d_status; a.go = (uint32_t*)(m + l.oGo);
    if (n) {
        b.launch(ZSK_K_CHUNK_SEGS, zsk_lane_grid(b.numCU, n), &a);
        if (int rc = b.check()) return rc;
        // the batch knows its largest source, as the host-buffer calls' batches do; the caller's own size hint is not touched
        if (int rc = b.compress(a.src, a.srcSegs, n, slots, a.slotSegs, (uint64_t*)(m + l.oSizes), a.status, (size_t)(srcSize < frameSize ? srcSize : frameSize))) return rc;
    }
    uint32_t span; a.nPart = zsk_scan_shape(a.n, &span);
    return zsk_compress_tail(b, a, (uint64_t*)(m + l.oPartSum), slots, a.slotSegs, ZSK_K_TABLE, &a);
}

// The front half of a call that compresses a caller's record table: the pre-check (two scans, a verdict), the segments, the batch into the context's slots.
// Reserves the meta area (the layout's bytes and extraMeta behind them) and the slots, fills *out with everything but the caller's dst / streamSize / outStatus.
template <class B> int zsk_records_front(B& b, const ZskRecordsLayout& l, size_t extraMeta, const void* d_src, uint64_t srcSize, const zhip_segment* d_records, size_t n,
                                         uint64_t maxContentBytes, uint64_t maxRecordBytes, int flags, ZskRecordsArgs* out, uint8_t** meta, uint8_t** slotArea)
{
    maxContentBytes = zsk_records_content_cap(maxContentBytes, n, maxRecordBytes);
    uint8_t* m = nullptr; uint8_t* slots = nullptr;
    if (int rc = b.reserve(ZSK_A_SK_META, l.metaBytes + extraMeta, &m)) return rc;
    if (n) if (int rc = b.reserve(ZSK_A_SK_SLOTS, (size_t)zsk_records_slot_bytes(maxContentBytes, n), &slots)) return rc;
    uint32_t* const words = (uint32_t*)(m + l.oGo);                        // go, pre, the pre-check's status pair
    ZskRecordsArgs r; memset(&r, 0, sizeof r);
    r.src = (const uint8_t*)d_src; r.srcSize = srcSize; r.records = (const uint64_t*)d_records; r.n = (uint32_t)n; r.checksum = flags & ZHIP_SEEKABLE_CHECKSUM ? 1u : 0u;
    r.maxContent = maxContentBytes; r.lenOffs = (const uint64_t*)(m + l.oLenOffs); r.slotOffs = (const uint64_t*)(m + l.oSlotOffs); r.partBad = (const uint64_t*)(m + l.oPreBad);
    r.srcSegs = (uint64_t*)(m + l.oSrcSegs); r.slotSegs = (uint64_t*)(m + l.oSlotSegs); r.pre = words + 1; r.preStatus = (int32_t*)(words + 2);
    r.outSizes = (const uint64_t*)(m + l.oSizes); r.status = (int32_t*)(m + l.oStatus); r.offs = (const uint64_t*)(m + l.oOffs); r.go = words;
    ZskScanArgs s; memset(&s, 0, sizeof s);
    s.in = (const uint8_t*)d_records + 8; s.stride = 16; s.mode = 3; s.n = (uint32_t)n; s.limit64 = maxRecordBytes; s.srcSize = srcSize;
    s.offs = (uint64_t*)(m + l.oLenOffs); s.partSum = (uint64_t*)(m + l.oPartSum); s.partBad = (uint64_t*)(m + l.oPreBad);
    uint32_t span; r.nPart = zsk_scan_shape(s.n, &span);
    if (int rc = zsk_launch_scan(b, s)) return rc;
    s.mode = 4; s.offs = (uint64_t*)(m + l.oSlotOffs); s.partBad = (uint64_t*)(m + l.oPartBad);
    if (int rc = zsk_launch_scan(b, s)) return rc;
    b.launch(ZSK_K_RECORDS_VERDICT, 1, &r);
    if (int rc = b.check()) return rc;
    if (n) {
        b.launch(ZSK_K_RECORDS_SEGS, zsk_lane_grid(b.numCU, n), &r);
        if (int rc = b.check()) return rc;
        // the batch's largest source is what the caller says it is; the caller's own size hint is not touched
        if (int rc = b.compress(r.src, r.srcSegs, n, slots, r.slotSegs, (uint64_t*)(m + l.oSizes), r.status, (size_t)maxRecordBytes)) return rc;
    }
    *out = r; *meta = m; *slotArea = slots;
    return 0;
}

// zsk_compress with the caller's record table in the place of the fixed cut: the front half above, then the same tail with the records' table writer
template <class B> int zsk_compress_records(B& b, bool ctx, const void* d_src, uint64_t srcSize, const zhip_segment* d_records, size_t n, uint64_t maxContentBytes, uint64_t maxRecordBytes, int flags,
                                            void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status)
{
    if (int rc = zsk_records_check(ctx && d_streamSize && d_status, d_records, n, maxRecordBytes, flags, b.err)) return rc;
    const ZskRecordsLayout l = zsk_records_layout(n);
    ZskRecordsArgs r; uint8_t* m; uint8_t* slots;
    if (int rc = zsk_records_front(b, l, 0, d_src, srcSize, d_records, n, maxContentBytes, maxRecordBytes, flags, &r, &m, &slots)) return rc;
    r.dst = (uint8_t*)d_dst; r.streamSize = d_streamSize; r.outStatus = d_status;
    ZskCompressArgs a; memset(&a, 0, sizeof a);
    a.n = (uint32_t)n; a.checksum = r.checksum; a.nPart = r.nPart; a.outSizes = r.outSizes; a.status = r.status; a.offs = r.offs; a.partBad = (const uint64_t*)(m + l.oPartBad);
    a.dst = (uint8_t*)d_dst; a.dstCapacity = dstCapacity; a.streamSize = d_streamSize; a.outStatus = d_status; a.go = (uint32_t*)(m + l.oGo);
    return zsk_compress_tail(b, a, (uint64_t*)(m + l.oPartSum), slots, r.slotSegs, ZSK_K_RECORDS_TABLE, &r);
}

// The open call: the footer and the table's header read back, then the three scans of the table's columns, their read-backs and the verdict. Every entry lies
// inside the stream once the header has passed; the kernels check what the entries SAY and build the offsets. Returns the ZHIP_ERR_* kind; *zerr the zstd
// error code and *index the entry where kind is ZHIP_ERR_ZSTD
template <class B> int zsk_open(B& b, const void* d_stream, uint64_t streamSize, ZskOpened* h, int* zerr, size_t* index)
{
    const uint8_t* const base = (const uint8_t*)d_stream;
    *zerr = 0; *index = 0;
    ZskLayout lay;
    if (streamSize < ZSK_HEADER + ZSK_FOOTER) { *zerr = ZSK_ERR_CORRUPT; return ZHIP_ERR_ZSTD; }
    uint8_t foot[ZSK_FOOTER], head[ZSK_HEADER];
    if (b.copy(foot, base + streamSize - ZSK_FOOTER, ZSK_FOOTER, ZSK_COPY_TO_HOST) || b.wait()) return zsk_refuse(b.err, ZHIP_ERR_HIP, "seekable open: reading the footer failed");
    if ((*zerr = zsk_parse_footer(foot, streamSize, &lay))) return ZHIP_ERR_ZSTD;
    if (b.copy(head, base + lay.tableOffset, ZSK_HEADER, ZSK_COPY_TO_HOST) || b.wait()) return zsk_refuse(b.err, ZHIP_ERR_HIP, "seekable open: reading the table's header failed");
    if ((*zerr = zsk_check_header(head, &lay))) return ZHIP_ERR_ZSTD;
    h->stream = base; h->streamSize = streamSize; h->lay = lay;
    const size_t n = lay.n;
    const ZskOpenLayout l = zsk_open_layout(n);
    uint8_t* pre = nullptr; uint8_t* pm = nullptr;
    if (int rc = b.reserve(ZSK_A_PREFIX, l.prefixBytes, &pre)) return rc;
    if (int rc = b.reserve(ZSK_A_META, l.metaBytes, &pm)) return rc;
    h->pre = pre;
    const uint8_t* const entries = base + lay.tableOffset + ZSK_HEADER;
    for (int k = 0; k < 3; k++) {
        ZskScanArgs s; memset(&s, 0, sizeof s);
        s.in = entries + (k ? 4 : 0); s.stride = lay.entry; s.mode = k == 2 ? 2u : 1u; s.limit = k == 1 ? ZSK_MAX_CONTENT : 0xFFFFFFFFu; s.n = lay.n;
        s.offs = (uint64_t*)(pre + k * l.col); s.partSum = (uint64_t*)(pm + 2 * k * l.part); s.partBad = (uint64_t*)(pm + (2 * k + 1) * l.part);
        if (zsk_launch_scan(b, s)) return ZHIP_ERR_HIP;
    }
    uint32_t span; const uint32_t grid = zsk_scan_shape(lay.n, &span);
    std::vector<uint64_t> bad(grid);
    uint64_t compressedTotal = 0;
    h->cOff.resize(n + 1); h->dOff.resize(n + 1); h->place.resize(n + 1);
    if (b.copy(h->cOff.data(), pre, (n + 1) * 8, ZSK_COPY_TO_HOST) || b.copy(h->dOff.data(), pre + l.col, (n + 1) * 8, ZSK_COPY_TO_HOST) || b.copy(h->place.data(), pre + 2 * l.col, (n + 1) * 8, ZSK_COPY_TO_HOST) ||
        b.copy(bad.data(), pm + 3 * l.part, grid * 8, ZSK_COPY_TO_HOST) || b.copy(&compressedTotal, pre + n * 8, 8, ZSK_COPY_TO_HOST) || b.wait()) return zsk_refuse(b.err, ZHIP_ERR_HIP, "seekable open: reading the table's scans failed");
    uint64_t lowestBad = ZSK_NONE;
    for (uint64_t v : bad) if (v < lowestBad) lowestBad = v;
    if ((*zerr = zsk_table_verdict(lowestBad, compressedTotal, &lay))) { *index = lowestBad != ZSK_NONE ? (size_t)lowestBad : 0; return ZHIP_ERR_ZSTD; }
    h->contentSize = h->dOff[n];
    for (size_t i = 0; i < n; i++) { const uint64_t d = h->dOff[i + 1] - h->dOff[i]; if (d > h->maxFrameContent) h->maxFrameContent = (uint32_t)d; }
    return 0;
}

// One range: the frames that cover it are one decode batch; the frames the range cuts decode into the edge area and their covered parts are copied
template <class B> int zsk_range(B& b, bool ctx, const ZskOpened* h, uint64_t offset, uint64_t length, void* d_dst, int32_t* d_status)
{
    if (!ctx || !h || !d_status) return zsk_refuse(b.err, ZHIP_ERR_UNSUPPORTED, "seekable decompress: bad arguments");
    if (int rc = zsk_range_check(offset, length, h->contentSize, b.err)) return rc;
    if (!length) return b.zero(d_status, 2 * sizeof(int32_t));
    if (!d_dst) return zsk_refuse(b.err, ZHIP_ERR_UNSUPPORTED, "seekable decompress: bad arguments");
    const uint64_t end = offset + length;
    // the frames that hold the range's first and last byte (both hold content: upper_bound steps over frames of none)
    const std::vector<uint64_t>& D = h->dOff;
    const uint32_t f0 = (uint32_t)(std::upper_bound(D.begin(), D.end(), offset) - D.begin() - 1), f1 = (uint32_t)(std::upper_bound(D.begin(), D.end(), end - 1) - D.begin() - 1);
    const size_t count = (size_t)(h->place[f1 + 1] - h->place[f0]);
    const bool cut0 = D[f0] < offset || D[f0 + 1] > end, cut1 = f1 != f0 && D[f1 + 1] > end;
    const size_t edgeBytes = (size_t)((cut0 ? D[f0 + 1] - D[f0] : 0) + (cut1 ? D[f1 + 1] - D[f1] : 0));
    const ZskItemsLayout l = zsk_items_layout(count, 16);
    uint8_t* m = nullptr; uint8_t* edge = nullptr;
    if (int rc = b.reserve(ZSK_A_META, l.metaBytes, &m)) return rc;
    if (edgeBytes) if (int rc = b.reserve(ZSK_A_EDGE, edgeBytes, &edge)) return rc;
    const uint8_t* const pre = h->pre; const size_t col = zsk_open_layout(h->lay.n).col;
    ZskRangeArgs a; memset(&a, 0, sizeof a);
    a.cOff = (const uint64_t*)pre; a.dOff = (const uint64_t*)(pre + col); a.place = (const uint64_t*)(pre + 2 * col);
    a.table = h->stream + h->lay.tableOffset + ZSK_HEADER; a.entry = h->lay.entry; a.checksum = (uint32_t)h->lay.checksum;
    a.f0 = f0; a.f1 = f1; a.count = (uint32_t)count; a.offset = offset; a.length = length;
    a.dst = (uint8_t*)d_dst; a.edge = edgeBytes ? edge : a.dst; a.dstBase = a.edge < a.dst ? a.edge : a.dst;
    a.srcSegs = (uint64_t*)(m + l.oSrcSegs); a.dstSegs = (uint64_t*)(m + l.oDstSegs); a.frameOf = (uint32_t*)(m + l.oFrameOf);
    a.outSizes = (const uint64_t*)(m + l.oSizes); a.status = (int32_t*)(m + l.oStatus); a.worst = (uint32_t*)(m + l.oWorst); a.outStatus = d_status;
    if (int rc = b.zero(a.worst, 4)) return rc;
    b.launch(ZSK_K_RANGE_SEGS, zsk_lane_grid(b.numCU, (uint64_t)f1 - f0 + 1), &a);
    if (int rc = b.check()) return rc;
    if (int rc = b.decompress(*h, a.srcSegs, count, a.dstBase, a.dstSegs, (uint64_t*)(m + l.oSizes), a.status)) return rc;
    b.launch(ZSK_K_RANGE_VERIFY, zsk_lane_grid(b.numCU, count), &a);
    b.launch(ZSK_K_RANGE_FINISH, zsk_lane_grid(b.numCU, (uint64_t)edgeBytes / 16 + 1), &a);
    return b.check();
}

// Many ranges in one decode batch per pass of the plan. stats (where given) receives the plan's counts
template <class B> int zsk_ranges(B& b, bool ctx, const ZskOpened* h, const uint64_t* rg, size_t R, void* d_dst, uint64_t dstCapacity, int32_t* d_status, zhip_seekable_gather_stats* stats, size_t* bad)
{
    bool any = false;
    if (int rc = zsk_ranges_check(ctx && h && d_status, rg, R, h ? h->contentSize : 0, d_dst, dstCapacity, bad, &any, b.err)) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    if (!any) return b.zero(d_status, (2 + 2 * R) * sizeof(int32_t));

    ZskGatherPlan plan;
    zsk_gather_plan(h->dOff.data(), h->place.data(), h->lay.n, rg, R, h->scratchLimit, &plan);
    if (stats) { stats->items = plan.items; stats->inPlace = plan.inPlace; stats->scratchBytes = plan.scratchBytes; stats->copyJobs = plan.jobs.size(); stats->passes = plan.passes.size(); }
    const size_t S = plan.segs.size(), J = plan.jobs.size();
    const ZskGatherLayout l = zsk_gather_layout(R, S, J, (size_t)plan.items);
    // (the scratch is allocated at exactly what the largest pass needs: it never exceeds max(limit, largest scratch frame))
    uint8_t* t = nullptr; uint8_t* m = nullptr; uint8_t* scratch = nullptr; uint8_t* pin = nullptr;
    if (int rc = b.reserve(ZSK_A_G_TABLES, l.tableBytes, &t)) return rc;
    if (int rc = b.reserve(ZSK_A_G_META, l.m.metaBytes, &m)) return rc;
    if (plan.scratchMax) if (int rc = b.reserve(ZSK_A_G_SCRATCH, (size_t)plan.scratchMax, &scratch)) return rc;
    if (int rc = b.reserve(ZSK_A_PIN, l.tableBytes, &pin)) return rc;
    memcpy(pin + l.oRanges, plan.ranges.data(), R * sizeof(ZskGatherRange));
    if (S) memcpy(pin + l.oSegs, plan.segs.data(), S * sizeof(ZskGatherSeg));
    if (J) memcpy(pin + l.oJobs, plan.jobs.data(), J * sizeof(ZskGatherJob));
    if (int rc = b.copy(t, pin, l.tableBytes, ZSK_COPY_FROM_PIN)) return rc;
    if (int rc = b.zero(m + l.m.oWorst, R * 4)) return rc;

    const uint8_t* const pre = h->pre; const size_t col = zsk_open_layout(h->lay.n).col;
    ZskGatherArgs a; memset(&a, 0, sizeof a);
    a.cOff = (const uint64_t*)pre; a.dOff = (const uint64_t*)(pre + col); a.place = (const uint64_t*)(pre + 2 * col);
    a.table = h->stream + h->lay.tableOffset + ZSK_HEADER; a.entry = h->lay.entry; a.checksum = (uint32_t)h->lay.checksum;
    a.ranges = (const ZskGatherRange*)(t + l.oRanges); a.nRanges = (uint32_t)R;
    a.dst = (uint8_t*)d_dst; a.scratch = plan.scratchMax ? scratch : a.dst; a.dstBase = a.scratch < a.dst ? a.scratch : a.dst;
    a.srcSegs = (uint64_t*)(m + l.m.oSrcSegs); a.dstSegs = (uint64_t*)(m + l.m.oDstSegs); a.frameOf = (uint32_t*)(m + l.m.oFrameOf);
    a.outSizes = (const uint64_t*)(m + l.m.oSizes); a.status = (int32_t*)(m + l.m.oStatus); a.worst = (uint32_t*)(m + l.m.oWorst); a.outStatus = d_status;
    int rc = 0;
    for (size_t p = 0; p < plan.passes.size() && !rc; p++) {
        const ZskGatherPass& ps = plan.passes[p];
        a.segs = (const ZskGatherSeg*)(t + l.oSegs) + ps.seg0; a.nSegs = ps.seg1 - ps.seg0; a.frames = ps.frames;
        a.jobs = (const ZskGatherJob*)(t + l.oJobs) + ps.job0; a.nJobs = ps.job1 - ps.job0; a.tiles = ps.tiles;
        a.item0 = ps.item0; a.count = ps.item1 - ps.item0; a.last = p + 1 == plan.passes.size() ? 1u : 0u;
        b.launch(ZSK_K_GATHER_SEGS, zsk_lane_grid(b.numCU, ps.frames), &a);
        if (a.count) {
            rc = b.decompress(*h, a.srcSegs + 2 * (size_t)a.item0, a.count, a.dstBase, a.dstSegs + 2 * (size_t)a.item0, (uint64_t*)(m + l.m.oSizes) + a.item0, a.status + a.item0);
            if (rc) break;
            b.launch(ZSK_K_GATHER_VERIFY, zsk_lane_grid(b.numCU, a.count), &a);
        }
        if (a.tiles || a.last) {
            const uint64_t lanes = a.tiles * 64 > (a.last ? R : 0) ? a.tiles * 64 : R;
            b.launch(ZSK_K_GATHER_FINISH, zsk_lane_grid(b.numCU, lanes), &a);
        }
        if (b.check()) rc = zsk_refuse(b.err, ZHIP_ERR_HIP, "seekable ranges: a launch failed");
    }
    return rc;
}

// The edit call's per-pick half: the stash (in place), the upload of the picks from `pin`, then sizes, the two scans, the verdict, the copy, the table.
// e arrives with the records' results (zsk_records_front's, or none); m is the meta area the layout's offsets count from
template <class B> int zsk_edit_picks(B& b, const ZskOpened* old, const ZskEditPick* pk, size_t n, bool inPlace, uint32_t checksum, const ZskEditLayout& l, uint8_t* m, uint8_t* pin, ZskEditArgs e,
                                      void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status)
{
    const uint32_t nOld = old ? old->lay.n : 0;
    if (old) {
        e.old = old->stream; e.cOff = (const uint64_t*)old->pre; e.oldEntries = old->stream + old->lay.tableOffset + ZSK_HEADER;
        if (inPlace && nOld) {      // the new frames overwrite the old table: its entries are kept aside first
            if (int rc = b.copy(m + l.oStash, e.oldEntries, (size_t)nOld * zsk_entry_size((int)checksum), ZSK_COPY_ON_DEVICE)) return rc;
            e.oldEntries = m + l.oStash;
        }
        if (inPlace) e.firstPick = nOld;
    }
    if (n) {
        memcpy(pin, pk, n * sizeof(ZskEditPick));
        if (int rc = b.copy(m + l.oPicks, pin, n * sizeof(ZskEditPick), ZSK_COPY_FROM_PIN)) return rc;
    }
    e.picks = (const ZskEditPick*)(m + l.oPicks); e.pickSize = (uint64_t*)(m + l.oPickSize); e.pickStatus = (int32_t*)(m + l.oPickStatus); e.tileOffs = (const uint64_t*)(m + l.oTileOffs);
    ZskCompressArgs& a = e.v;
    a.n = (uint32_t)n; a.checksum = checksum; a.status = e.pickStatus; a.outSizes = e.pickSize; a.offs = (const uint64_t*)(m + l.oOffs); a.partBad = (const uint64_t*)(m + l.oPartBad);
    a.dst = (uint8_t*)d_dst; a.dstCapacity = dstCapacity; a.streamSize = d_streamSize; a.outStatus = d_status; a.go = (uint32_t*)(m + l.oGo);
    uint32_t span; a.nPart = zsk_scan_shape(a.n, &span);
    b.launch(ZSK_K_EDIT_SIZES, zsk_lane_grid(b.numCU, n), &e);
    if (int rc = b.check()) return rc;
    ZskScanArgs s; memset(&s, 0, sizeof s);
    s.in = m + l.oPickSize; s.status = e.pickStatus; s.mode = 0; s.n = (uint32_t)n; s.offs = (uint64_t*)(m + l.oOffs); s.partSum = (uint64_t*)(m + l.oPartSum); s.partBad = (uint64_t*)(m + l.oPartBad);
    if (int rc = zsk_launch_scan(b, s)) return rc;
    s.mode = 5; s.status = nullptr; s.offs = (uint64_t*)(m + l.oTileOffs); s.partBad = (uint64_t*)(m + l.oTileBad);
    if (int rc = zsk_launch_scan(b, s)) return rc;
    b.launch(ZSK_K_EDIT_VERDICT, 1, &e);
    b.launch(ZSK_K_EDIT_COPY, zsk_edit_copy_grid(b.numCU, dstCapacity, n), &e);
    b.launch(ZSK_K_EDIT_TABLE, zsk_lane_grid(b.numCU, n), &e);
    return b.check();
}

// The records call's front half (where there are records), then everything per PICK
template <class B> int zsk_edit(B& b, bool ctx, const ZskOpened* old, const ZskEditPick* pk, size_t n, const void* d_src, uint64_t srcSize, const zhip_segment* d_records, size_t nRecords,
                                uint64_t maxContentBytes, uint64_t maxRecordBytes, int flags, void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status)
{
    bool inPlace = false; size_t bad = 0;
    if (int rc = zsk_edit_call_check(ctx && d_streamSize && d_status, old, pk, n, d_records, nRecords, maxRecordBytes, flags, d_dst, dstCapacity, &inPlace, &bad, b.err)) return rc;
    const uint32_t checksum = flags & ZHIP_SEEKABLE_CHECKSUM ? 1u : 0u;
    const ZskEditLayout l = zsk_edit_layout(n, nRecords, old ? old->lay.n : 0, inPlace, zsk_entry_size((int)checksum));
    uint8_t* pin = nullptr; uint8_t* m = nullptr; uint8_t* slots = nullptr;
    if (n) if (int rc = b.reserve(ZSK_A_PIN, n * sizeof(ZskEditPick), &pin)) return rc;
    ZskEditArgs e; memset(&e, 0, sizeof e);
    if (nRecords) {
        const ZskRecordsLayout rl = zsk_records_layout(nRecords);
        ZskRecordsArgs r;
        if (int rc = zsk_records_front(b, rl, l.end - rl.metaBytes, d_src, srcSize, d_records, nRecords, maxContentBytes, maxRecordBytes, flags, &r, &m, &slots)) return rc;
        e.src = r.src; e.records = r.records; e.slots = slots; e.slotSegs = r.slotSegs; e.recSizes = r.outSizes; e.recStatus = r.status; e.pre = r.pre; e.preStatus = r.preStatus;
    } else if (int rc = b.reserve(ZSK_A_SK_META, l.end, &m)) return rc;
    return zsk_edit_picks(b, old, pk, n, inPlace, checksum, l, m, pin, e, d_dst, dstCapacity, d_streamSize, d_status);
}
