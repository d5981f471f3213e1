// zhip_seekable.hpp -- the zstd seekable format on the device: independent frames back to back, then one skippable frame that holds a seek table
//
//     Skippable_Magic_Number 0x184D2A5E | Frame_Size = n * E + 9 | n entries of E = 8 (12 with checksums) bytes | Number_Of_Frames | Descriptor | 0x8F92EAB1
//
// (all little-endian; an entry is Compressed_Size, Decompressed_Size and, with bit 7 of the descriptor, the low 32 bits of XXH64 of the frame's content).
// What is here: the format's arithmetic and checks (plain functions, host and device), and the kernels around the batch calls -- chunk segments, a
// multi-workgroup exclusive scan of 64-bit sizes, the table writer, their twins for a caller's record table (one frame per record), the range pieces
// (segment builder, size / checksum verifier, edge copy), and the edit pieces (pick sizes, verdict, the tiled copy of kept and new frames, the table).
// Every kernel is one-wave workgroups written against zhip_device.hpp, so the same bodies run under the host wave emulator (tests/emu/emu_seekable.cpp).
#pragma once
#include "zhip_device.hpp"
#include "zhip_xxh64.hpp"
#include <string.h>
#include <algorithm>
#include <vector>

#ifndef ZHIP_EMU
#define ZSK_HD __host__ __device__ static inline
#else
#define ZSK_HD static inline
#endif

#define ZSK_SKIP_MAGIC 0x184D2A5Eu
#define ZSK_SEEK_MAGIC 0x8F92EAB1u
#define ZSK_MAX_FRAMES 0x8000000u            // 2^27
#define ZSK_MAX_CONTENT 0x40000000u          // 2^30: most bytes one frame may decompress to
#define ZSK_FOOTER 9u                        // Number_Of_Frames, descriptor, magic
#define ZSK_HEADER 8u                        // skippable magic, Frame_Size
#define ZSK_ERR_PREFIX 10
#define ZSK_ERR_CORRUPT 20
#define ZSK_ERR_CHECKSUM 22
#define ZSK_ERR_DSTSIZE 70
#define ZSK_NONE (~(uint64_t)0)

// the scan's tiles: a workgroup is one wave; a lane takes ZSK_SCAN_PER_LANE neighbouring items of a tile, a workgroup walks a contiguous span of whole tiles,
// and a launch has at most ZSK_SCAN_GRID workgroups -- beyond ZSK_SCAN_GRID tiles (one full grid pass) the spans are several tiles long
#define ZSK_SCAN_LANES 64u
#define ZSK_SCAN_PER_LANE 4u
#define ZSK_SCAN_TILE (ZSK_SCAN_LANES * ZSK_SCAN_PER_LANE)
#define ZSK_SCAN_GRID 1024u
#define ZSK_COPY_TILE 4096u                  // bytes one workgroup copies per step: 4 x 16 bytes per lane

ZSK_HD uint64_t zsk_compress_bound(uint64_t n) { return n + (n >> 8) + (n < (128u << 10) ? (((128u << 10) - n) >> 11) : 0); }      // == zhip_compress_bound
ZSK_HD uint64_t zsk_frame_count(uint64_t srcSize, uint32_t frameSize) { return frameSize ? srcSize / frameSize + (srcSize % frameSize ? 1 : 0) : 0; }
ZSK_HD uint32_t zsk_entry_size(int checksum) { return checksum ? 12u : 8u; }
ZSK_HD uint64_t zsk_table_size(uint64_t n, int checksum) { return ZSK_HEADER + n * zsk_entry_size(checksum) + ZSK_FOOTER; }
ZSK_HD bool zsk_args_ok(uint64_t srcSize, uint32_t frameSize) { return frameSize >= 1 && frameSize <= ZSK_MAX_CONTENT && zsk_frame_count(srcSize, frameSize) <= ZSK_MAX_FRAMES; }
// distance between the compressBound-sized slots the chunks are compressed into (16-byte aligned: the compaction reads a slot 16 bytes at a time)
ZSK_HD uint64_t zsk_slot_stride(uint32_t frameSize) { return (zsk_compress_bound(frameSize) + 15) & ~(uint64_t)15; }
ZSK_HD uint64_t zsk_bound(uint64_t srcSize, uint32_t frameSize, int checksum)
{
    if (!zsk_args_ok(srcSize, frameSize)) return 0;
    const uint64_t n = zsk_frame_count(srcSize, frameSize);
    if (!n) return zsk_table_size(0, checksum);
    return (n - 1) * zsk_compress_bound(frameSize) + zsk_compress_bound(srcSize - (n - 1) * frameSize) + zsk_table_size(n, checksum);
}

struct ZskLayout { uint32_t n, entry; int checksum; uint64_t tableOffset; };      // tableOffset: where the table frame starts == what the compressed sizes must sum to
static inline uint32_t zsk_rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
// the last 9 bytes of a stream of streamSize bytes -> the table's shape. 0, or the zstd error code
static inline int zsk_parse_footer(const uint8_t* footer, uint64_t streamSize, ZskLayout* l)
{
    if (streamSize < ZSK_HEADER + ZSK_FOOTER) return ZSK_ERR_CORRUPT;
    if (zsk_rd32(footer + 5) != ZSK_SEEK_MAGIC) return ZSK_ERR_PREFIX;
    const uint32_t desc = footer[4];
    if (desc & 0x7Cu) return ZSK_ERR_CORRUPT;                                  // reserved bits 6..2 (bits 1..0 are unused: ignored)
    l->checksum = (desc >> 7) & 1; l->entry = zsk_entry_size(l->checksum);
    l->n = zsk_rd32(footer);
    if (l->n > ZSK_MAX_FRAMES) return ZSK_ERR_CORRUPT;
    const uint64_t table = zsk_table_size(l->n, l->checksum);
    if (table > streamSize) return ZSK_ERR_CORRUPT;
    l->tableOffset = streamSize - table;
    return 0;
}
// the 8 bytes at l->tableOffset
static inline int zsk_check_header(const uint8_t* header, const ZskLayout* l)
{
    if (zsk_rd32(header) != ZSK_SKIP_MAGIC) return ZSK_ERR_PREFIX;
    if ((uint64_t)zsk_rd32(header + 4) != (uint64_t)l->n * l->entry + ZSK_FOOTER) return ZSK_ERR_CORRUPT;
    return 0;
}
// what the kernels found: the lowest entry with a Decompressed_Size above the limit (ZSK_NONE: none) and the sum of the Compressed_Size column
static inline int zsk_table_verdict(uint64_t lowestBad, uint64_t compressedTotal, const ZskLayout* l) { return lowestBad != ZSK_NONE || compressedTotal != l->tableOffset ? ZSK_ERR_CORRUPT : 0; }

// ------------------------------------------------------------------------------------------------ wave helpers (64-bit values over the 32-bit shuffles)
ZH_DEV uint64_t zsk_shfl64(uint64_t v, uint32_t srcLane) { const uint32_t lo = zh_shfl((uint32_t)v, srcLane), hi = zh_shfl((uint32_t)(v >> 32), srcLane); return ((uint64_t)hi << 32) | lo; }
ZH_DEV uint64_t zsk_wave_sum64(uint64_t v) { for (uint32_t d = 32; d; d >>= 1) v += zsk_shfl64(v, zh_lane() ^ d); return v; }
ZH_DEV uint64_t zsk_wave_min64(uint64_t v) { for (uint32_t d = 32; d; d >>= 1) { const uint64_t o = zsk_shfl64(v, zh_lane() ^ d); v = o < v ? o : v; } return v; }
ZH_DEV uint64_t zsk_wave_scan64(uint64_t v)          // inclusive
{
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t lo = zh_shfl_up((uint32_t)v, d), hi = zh_shfl_up((uint32_t)(v >> 32), d);
        if (zh_lane() >= d) v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// ------------------------------------------------------------------------------------------------ the scan
// Exclusive prefix sums of n 64-bit sizes in two launches of the same grid: zsk_scan_reduce (a workgroup's span -> its sum and its lowest bad item) and
// zsk_scan_write (the sums of the workgroups in front, then the span again tile by tile). No workgroup waits for another one.
//   mode 0: in = uint64_t[n]; an item whose status is non-zero counts 0 and is "bad"
//   mode 1: in = a 32-bit column of the seek table (any alignment), `stride` bytes from entry to entry; an item above `limit` is "bad"
//   mode 2: the same column, an item counts 1 where it is non-zero (which place a frame has among those that hold content)
//   mode 3: in = the 64-bit length column of a record table (record i's length at in + i * stride, its offset 8 bytes in front; 8-byte aligned); an item counts
//           its length and is "bad" where the length is above limit64, or offset + length ends beyond srcSize or wraps
//   mode 4: the same column, an item counts (zsk_compress_bound(length) + 15) & ~15 -- the distance to the next record's slot; no item is bad
//   mode 5: in = uint64_t[n]; an item counts the copy tiles of that many bytes, ceil(size / ZSK_COPY_TILE); no item is bad
struct ZskScanArgs {
    const uint8_t* in; const int32_t* status; uint32_t stride, mode, limit, n;
    uint32_t span;                    // items per workgroup: whole tiles (zsk_scan_shape)
    uint64_t* offs;                   // [n + 1]: offs[n] = the total
    uint64_t* partSum; uint64_t* partBad;      // [grid]
    uint64_t limit64, srcSize;        // modes 3 and 4 (0 in the other modes)
};
static inline uint32_t zsk_scan_shape(uint32_t n, uint32_t* span)
{
    const uint32_t tiles = n / ZSK_SCAN_TILE + (n % ZSK_SCAN_TILE ? 1 : 0);
    const uint32_t grid = tiles < 1 ? 1 : tiles < ZSK_SCAN_GRID ? tiles : ZSK_SCAN_GRID;
    *span = (tiles / grid + (tiles % grid ? 1 : 0)) * ZSK_SCAN_TILE;
    return grid;
}
ZH_DEV uint64_t zsk_scan_item(const ZskScanArgs& a, uint32_t i, bool* bad)
{
    if (a.mode == 0) { const bool b = a.status[i] != 0; *bad = b; return b ? 0 : ((const uint64_t*)a.in)[i]; }
    if (a.mode == 5) { *bad = false; return (((const uint64_t*)a.in)[i] + ZSK_COPY_TILE - 1) / ZSK_COPY_TILE; }
    if (a.mode >= 3) {
        const uint64_t* const rec = (const uint64_t*)(a.in + (size_t)i * a.stride);
        const uint64_t len = rec[0];
        if (a.mode == 4) { *bad = false; return (zsk_compress_bound(len) + 15) & ~(uint64_t)15; }
        const uint64_t off = rec[-1];
        *bad = len > a.limit64 || off + len < off || off + len > a.srcSize;
        return len;
    }
    const uint32_t v = zh_ld32(a.in + (size_t)i * a.stride);
    *bad = v > a.limit;
    return a.mode == 1 ? (uint64_t)v : (uint64_t)(v != 0);
}
ZH_DEV void zsk_scan_reduce_body(const ZskScanArgs& a)
{
    const uint64_t lo64 = (uint64_t)zh_block() * a.span;
    const uint32_t lo = lo64 < a.n ? (uint32_t)lo64 : a.n, hi = a.n - lo < a.span ? a.n : lo + a.span;
    uint64_t sum = 0, lowest = ZSK_NONE;
    for (uint32_t i = lo + zh_lane(); i < hi; i += ZSK_SCAN_LANES) {
        bool bad; sum += zsk_scan_item(a, i, &bad);
        if (bad && lowest == ZSK_NONE) lowest = i;
    }
    sum = zsk_wave_sum64(sum); lowest = zsk_wave_min64(lowest);
    if (zh_lane() == 0) { a.partSum[zh_block()] = sum; a.partBad[zh_block()] = lowest; }
}
ZH_DEV void zsk_scan_write_body(const ZskScanArgs& a)
{
    const uint32_t b = zh_block();
    uint64_t base = 0, all = 0;
    for (uint32_t j = zh_lane(); j < zh_nblocks(); j += ZSK_SCAN_LANES) { const uint64_t s = a.partSum[j]; all += s; if (j < b) base += s; }
    base = zsk_wave_sum64(base);
    if (b == 0) { all = zsk_wave_sum64(all); if (zh_lane() == 0) a.offs[a.n] = all; }
    const uint64_t lo64 = (uint64_t)b * a.span;
    const uint32_t lo = lo64 < a.n ? (uint32_t)lo64 : a.n, hi = a.n - lo < a.span ? a.n : lo + a.span;
    for (uint32_t t = lo; t < hi; t += ZSK_SCAN_TILE) {                  // (t, hi are the same in every lane: the wave stays together through the shuffles)
        const uint32_t first = t + zh_lane() * ZSK_SCAN_PER_LANE;
        uint64_t v[ZSK_SCAN_PER_LANE], mine = 0;
        for (uint32_t k = 0; k < ZSK_SCAN_PER_LANE; k++) { bool bad; v[k] = first + k < hi ? zsk_scan_item(a, first + k, &bad) : 0; mine += v[k]; }
        const uint64_t incl = zsk_wave_scan64(mine);
        uint64_t run = base + incl - mine;
        for (uint32_t k = 0; k < ZSK_SCAN_PER_LANE; k++) if (first + k < hi) { a.offs[first + k] = run; run += v[k]; }
        base += zsk_shfl64(incl, 63);
    }
}

// ------------------------------------------------------------------------------------------------ compress: chunks, verdict, table
struct ZskCompressArgs {
    const uint8_t* src; uint64_t srcSize; uint32_t frameSize, n, checksum, nPart;
    uint64_t* srcSegs; uint64_t* slotSegs;      // [n][2]: (offset, length) of chunk i in src, of its slot in the slot area
    const uint64_t* outSizes; int32_t* status;  // [n]: what zhip_compress_batch_device wrote
    const uint64_t* offs;                       // [n + 1]: the scan of outSizes
    const uint64_t* partBad;                    // [nPart]: the scan's lowest failing frame per workgroup
    uint8_t* dst; uint64_t dstCapacity;
    uint64_t* streamSize; int32_t* outStatus;   // the caller's
    uint32_t* go;                               // 1: the stream is written; 0: it failed, nothing is
};
ZH_DEV uint32_t zsk_chunk_len(const ZskCompressArgs& a, uint32_t i) { const uint64_t at = (uint64_t)i * a.frameSize, left = a.srcSize - at; return left < a.frameSize ? (uint32_t)left : a.frameSize; }
// a lane per frame: where chunk i lies in the source, and the compressBound-sized slot it is compressed into
ZH_DEV void zsk_chunk_segs_body(const ZskCompressArgs& a)
{
    const uint64_t stride = zsk_slot_stride(a.frameSize);
    for (uint64_t i = (uint64_t)zh_block() * 64 + zh_lane(); i < a.n; i += (uint64_t)zh_nblocks() * 64) {
        const uint32_t len = zsk_chunk_len(a, (uint32_t)i);
        a.srcSegs[2 * i] = i * a.frameSize; a.srcSegs[2 * i + 1] = len;
        a.slotSegs[2 * i] = i * stride; a.slotSegs[2 * i + 1] = zsk_compress_bound(len);
    }
}
// one wave: the stream's status -- the lowest failing frame, else whether frames + table fit the capacity -- and its size
ZH_DEV void zsk_verdict_body(const ZskCompressArgs& a)
{
    uint64_t bad = ZSK_NONE;
    for (uint32_t j = zh_lane(); j < a.nPart; j += 64) { const uint64_t v = a.partBad[j]; bad = v < bad ? v : bad; }
    bad = zsk_wave_min64(bad);
    if (zh_lane() != 0) return;
    const uint64_t frames = a.offs[a.n], need = frames + zsk_table_size(a.n, (int)a.checksum);
    int32_t code = 0; uint32_t index = 0;
    if (bad != ZSK_NONE) { code = a.status[bad]; index = (uint32_t)bad; }
    else if (need > a.dstCapacity) {
        // the first frame that ends beyond the capacity; the last frame where only the table does not fit (offs is non-decreasing: bisect)
        uint32_t lo = 0, hi = a.n;
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (a.offs[mid + 1] > a.dstCapacity) hi = mid; else lo = mid + 1; }
        code = ZSK_ERR_DSTSIZE; index = lo < a.n ? lo : a.n ? a.n - 1 : 0;
    }
    a.outStatus[0] = code; a.outStatus[1] = (int32_t)index;
    *a.streamSize = code ? 0 : need;
    *a.go = code ? 0u : 1u;
}
// a lane per frame: its entry (with the checksum of the SOURCE chunk where asked for); lane 0 of the grid: the table frame's header and footer.
// A failed stream writes nothing: every frame's status is made non-zero instead, which is what keeps the compaction behind this kernel from copying.
ZH_DEV void zsk_table_body(const ZskCompressArgs& a)
{
    const bool go = *a.go != 0;
    const uint32_t entry = zsk_entry_size((int)a.checksum);
    uint8_t* const table = a.dst + a.offs[a.n];
    for (uint64_t i = (uint64_t)zh_block() * 64 + zh_lane(); i < a.n; i += (uint64_t)zh_nblocks() * 64) {
        if (!go) { if (!a.status[i]) a.status[i] = ZSK_ERR_DSTSIZE; continue; }
        const uint32_t len = zsk_chunk_len(a, (uint32_t)i);
        uint8_t* const e = table + ZSK_HEADER + i * entry;
        zh_st32(e, (uint32_t)a.outSizes[i]); zh_st32(e + 4, len);
        if (a.checksum) zh_st32(e + 8, (uint32_t)ze_xxh64(a.src + i * a.frameSize, len));
    }
    if (go && zh_block() == 0 && zh_lane() == 0) {
        uint8_t* const f = table + ZSK_HEADER + (uint64_t)a.n * entry;
        zh_st32(table, ZSK_SKIP_MAGIC); zh_st32(table + 4, a.n * entry + ZSK_FOOTER);
        zh_st32(f, a.n); f[4] = a.checksum ? 0x80 : 0; zh_st32(f + 5, ZSK_SEEK_MAGIC);
    }
}

// ------------------------------------------------------------------------------------------------ compress: records
// One frame per record: the caller's table of (offset, length) in device memory takes the place of the fixed cut. The host knows bounds only -- what the
// lengths sum to at most (it sizes the slot area), what a length is at most (the batch's size hint) --, so the device checks them before anything is
// compressed: two scans of the length column (mode 3: the lengths, with the per-record checks; mode 4: the slot strides), one wave's verdict, and a lane per
// record that hands the batch either the records and their slots or, after a failed check, n empty sources with 64-byte slots (zsk_compress_bound(0)) at 64 * i.
//
// The slot area. Record i's slot starts at the sum of the strides in front, a stride being zsk_compress_bound(len) rounded up to 16. zsk_compress_bound(len)
// = len + (len >> 8) + (len < 128 KiB ? (128 KiB - len) >> 11 : 0) <= len + (len >> 8) + 64, so a stride is at most len + (len >> 8) + 64 + 15, and
// sum(len >> 8) <= (sum len) >> 8: n records whose lengths sum to at most C need at most C + (C >> 8) + 79 * n bytes. The host reserves
// zsk_records_slot_bytes = C + (C >> 8) + 80 * n, which also holds the 64 * n bytes of the harmless form.
#define ZSK_ERR_SRCSIZE 72
ZSK_HD uint64_t zsk_records_slot_bytes(uint64_t maxContent, uint64_t n) { return maxContent + (maxContent >> 8) + 80 * n; }
// (no record is above maxRecord, so the lengths cannot sum to more than n of them: a generous maxContent does not size the slots)
ZSK_HD uint64_t zsk_records_content_cap(uint64_t maxContent, uint64_t n, uint64_t maxRecord) { return maxContent > n * maxRecord ? n * maxRecord : maxContent; }
ZSK_HD bool zsk_records_args_ok(uint64_t maxContent, uint64_t n) { return n <= ZSK_MAX_FRAMES && maxContent <= (uint64_t)ZSK_MAX_FRAMES * ZSK_MAX_CONTENT; }
// worst-case stream bytes: every frame at its zsk_compress_bound (the derivation above without the rounding), and the table
ZSK_HD uint64_t zsk_records_bound(uint64_t maxContent, uint64_t n, int checksum)
{
    if (!zsk_records_args_ok(maxContent, n)) return 0;
    return maxContent + (maxContent >> 8) + 64 * n + zsk_table_size(n, checksum);
}
struct ZskRecordsArgs {
    const uint8_t* src; uint64_t srcSize;
    const uint64_t* records;                    // [n][2]: the caller's (offset, length) of record i in src -- device memory
    uint32_t n, checksum, nPart;
    uint64_t maxContent;                        // what the lengths may sum to
    const uint64_t* lenOffs;                    // [n + 1]: the scan of the lengths (mode 3)
    const uint64_t* slotOffs;                   // [n + 1]: the scan of the slot strides (mode 4)
    const uint64_t* partBad;                    // [nPart]: the length scan's lowest bad record per workgroup
    uint64_t* srcSegs; uint64_t* slotSegs;      // [n][2]: what the batch call is handed
    uint32_t* pre; int32_t* preStatus;          // the pre-check's go word (1: passed) and its {code, index}
    const uint64_t* outSizes; int32_t* status;  // [n]: what zhip_compress_batch_device wrote
    const uint64_t* offs;                       // [n + 1]: the scan of outSizes
    const uint32_t* go;                         // zsk_verdict_body's word
    uint8_t* dst; uint64_t* streamSize; int32_t* outStatus;      // the caller's
};
// one wave: the pre-check's verdict -- the lowest record a lane of the scan refused, else the lowest record whose running end exceeds maxContent
ZH_DEV void zsk_records_verdict_body(const ZskRecordsArgs& a)
{
    uint64_t bad = ZSK_NONE;
    for (uint32_t j = zh_lane(); j < a.nPart; j += 64) { const uint64_t v = a.partBad[j]; bad = v < bad ? v : bad; }
    bad = zsk_wave_min64(bad);
    if (zh_lane() != 0) return;
    int32_t code = 0; uint32_t index = 0;
    if (bad != ZSK_NONE) { code = ZSK_ERR_SRCSIZE; index = (uint32_t)bad; }
    else if (a.lenOffs[a.n] > a.maxContent) {
        // (every length passed its check: at most 2^27 of at most 2^30, the sums did not wrap and do not decrease: bisect)
        uint32_t lo = 0, hi = a.n;
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (a.lenOffs[mid + 1] > a.maxContent) hi = mid; else lo = mid + 1; }
        code = ZSK_ERR_SRCSIZE; index = lo;
    }
    a.preStatus[0] = code; a.preStatus[1] = (int32_t)index;
    *a.pre = code ? 0u : 1u;
}
// a lane per record: its source segment and its slot. After a failed pre-check the batch still runs (the host cannot know the verdict): it is handed empty
// sources and 64-byte slots, all inside the source and the slot area whatever the records say
ZH_DEV void zsk_records_segs_body(const ZskRecordsArgs& a)
{
    const bool ok = *a.pre != 0;
    for (uint64_t i = (uint64_t)zh_block() * 64 + zh_lane(); i < a.n; i += (uint64_t)zh_nblocks() * 64) {
        const uint64_t len = ok ? a.records[2 * i + 1] : 0;
        a.srcSegs[2 * i] = ok ? a.records[2 * i] : 0; a.srcSegs[2 * i + 1] = len;
        a.slotSegs[2 * i] = ok ? a.slotOffs[i] : 64 * i; a.slotSegs[2 * i + 1] = zsk_compress_bound(len);
    }
}
// zsk_table_body's twin: a record's length and checksum come from the caller's table. Where the pre-check failed, lane 0 of the grid puts its status over
// what zsk_verdict_body made of the harmless batch and sets the stream size to 0; every frame's status is made non-zero as for any failed stream
ZH_DEV void zsk_records_table_body(const ZskRecordsArgs& a)
{
    const bool pre = *a.pre != 0, go = pre && *a.go != 0;
    const uint32_t entry = zsk_entry_size((int)a.checksum);
    uint8_t* const table = a.dst + a.offs[a.n];
    for (uint64_t i = (uint64_t)zh_block() * 64 + zh_lane(); i < a.n; i += (uint64_t)zh_nblocks() * 64) {
        if (!go) { if (!a.status[i]) a.status[i] = ZSK_ERR_DSTSIZE; continue; }
        const uint64_t at = a.records[2 * i]; const uint32_t len = (uint32_t)a.records[2 * i + 1];
        uint8_t* const e = table + ZSK_HEADER + i * entry;
        zh_st32(e, (uint32_t)a.outSizes[i]); zh_st32(e + 4, len);
        if (a.checksum) zh_st32(e + 8, (uint32_t)ze_xxh64(a.src + at, len));
    }
    if (zh_block() != 0 || zh_lane() != 0) return;
    if (go) {
        uint8_t* const f = table + ZSK_HEADER + (uint64_t)a.n * entry;
        zh_st32(table, ZSK_SKIP_MAGIC); zh_st32(table + 4, a.n * entry + ZSK_FOOTER);
        zh_st32(f, a.n); f[4] = a.checksum ? 0x80 : 0; zh_st32(f + 5, ZSK_SEEK_MAGIC);
    } else if (!pre) { a.outStatus[0] = a.preStatus[0]; a.outStatus[1] = a.preStatus[1]; *a.streamSize = 0; }
}

// reads by frame index: which content bytes a frame is (zhip_seekable_frame_offsets), and the range list zhip_seekable_decompress_frames_device hands the
// many-ranges plan -- rg [count][3] = {dOff[f], dOff[f + 1] - dOff[f], dstOffsets[k] or, without them, the sizes in front}. Returns count, or the position of
// the first index that is not a frame of the table
static inline bool zsk_frame_offsets(const uint64_t* D, uint32_t n, uint32_t first, uint32_t count, uint64_t* out)
{
    if (first > n || count > n - first) return false;
    for (uint64_t k = 0; k <= count; k++) out[k] = D[first + k];
    return true;
}
static inline size_t zsk_frames_to_ranges(const uint64_t* D, uint32_t n, const uint32_t* frames, size_t count, const uint64_t* dstOffsets, uint64_t* rg)
{
    uint64_t at = 0;
    for (size_t k = 0; k < count; k++) {
        const uint32_t f = frames[k];
        if (f >= n) return k;
        const uint64_t len = D[f + 1] - D[f];
        rg[3 * k] = D[f]; rg[3 * k + 1] = len; rg[3 * k + 2] = dstOffsets ? dstOffsets[k] : at;
        at += len;
    }
    return count;
}

// ------------------------------------------------------------------------------------------------ ranges
// The frames f0 .. f1 that cover a range are ONE decode batch of the `count` of them that hold content. A frame wholly inside the range decodes into its place
// in the caller's buffer; f0 and f1 where the range cuts them decode into `edge` and the covered part is copied. The batch call takes one base address and
// offsets from it: the base is the lower of the two buffers' addresses (dstBase), so every offset is a plain distance.
struct ZskRangeArgs {
    const uint64_t* cOff; const uint64_t* dOff; const uint64_t* place;     // [n + 1] each: the open call's scans (compressed / decompressed offsets, place among the frames with content)
    const uint8_t* table; uint32_t entry, checksum;                        // the entries in the stream
    uint32_t f0, f1, count;
    uint64_t offset, length;                                               // the range, in content bytes
    uint8_t* dst; uint8_t* edge; uint8_t* dstBase;
    uint64_t* srcSegs; uint64_t* dstSegs; uint32_t* frameOf;               // [count]
    const uint64_t* outSizes; int32_t* status;                             // [count]: what zhip_decompress_batch_device wrote
    uint32_t* worst;                                                       // ~(lowest failing batch item), 0 = none (zeroed before the verifier)
    int32_t* outStatus;
};
// where frame f's content is decoded to, and whether that is the edge buffer (f0's part first, f1's behind it)
ZH_DEV uint8_t* zsk_frame_home(const ZskRangeArgs& a, uint32_t f, bool* partial)
{
    const uint64_t at = a.dOff[f], end = a.dOff[f + 1];
    *partial = at < a.offset || end > a.offset + a.length;
    if (!*partial) return a.dst + (at - a.offset);
    if (f == a.f0) return a.edge;
    const uint64_t d0 = a.dOff[a.f0], e0 = a.dOff[a.f0 + 1];
    return a.edge + (d0 < a.offset || e0 > a.offset + a.length ? e0 - d0 : 0);
}
ZH_DEV void zsk_range_segs_body(const ZskRangeArgs& a)
{
    const uint64_t nf = (uint64_t)a.f1 - a.f0 + 1;
    for (uint64_t j = (uint64_t)zh_block() * 64 + zh_lane(); j < nf; j += (uint64_t)zh_nblocks() * 64) {
        const uint32_t f = a.f0 + (uint32_t)j;
        const uint64_t size = a.dOff[f + 1] - a.dOff[f];
        if (!size) continue;                                                // a skippable or an empty frame: never the decoder's
        const uint64_t k = a.place[f] - a.place[a.f0];
        bool partial; uint8_t* const home = zsk_frame_home(a, f, &partial);
        a.srcSegs[2 * k] = a.cOff[f]; a.srcSegs[2 * k + 1] = a.cOff[f + 1] - a.cOff[f];
        a.dstSegs[2 * k] = (uint64_t)(home - a.dstBase); a.dstSegs[2 * k + 1] = size;
        a.frameOf[k] = f;
    }
}
// a lane per decoded frame: the size it came out at against its entry's (20), its content's XXH64 against its entry's (22)
ZH_DEV void zsk_range_verify_body(const ZskRangeArgs& a)
{
    for (uint64_t k = (uint64_t)zh_block() * 64 + zh_lane(); k < a.count; k += (uint64_t)zh_nblocks() * 64) {
        int32_t code = a.status[k];
        if (!code) {
            const uint32_t f = a.frameOf[k];
            const uint64_t size = a.dOff[f + 1] - a.dOff[f];
            if (a.outSizes[k] != size) code = ZSK_ERR_CORRUPT;
            else if (a.checksum) {
                const uint32_t want = zh_ld32(a.table + (uint64_t)f * a.entry + 8);
                if ((uint32_t)ze_xxh64(a.dstBase + a.dstSegs[2 * k], (uint32_t)size) != want) code = ZSK_ERR_CHECKSUM;
            }
            if (code) a.status[k] = code;
        }
        if (code) zh_atomic_max(a.worst, ~(uint32_t)k);
    }
}
// the covered parts of the edge frames into the caller's buffer, 16 bytes per lane; lane 0 of the grid also writes the range's status
ZH_DEV void zsk_range_finish_body(const ZskRangeArgs& a)
{
    if (zh_block() == 0 && zh_lane() == 0) {
        const uint32_t w = *a.worst;
        a.outStatus[0] = w ? a.status[~w] : 0; a.outStatus[1] = w ? (int32_t)a.frameOf[~w] : 0;
    }
    const uint64_t rangeEnd = a.offset + a.length;
    for (int side = 0; side < 2; side++) {
        const uint32_t f = side ? a.f1 : a.f0;
        if (side && a.f1 == a.f0) break;
        const uint64_t at = a.dOff[f], end = a.dOff[f + 1];
        if (at == end) continue;
        bool partial; const uint8_t* const home = zsk_frame_home(a, f, &partial);
        if (!partial) continue;
        const uint64_t from = at > a.offset ? at : a.offset, to = end < rangeEnd ? end : rangeEnd;       // the covered part, in content bytes
        if (from >= to) continue;
        const uint8_t* const s = home + (from - at); uint8_t* const d = a.dst + (from - a.offset);
        const uint64_t len = to - from, whole = len & ~(uint64_t)15;
        const uint64_t lane = (uint64_t)zh_block() * 64 + zh_lane(), lanes = (uint64_t)zh_nblocks() * 64;
        for (uint64_t j = lane * 16; j < whole; j += lanes * 16) { const zh_v16 v = zh_ld128(s + j); zh_st64(d + j, v.lo); zh_st64(d + j + 8, v.hi); }
        if (lane < len - whole) d[whole + lane] = s[whole + lane];
    }
}

// ------------------------------------------------------------------------------------------------ many ranges in one decode batch
// R ranges -> every frame with content that at least one of them touches is ONE item of the decode batch. A frame that lies wholly inside exactly one range
// and is touched by no other decodes into its place in the caller's buffer; every other frame (cut by a range's edge, or needed by two or more ranges) decodes
// into the handle's scratch, slots in ascending frame order, and contiguous copies ("jobs") move the covered parts to the ranges that need them. Where the
// scratch frames exceed the handle's limit the item list is cut at frame boundaries into passes -- each a batch of its own that reuses the scratch from 0.
// The plan is a host function over the open call's dOff / place columns: O(R log R) + segments + jobs, never O(frames of the stream).
#define ZSK_MAX_RANGES 0x8000000u            // 2^27
#define ZSK_SCRATCH_DEFAULT 0x40000000ull    // 1 GiB: holds the largest frame the format allows
struct ZskGatherRange { uint64_t offset, length, dstOffset; uint32_t f0, f1; };      // f0 .. f1: the frames of the first and last byte (length 0: f0 = 1, f1 = 0)
// frames first .. first + frames - 1 share a home: content byte dOff[first] lies at `home` from d_dst (inPlace) or from the scratch; framePrefix counts the
// pass's frames in front (a lane of the segment builder bisects it), item is the batch item of the segment's first frame with content, counted over the call
struct ZskGatherSeg { uint32_t first, frames, framePrefix, item; uint64_t home; uint32_t inPlace, pass; };
struct ZskGatherJob { uint64_t src, dst, bytes, tilePrefix; };                       // scratch + src -> d_dst + dst; tilePrefix: the pass's copy tiles in front
struct ZskGatherPass { uint32_t seg0, seg1, item0, item1, job0, job1, frames; uint64_t scratch, tiles; };

struct ZskGatherPlan {
    std::vector<ZskGatherRange> ranges; std::vector<ZskGatherSeg> segs; std::vector<ZskGatherJob> jobs; std::vector<ZskGatherPass> passes;
    uint64_t items = 0, inPlace = 0, scratchBytes = 0, scratchMax = 0;               // scratchMax: the largest pass's scratch == what the handle must hold
};
// the checks in front of the plan; rg = [R][3] (offset, length, dstOffset). 0, or 1: range *bad ends beyond the content (or wraps), 2: its destination ends
// beyond the capacity (or wraps), 3: its destination overlaps that of range *other. The overlap check is a sort by dstOffset.
static inline int zsk_gather_check(const uint64_t* rg, size_t R, uint64_t contentSize, uint64_t dstCapacity, size_t* bad, size_t* other)
{
    for (size_t r = 0; r < R; r++) {
        const uint64_t off = rg[3 * r], len = rg[3 * r + 1], at = rg[3 * r + 2];
        *bad = r; *other = r;
        if (off + len < off || off + len > contentSize) return 1;
        if (at + len < at || at + len > dstCapacity) return 2;
    }
    std::vector<size_t> order;
    for (size_t r = 0; r < R; r++) if (rg[3 * r + 1]) order.push_back(r);
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return rg[3 * x + 2] != rg[3 * y + 2] ? rg[3 * x + 2] < rg[3 * y + 2] : x < y; });
    for (size_t i = 1; i < order.size(); i++) {
        const size_t p = order[i - 1], q = order[i];
        if (rg[3 * p + 2] + rg[3 * p + 1] > rg[3 * q + 2]) { *bad = p < q ? q : p; *other = p < q ? p : q; return 3; }
    }
    return 0;
}
// D = dOff, P = place: [n + 1] each. The ranges have passed zsk_gather_check. limit 0 = ZSK_SCRATCH_DEFAULT.
static inline void zsk_gather_plan(const uint64_t* D, const uint64_t* P, uint32_t n, const uint64_t* rg, size_t R, uint64_t limit, ZskGatherPlan* out)
{
    if (!limit) limit = ZSK_SCRATCH_DEFAULT;
    *out = ZskGatherPlan();
    out->ranges.resize(R);
    // 1. every range's first and last frame (both hold content: upper_bound steps over frames of none), and its intervals: the frames it covers whole,
    //    and each frame it cuts as an interval of its own
    struct Ev { uint32_t pos; int32_t d, partial; uint64_t r; };
    std::vector<Ev> ev;
    for (size_t r = 0; r < R; r++) {
        ZskGatherRange& g = out->ranges[r];
        g.offset = rg[3 * r]; g.length = rg[3 * r + 1]; g.dstOffset = rg[3 * r + 2]; g.f0 = 1; g.f1 = 0;
        if (!g.length) continue;
        const uint64_t end = g.offset + g.length;
        g.f0 = (uint32_t)(std::upper_bound(D, D + n + 1, g.offset) - D - 1); g.f1 = (uint32_t)(std::upper_bound(D, D + n + 1, end - 1) - D - 1);
        const uint32_t cut0 = D[g.f0] < g.offset || D[g.f0 + 1] > end ? 1u : 0u, cut1 = g.f1 != g.f0 && D[g.f1 + 1] > end ? 1u : 0u;
        if (cut0) { ev.push_back({g.f0, 1, 1, r}); ev.push_back({g.f0 + 1, -1, 1, r}); }
        if (cut1) { ev.push_back({g.f1, 1, 1, r}); ev.push_back({g.f1 + 1, -1, 1, r}); }
        if (g.f0 + cut0 < g.f1 + 1 - cut1) { ev.push_back({g.f0 + cut0, 1, 0, r}); ev.push_back({g.f1 + 1 - cut1, -1, 0, r}); }
    }
    std::sort(ev.begin(), ev.end(), [](const Ev& x, const Ev& y) { return x.pos < y.pos; });
    // 2. the sweep: runs of frames under one state -- in place (one interval over them, and that one whole: `sum` is then its range) or scratch. Neighbouring
    //    runs of the same state are one run (scratch slots ascend with frames, so neighbouring scratch runs are contiguous there too)
    struct Run { uint32_t a, b; uint32_t inPlace; uint64_t owner; };
    std::vector<Run> runs;
    {
        int64_t cnt = 0, part = 0; uint64_t sum = 0; uint32_t prev = 0;
        for (size_t i = 0; i < ev.size();) {
            const uint32_t pos = ev[i].pos;
            if (cnt > 0 && pos > prev) {
                const uint32_t inPlace = cnt == 1 && part == 0 ? 1u : 0u;
                if (!runs.empty() && runs.back().b == prev && runs.back().inPlace == inPlace && (!inPlace || runs.back().owner == sum)) runs.back().b = pos;
                else runs.push_back({prev, pos, inPlace, sum});
            }
            for (; i < ev.size() && ev[i].pos == pos; i++) { cnt += ev[i].d; part += ev[i].d * ev[i].partial; sum += (uint64_t)(int64_t)ev[i].d * ev[i].r; }
            prev = pos;
        }
    }
    // 3. passes: the runs in frame order, a scratch run cut where the pass's scratch would exceed the limit (a frame above the limit alone in its pass's scratch)
    ZskGatherPass cur; memset(&cur, 0, sizeof cur);
    uint64_t used = 0; uint32_t items = 0;
    auto closePass = [&]() {
        cur.seg1 = (uint32_t)out->segs.size(); cur.item1 = items; cur.scratch = used;
        if (cur.seg1 > cur.seg0) { out->passes.push_back(cur); if (used > out->scratchMax) out->scratchMax = used; }
        memset(&cur, 0, sizeof cur); cur.seg0 = (uint32_t)out->segs.size(); cur.item0 = items; used = 0;
    };
    auto pushSeg = [&](uint32_t a, uint32_t b, uint64_t home, uint32_t inPlace) {
        out->segs.push_back({a, b - a, cur.frames, items, home, inPlace, (uint32_t)out->passes.size()});
        cur.frames += b - a; items += (uint32_t)(P[b] - P[a]);
    };
    for (const Run& run : runs) {
        if (run.inPlace) {
            const ZskGatherRange& g = out->ranges[run.owner];
            pushSeg(run.a, run.b, g.dstOffset + (D[run.a] - g.offset), 1);
            out->inPlace += P[run.b] - P[run.a];
            continue;
        }
        for (uint32_t a = run.a; a < run.b;) {
            const uint64_t room = used < limit ? limit - used : 0;
            uint32_t e = (uint32_t)(std::upper_bound(D + a + 1, D + run.b + 1, D[a] + room) - D - 1);          // the last e in [a, b] with D[e] - D[a] <= room
            if (e == a) { if (used) { closePass(); continue; } e = a + 1; }
            pushSeg(a, e, used, 0);
            used += D[e] - D[a]; out->scratchBytes += D[e] - D[a];
            a = e;
        }
    }
    closePass();
    out->items = items;
    // 4. copy jobs: per range and scratch segment it touches (a maximal run of consecutive scratch frames of one pass), clipped to the range
    std::vector<ZskGatherJob> jobs; std::vector<uint32_t> passOf;
    for (size_t r = 0; r < R; r++) {
        const ZskGatherRange& g = out->ranges[r];
        if (!g.length) continue;
        const uint64_t end = g.offset + g.length;
        size_t s = (size_t)(std::upper_bound(out->segs.begin(), out->segs.end(), g.f0, [](uint32_t f, const ZskGatherSeg& x) { return f < x.first; }) - out->segs.begin()) - 1;
        for (; s < out->segs.size() && out->segs[s].first <= g.f1; s++) {
            const ZskGatherSeg& x = out->segs[s];
            if (x.inPlace) continue;
            const uint64_t at = D[x.first], to0 = D[x.first + x.frames];
            const uint64_t from = at > g.offset ? at : g.offset, to = to0 < end ? to0 : end;
            if (from >= to) continue;
            jobs.push_back({x.home + (from - at), g.dstOffset + (from - g.offset), to - from, 0}); passOf.push_back(x.pass);
        }
    }
    std::vector<uint32_t> at(out->passes.size() + 1, 0);
    for (uint32_t p : passOf) at[p + 1]++;
    for (size_t p = 0; p < out->passes.size(); p++) { at[p + 1] += at[p]; out->passes[p].job0 = at[p]; out->passes[p].job1 = at[p + 1]; }
    out->jobs.resize(jobs.size());
    for (size_t j = 0; j < jobs.size(); j++) out->jobs[at[passOf[j]]++] = jobs[j];
    for (ZskGatherPass& p : out->passes) {
        uint64_t tiles = 0;
        for (uint32_t j = p.job0; j < p.job1; j++) { out->jobs[j].tilePrefix = tiles; tiles += (out->jobs[j].bytes + ZSK_COPY_TILE - 1) / ZSK_COPY_TILE; }
        p.tiles = tiles;
    }
}

// one pass's launches read this; the item arrays and `worst` are the whole call's (items are counted over the call, so a range's lowest failing item is its
// lowest failing frame whatever pass decoded it)
struct ZskGatherArgs {
    const uint64_t* cOff; const uint64_t* dOff; const uint64_t* place;
    const uint8_t* table; uint32_t entry, checksum;
    const ZskGatherRange* ranges; uint32_t nRanges;
    const ZskGatherSeg* segs; uint32_t nSegs, frames;                      // the pass's
    const ZskGatherJob* jobs; uint32_t nJobs; uint64_t tiles;              // the pass's
    uint32_t item0, count;                                                 // the pass's items
    uint8_t* dst; uint8_t* scratch; uint8_t* dstBase;
    uint64_t* srcSegs; uint64_t* dstSegs; uint32_t* frameOf; const uint64_t* outSizes; int32_t* status;
    uint32_t* worst;                                                       // [nRanges]: ~(lowest failing item among the frames the range needs), 0 = none
    int32_t* outStatus; uint32_t last;                                     // last: this pass's finish also writes the status pairs
};
// a lane per frame of the pass's segments: its batch item
ZH_DEV void zsk_gather_segs_body(const ZskGatherArgs& a)
{
    for (uint64_t j = (uint64_t)zh_block() * 64 + zh_lane(); j < a.frames; j += (uint64_t)zh_nblocks() * 64) {
        uint32_t lo = 0, hi = a.nSegs;                                      // the last segment whose framePrefix <= j
        while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (a.segs[mid].framePrefix <= j) lo = mid; else hi = mid; }
        const ZskGatherSeg s = a.segs[lo];
        const uint32_t f = s.first + ((uint32_t)j - s.framePrefix);
        const uint64_t size = a.dOff[f + 1] - a.dOff[f];
        if (!size) continue;                                                // a skippable or an empty frame: never the decoder's
        const uint64_t k = s.item + (a.place[f] - a.place[s.first]);
        uint8_t* const home = (s.inPlace ? a.dst : a.scratch) + s.home + (a.dOff[f] - a.dOff[s.first]);
        a.srcSegs[2 * k] = a.cOff[f]; a.srcSegs[2 * k + 1] = a.cOff[f + 1] - a.cOff[f];
        a.dstSegs[2 * k] = (uint64_t)(home - a.dstBase); a.dstSegs[2 * k + 1] = size;
        a.frameOf[k] = f;
    }
}
// a lane per item of the pass, as zsk_range_verify_body; a failing item is folded into every range that needs its frame (the rare path: the lane walks them)
ZH_DEV void zsk_gather_verify_body(const ZskGatherArgs& a)
{
    for (uint64_t i = (uint64_t)zh_block() * 64 + zh_lane(); i < a.count; i += (uint64_t)zh_nblocks() * 64) {
        const uint64_t k = a.item0 + i;
        int32_t code = a.status[k];
        const uint32_t f = a.frameOf[k];
        if (!code) {
            const uint64_t size = a.dOff[f + 1] - a.dOff[f];
            if (a.outSizes[k] != size) code = ZSK_ERR_CORRUPT;
            else if (a.checksum) {
                const uint32_t want = zh_ld32(a.table + (uint64_t)f * a.entry + 8);
                if ((uint32_t)ze_xxh64(a.dstBase + a.dstSegs[2 * k], (uint32_t)size) != want) code = ZSK_ERR_CHECKSUM;
            }
            if (code) a.status[k] = code;
        }
        if (code) for (uint32_t r = 0; r < a.nRanges; r++) if (a.ranges[r].f0 <= f && f <= a.ranges[r].f1) zh_atomic_max(a.worst + r, ~(uint32_t)k);
    }
}
// the pass's copy jobs, a workgroup per ZSK_COPY_TILE bytes (it bisects the jobs' tile prefix), 16 bytes per lane; behind the last pass a lane per range
// writes the range's pair and workgroup 0 the overall one: the lowest range that failed
ZH_DEV void zsk_gather_finish_body(const ZskGatherArgs& a)
{
    for (uint64_t t = zh_block(); t < a.tiles; t += zh_nblocks()) {
        uint32_t lo = 0, hi = a.nJobs;
        while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (a.jobs[mid].tilePrefix <= t) lo = mid; else hi = mid; }
        const ZskGatherJob job = a.jobs[lo];
        const uint64_t off = (t - job.tilePrefix) * ZSK_COPY_TILE, left = job.bytes - off;
        const uint32_t bytes = left < ZSK_COPY_TILE ? (uint32_t)left : ZSK_COPY_TILE, whole = bytes & ~15u;
        const uint8_t* const s = a.scratch + job.src + off; uint8_t* const d = a.dst + job.dst + off;
        for (uint32_t j = zh_lane() * 16; j < whole; j += 64 * 16) { const zh_v16 v = zh_ld128(s + j); zh_st64(d + j, v.lo); zh_st64(d + j + 8, v.hi); }
        if (zh_lane() < bytes - whole) d[whole + zh_lane()] = s[whole + zh_lane()];
    }
    if (!a.last) return;
    for (uint64_t r = (uint64_t)zh_block() * 64 + zh_lane(); r < a.nRanges; r += (uint64_t)zh_nblocks() * 64) {
        const uint32_t w = a.worst[r];
        a.outStatus[2 + 2 * r] = w ? a.status[~w] : 0; a.outStatus[3 + 2 * r] = w ? (int32_t)a.frameOf[~w] : 0;
    }
    if (zh_block() != 0) return;
    uint64_t first = ZSK_NONE;
    for (uint32_t r = zh_lane(); r < a.nRanges; r += 64) if (a.worst[r] && first == ZSK_NONE) first = r;
    first = zsk_wave_min64(first);
    if (zh_lane() == 0) { a.outStatus[0] = first != ZSK_NONE ? a.status[~a.worst[first]] : 0; a.outStatus[1] = first != ZSK_NONE ? (int32_t)first : 0; }
}

// ------------------------------------------------------------------------------------------------ edit: a new stream from kept frames and new records
// The new stream is nPicks frames in pick order and a table: a FRAME pick is frame `index` of the opened stream, its bytes and its table entry as they are;
// a RECORD pick is record `index` of the caller's record table, compressed by this call into its slot (the records call's front half). Nothing looks inside
// a frame. A lane per pick writes its size and status; the scan in mode 0 and zsk_verdict_body over the picks give the offsets, the stream size, the status
// and the go word; the scan in mode 5 gives the picks' copy tiles in front; the copy kernel moves every pick to its place, a workgroup per tile; the table
// writer follows it on the stream. In place (d_dst is the old stream's base and the picks begin with every old frame in order) the kept prefix is where
// it belongs -- the copy starts behind it -- and the new frames start where the old table started, so the old entries are read from a stash.
static_assert(ZSK_COPY_TILE == 4 * 64 * 16, "zsk_edit_copy_body moves a whole tile as four 16-byte accesses per lane");
#define ZSK_PICK_FRAME 0u
#define ZSK_PICK_RECORD 1u
struct ZskEditPick { uint32_t from, index; };
struct ZskEditArgs {
    ZskCompressArgs v;                          // zsk_verdict_body's: n = nPicks, status = pickStatus, offs, partBad, dstCapacity, streamSize, outStatus, go
    const ZskEditPick* picks;
    const uint8_t* old; const uint64_t* cOff;   // the opened stream and its compressed offsets [nFrames + 1] (NULL without one)
    const uint8_t* oldEntries;                  // its table's entries: in the stream or, in place, in the stash
    const uint8_t* src; const uint64_t* records;             // the caller's source and record table [nRecords][2]
    const uint8_t* slots; const uint64_t* slotSegs;          // where the batch put record j's frame
    const uint64_t* recSizes; const int32_t* recStatus;      // [nRecords]: what zhip_compress_batch_device wrote
    const uint32_t* pre; const int32_t* preStatus;           // the records' pre-check (NULL without records)
    uint64_t* pickSize; int32_t* pickStatus;    // [nPicks]
    const uint64_t* tileOffs;                   // [nPicks + 1]: the scan of the picks' copy tiles (mode 5)
    uint32_t firstPick;                         // the copy starts at this pick: in place the frames of the kept prefix are where they belong, and nobody walks their tiles
};
// a lane per pick: its frame's size and status
ZH_DEV void zsk_edit_sizes_body(const ZskEditArgs& e)
{
    for (uint64_t k = (uint64_t)zh_block() * 64 + zh_lane(); k < e.v.n; k += (uint64_t)zh_nblocks() * 64) {
        const ZskEditPick p = e.picks[k];
        uint64_t size; int32_t status = 0;
        if (p.from == ZSK_PICK_FRAME) size = e.cOff[p.index + 1] - e.cOff[p.index];
        else { status = e.recStatus[p.index]; size = status ? 0 : e.recSizes[p.index]; }
        e.pickSize[k] = size; e.pickStatus[k] = status;
    }
}
// one wave: zsk_verdict_body over the picks; a failed record pre-check then puts its status over the verdict (the batch compressed the harmless form)
ZH_DEV void zsk_edit_verdict_body(const ZskEditArgs& e)
{
    zsk_verdict_body(e.v);
    if (zh_lane() != 0 || !e.pre || *e.pre) return;
    e.v.outStatus[0] = e.preStatus[0]; e.v.outStatus[1] = e.preStatus[1];
    *e.v.streamSize = 0; *e.v.go = 0;
}
// a workgroup per ZSK_COPY_TILE bytes of a pick, over a fixed grid (the tile count is the device's): it bisects the tile prefix for its pick and copies from
// the old stream or from the record's slot, 16 bytes per lane, whatever the two addresses are modulo 16; the bytes behind the last whole 16 go one per lane.
// Only bytes [offs[k], offs[k + 1]) of the destination are written: the neighbouring picks are other workgroups'. A failed stream copies nothing.
ZH_DEV void zsk_edit_copy_body(const ZskEditArgs& e)
{
    if (!*e.v.go) return;
    const uint64_t tiles = e.tileOffs[e.v.n];
    for (uint64_t t = e.tileOffs[e.firstPick] + zh_block(); t < tiles; t += zh_nblocks()) {
        uint32_t lo = e.firstPick, hi = e.v.n;                               // the last pick whose tile prefix <= t: the picks behind it of no bytes share its prefix
        while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (e.tileOffs[mid] <= t) lo = mid; else hi = mid; }
        const ZskEditPick p = e.picks[lo];
        const uint8_t* const from = p.from == ZSK_PICK_FRAME ? e.old + e.cOff[p.index] : e.slots + e.slotSegs[2 * (uint64_t)p.index];
        uint8_t* const to = e.v.dst + e.v.offs[lo];
        const uint64_t off = (t - e.tileOffs[lo]) * ZSK_COPY_TILE, left = e.pickSize[lo] - off;
        const uint32_t bytes = left < ZSK_COPY_TILE ? (uint32_t)left : ZSK_COPY_TILE, whole = bytes & ~15u;
        const uint8_t* const s = from + off; uint8_t* const d = to + off;
        if (bytes == ZSK_COPY_TILE) {                                        // a whole tile: its four loads are in flight together
            const uint32_t j = zh_lane() * 16;
            const zh_v16 v0 = zh_ld128_nt(s + j), v1 = zh_ld128_nt(s + j + 1024), v2 = zh_ld128_nt(s + j + 2048), v3 = zh_ld128_nt(s + j + 3072);      // (read once: streaming loads)
            zh_st128(d + j, v0); zh_st128(d + j + 1024, v1); zh_st128(d + j + 2048, v2); zh_st128(d + j + 3072, v3);
            continue;
        }
        for (uint32_t j = zh_lane() * 16; j < whole; j += 64 * 16) zh_st128(d + j, zh_ld128_nt(s + j));
        if (zh_lane() < bytes - whole) d[whole + zh_lane()] = s[whole + zh_lane()];
    }
}
// a lane per pick: a kept frame's entry as it was (the checksum word included), a record's (frame size, length, XXH64 low word of its source bytes);
// lane 0 of the grid: the table frame's header and footer. A failed stream writes nothing
ZH_DEV void zsk_edit_table_body(const ZskEditArgs& e)
{
    if (!*e.v.go) return;
    const uint32_t entry = zsk_entry_size((int)e.v.checksum);
    uint8_t* const table = e.v.dst + e.v.offs[e.v.n];
    for (uint64_t k = (uint64_t)zh_block() * 64 + zh_lane(); k < e.v.n; k += (uint64_t)zh_nblocks() * 64) {
        const ZskEditPick p = e.picks[k];
        uint8_t* const w = table + ZSK_HEADER + k * entry;
        if (p.from == ZSK_PICK_FRAME) {
            const uint8_t* const was = e.oldEntries + (uint64_t)p.index * entry;
            for (uint32_t j = 0; j < entry; j += 4) zh_st32(w + j, zh_ld32(was + j));
        } else {
            const uint64_t at = e.records[2 * (uint64_t)p.index]; const uint32_t len = (uint32_t)e.records[2 * (uint64_t)p.index + 1];
            zh_st32(w, (uint32_t)e.pickSize[k]); zh_st32(w + 4, len);
            if (e.v.checksum) zh_st32(w + 8, (uint32_t)ze_xxh64(e.src + at, len));
        }
    }
    if (zh_block() != 0 || zh_lane() != 0) return;
    uint8_t* const f = table + ZSK_HEADER + (uint64_t)e.v.n * entry;
    zh_st32(table, ZSK_SKIP_MAGIC); zh_st32(table + 4, e.v.n * entry + ZSK_FOOTER);
    zh_st32(f, e.v.n); f[4] = e.v.checksum ? 0x80 : 0; zh_st32(f + 5, ZSK_SEEK_MAGIC);
}
// the host's checks of a pick list: 0, 1 (a pick that is neither kind, or a FRAME pick without a stream), 2 (an index that is no frame / no record; *bad = its position)
static inline int zsk_edit_check(const ZskEditPick* picks, size_t nPicks, bool haveOld, uint32_t nFrames, uint64_t nRecords, size_t* bad)
{
    for (size_t k = 0; k < nPicks; k++) {
        *bad = k;
        if (picks[k].from > ZSK_PICK_RECORD || (picks[k].from == ZSK_PICK_FRAME && !haveOld)) return 1;
        if (picks[k].index >= (picks[k].from == ZSK_PICK_FRAME ? (uint64_t)nFrames : nRecords)) return 2;
    }
    return 0;
}
// the append form: the picks begin with every frame of the opened stream, in order
static inline bool zsk_edit_is_append(const ZskEditPick* picks, size_t nPicks, uint32_t nFrames)
{
    if (nPicks < nFrames) return false;
    for (uint32_t k = 0; k < nFrames; k++) if (picks[k].from != ZSK_PICK_FRAME || picks[k].index != k) return false;
    return true;
}
// worst-case bytes of the new stream: the kept frames as they are, every record at zsk_compress_bound(maxRecord) (monotonic: it covers a shorter record), the
// table. The picks have passed zsk_edit_check. C = the opened stream's compressed offsets (host)
static inline uint64_t zsk_edit_bound(const ZskEditPick* picks, size_t nPicks, const uint64_t* C, uint64_t maxRecord, int checksum)
{
    uint64_t total = zsk_table_size(nPicks, checksum);
    for (size_t k = 0; k < nPicks; k++) total += picks[k].from == ZSK_PICK_FRAME ? C[picks[k].index + 1] - C[picks[k].index] : zsk_compress_bound(maxRecord);
    return total;
}

#ifndef ZHIP_EMU
__global__ __launch_bounds__(64) void zhip_seekable_scan_reduce_kernel(ZskScanArgs a) { zsk_scan_reduce_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_scan_write_kernel(ZskScanArgs a) { zsk_scan_write_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_chunk_segs_kernel(ZskCompressArgs a) { zsk_chunk_segs_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_verdict_kernel(ZskCompressArgs a) { zsk_verdict_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_table_kernel(ZskCompressArgs a) { zsk_table_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_records_verdict_kernel(ZskRecordsArgs a) { zsk_records_verdict_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_records_segs_kernel(ZskRecordsArgs a) { zsk_records_segs_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_records_table_kernel(ZskRecordsArgs a) { zsk_records_table_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_range_segs_kernel(ZskRangeArgs a) { zsk_range_segs_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_range_verify_kernel(ZskRangeArgs a) { zsk_range_verify_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_range_finish_kernel(ZskRangeArgs a) { zsk_range_finish_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_gather_segs_kernel(ZskGatherArgs a) { zsk_gather_segs_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_gather_verify_kernel(ZskGatherArgs a) { zsk_gather_verify_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_gather_finish_kernel(ZskGatherArgs a) { zsk_gather_finish_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_edit_sizes_kernel(ZskEditArgs e) { zsk_edit_sizes_body(e); }
__global__ __launch_bounds__(64) void zhip_seekable_edit_verdict_kernel(ZskEditArgs e) { zsk_edit_verdict_body(e); }
__global__ __launch_bounds__(64) void zhip_seekable_edit_copy_kernel(ZskEditArgs e) { zsk_edit_copy_body(e); }
__global__ __launch_bounds__(64) void zhip_seekable_edit_table_kernel(ZskEditArgs e) { zsk_edit_table_body(e); }
#endif
