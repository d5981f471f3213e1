// tests/emu/emu_seekable.cpp -- the seekable-stream calls (python-zstandard_amd/csrc/zhip_seekable_calls.hpp) and kernels (zhip_seekable.hpp) on the host wave
// emulator. Test infrastructure only (tests/test_emu_seekable.py); compiled with zhemu.cpp like emu_greedy_row.cpp. Every call here IS the library's sequence:
// the shared template over the emulator's backend (emu_seekable_backend.hpp), so the layouts, the wiring, the grids and the order are the library's own.
#include "emu_seekable_backend.hpp"
#include <string.h>
#include <algorithm>
#include <vector>

// both launches of the scan alone (the unit entries); returns the lowest bad item (ZSK_NONE: none)
static uint64_t run_scan(ZskScanArgs s)
{
    const uint32_t grid = zsk_scan_shape(s.n, &s.span);
    std::vector<uint64_t> sum(grid, 0xA5A5A5A5A5A5A5A5ull), bad(grid, 0xA5A5A5A5A5A5A5A5ull);
    s.partSum = sum.data(); s.partBad = bad.data();
    zhemu::run_grid(grid, scan_reduce_lane, &s);
    zhemu::run_grid(grid, scan_write_lane, &s);
    return *std::min_element(bad.begin(), bad.end());
}

// the kernel's own tile sizes: lanes per workgroup, items per workgroup, items of one full grid pass
extern "C" void emu_seekable_tiles(uint32_t* out) { out[0] = ZSK_SCAN_LANES; out[1] = ZSK_SCAN_TILE; out[2] = ZSK_SCAN_GRID * ZSK_SCAN_TILE; }

// mode 0 (what the compress call runs): offs has n + 1 cells, the last one receives the total
extern "C" uint64_t emu_seekable_scan(const uint64_t* sizes, const int32_t* status, uint32_t n, uint64_t* offs)
{
    ZskScanArgs s; memset(&s, 0, sizeof s);
    s.in = (const uint8_t*)sizes; s.status = status; s.mode = 0; s.n = n; s.offs = offs;
    return run_scan(s);
}

// the compress call with the batch replaced by the given outSizes / status; the frames' bytes are not written (sizesOnly). dst holds dstCapacity bytes;
// srcSegs / slotSegs [n][2] receive the chunk segments, status what the table writer left. Returns the stream size (0: failed or refused), outStatus[2] the status.
extern "C" uint64_t emu_seekable_table(const uint8_t* src, uint64_t srcSize, uint32_t frameSize, uint32_t checksum, const uint64_t* outSizes, int32_t* status,
                                       uint8_t* dst, uint64_t dstCapacity, uint64_t* srcSegs, uint64_t* slotSegs, int32_t* outStatus)
{
    EmuBackend b; b.givenSizes = outSizes; b.givenStatus = status; b.srcSize = srcSize; b.sizesOnly = true;
    uint64_t streamSize = ~0ull;
    if (zsk_compress(b, true, src, srcSize, frameSize, checksum ? ZHIP_SEEKABLE_CHECKSUM : 0, dst, dstCapacity, &streamSize, outStatus)) return 0;
    const ZskCompressArgs& a = b.sawCompress;
    if (a.n && !b.traceOnly) { memcpy(srcSegs, a.srcSegs, (size_t)a.n * 16); memcpy(slotSegs, a.slotSegs, (size_t)a.n * 16); memcpy(status, a.status, (size_t)a.n * 4); }
    return streamSize;
}

// zhip_seekable_open_device (open_stream) on a stream in host memory. Returns 0 or the zstd error code; on success info = {n, entry size, checksum flag,
// table offset, content size} and, where given, cOff / dOff / place receive the n + 1 cells of the three scans.
extern "C" int emu_seekable_validate(const uint8_t* stream, uint64_t size, uint64_t* info, uint64_t* cOff, uint64_t* dOff, uint64_t* place)
{
    Opened o;
    const int e = open_stream(stream, size, &o);
    if (e) return e;
    const size_t n = o.lay.n;
    if (info) { info[0] = n; info[1] = o.lay.entry; info[2] = (uint64_t)o.lay.checksum; info[3] = o.lay.tableOffset; info[4] = o.dOff[n]; }
    if (cOff) memcpy(cOff, o.cOff.data(), (n + 1) * 8);
    if (dOff) memcpy(dOff, o.dOff.data(), (n + 1) * 8);
    if (place) memcpy(place, o.place.data(), (n + 1) * 8);
    return 0;
}

// zhip_seekable_decompress_device with the decoder replaced by a copy: frame f "decodes" to content[dOff[f], dOff[f + 1]) -- `content` is what the test says the
// stream holds -- except frame `shortFrame` (-1: none), which comes out one byte short. dst has `length` bytes. Returns the library's code (ZHIP_ERR_SIZE_MISMATCH:
// the range is outside the content), the open's error code, or -1 where a segment lies outside its buffer; outStatus[2] the range's status; segsOut (where
// given) [count][4] = srcSeg, dstSeg relative to dst or, for a frame in the edge area, 2^63 + its offset there.
extern "C" int emu_seekable_range(const uint8_t* stream, uint64_t size, const uint8_t* content, uint64_t offset, uint64_t length, uint8_t* dst, int64_t shortFrame,
                                  int32_t* outStatus, uint64_t* segsOut, uint32_t* countOut)
{
    Opened o;
    if (int e = open_stream(stream, size, &o)) return e;
    if (countOut) *countOut = 0;
    EmuBackend& b = o.b; b.content = content; b.shortFrame = shortFrame; b.dst = dst; b.dstBytes = length; b.segsOut = segsOut;
    const int rc = zsk_range(b, true, &o, offset, length, dst, outStatus);
    if (!rc && length && countOut) *countOut = b.sawRange.count;
    return rc;
}

extern "C" uint64_t emu_seekable_bound(uint64_t srcSize, uint32_t frameSize, int checksum) { return zsk_bound(srcSize, frameSize, checksum); }
extern "C" uint64_t emu_seekable_xxh64(const uint8_t* p, uint32_t n) { return ze_xxh64(p, n); }
