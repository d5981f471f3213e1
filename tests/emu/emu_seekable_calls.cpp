// tests/emu/emu_seekable_calls.cpp -- what tests/test_emu_seekable_calls.py needs beyond the calls themselves: every layout of
// python-zstandard_amd/csrc/zhip_seekable_calls.hpp as a list of arrays, the host checks with their code and text, the last call's launch trace, the CU count and
// the record-only mode of the backend, and the whole edit call (records' front half included). Test infrastructure only.
#include "emu_seekable_edit.cpp"

extern "C" void emu_calls_mode(int numCU, int traceOnly) { g_emuNumCU = numCU; g_emuTraceOnly = traceOnly != 0; }
// the last backend's launches as (kernel, grid) pairs; returns how many pairs there were
extern "C" uint64_t emu_calls_trace(uint32_t* out, uint64_t capPairs)
{
    for (size_t i = 0; i < g_emuTrace.size() && i < 2 * capPairs; i++) out[i] = g_emuTrace[i];
    return g_emuTrace.size() / 2;
}
// the ids the trace uses: the 18 kernels in ZskKernel's order, then the compaction and the two batch calls
extern "C" void emu_calls_ids(uint32_t* out) { out[0] = ZSK_K_COUNT; out[1] = EMU_T_COMPACT; out[2] = EMU_T_COMPRESS; out[3] = EMU_T_DECOMPRESS; }

// A layout as rows of {area, offset, bytes}: every array with the length its kernel indexes, then one row per area {area, reserved bytes, ~0}.
// kind 0: fixed-size compress (n)   1: records (n)   2: the single range (count)   3: many ranges (R, S, J, count; area 0 the tables, 1 the meta area)
//      4: edit (nPicks, nRecords, nOld, inPlace, entry)   5: open (n; area 0 the prefix columns, 1 the partial areas)
extern "C" uint64_t emu_calls_layout(uint32_t kind, const uint64_t* p, uint64_t* out)
{
    uint64_t rows = 0;
    auto row = [&](uint64_t area, uint64_t off, uint64_t bytes) { out[3 * rows] = area; out[3 * rows + 1] = off; out[3 * rows + 2] = bytes; rows++; };
    const uint64_t part = (uint64_t)ZSK_SCAN_GRID * 8;
    auto records = [&](uint64_t n) {
        const ZskRecordsLayout l = zsk_records_layout((size_t)n);
        row(0, l.oSrcSegs, n * 16); row(0, l.oSlotSegs, n * 16); row(0, l.oSizes, n * 8); row(0, l.oOffs, (n + 1) * 8); row(0, l.oLenOffs, (n + 1) * 8); row(0, l.oSlotOffs, (n + 1) * 8);
        row(0, l.oPartSum, part); row(0, l.oPartBad, part); row(0, l.oPreBad, part); row(0, l.oGo, 16); row(0, l.oStatus, n * 4);
        return (uint64_t)l.metaBytes;
    };
    auto items = [&](uint64_t area, const ZskItemsLayout& l, uint64_t count, uint64_t worst) {
        row(area, l.oSrcSegs, count * 16); row(area, l.oDstSegs, count * 16); row(area, l.oSizes, count * 8); row(area, l.oFrameOf, count * 4); row(area, l.oStatus, count * 4);
        row(area, l.oWorst, worst); row(area, l.metaBytes, ~0ull);
    };
    if (kind == 0) {
        const uint64_t n = p[0]; const ZskCompressLayout l = zsk_compress_layout((size_t)n);
        row(0, l.oSrcSegs, n * 16); row(0, l.oSlotSegs, n * 16); row(0, l.oSizes, n * 8); row(0, l.oOffs, (n + 1) * 8); row(0, l.oPartSum, part); row(0, l.oPartBad, part);
        row(0, l.oGo, 16); row(0, l.oStatus, n * 4); row(0, l.metaBytes, ~0ull);
    } else if (kind == 1) { const uint64_t total = records(p[0]); row(0, total, ~0ull); }
    else if (kind == 2) items(0, zsk_items_layout((size_t)p[0], 16), p[0], 4);
    else if (kind == 3) {
        const ZskGatherLayout l = zsk_gather_layout((size_t)p[0], (size_t)p[1], (size_t)p[2], (size_t)p[3]);
        row(0, l.oRanges, p[0] * sizeof(ZskGatherRange)); row(0, l.oSegs, p[1] * sizeof(ZskGatherSeg)); row(0, l.oJobs, p[2] * sizeof(ZskGatherJob)); row(0, l.tableBytes, ~0ull);
        items(1, l.m, p[3], p[0] * 4);
    } else if (kind == 4) {
        const uint64_t n = p[0];
        const ZskEditLayout l = zsk_edit_layout((size_t)n, (size_t)p[1], (size_t)p[2], p[3] != 0, (size_t)p[4]);
        if (p[1]) records(p[1]);
        row(0, l.oPicks, n * sizeof(ZskEditPick)); row(0, l.oPickSize, n * 8); row(0, l.oOffs, (n + 1) * 8); row(0, l.oTileOffs, (n + 1) * 8); row(0, l.oPartSum, part); row(0, l.oPartBad, part);
        row(0, l.oTileBad, part); row(0, l.oGo, 16); row(0, l.oPickStatus, n * 4); row(0, l.oStash, p[3] ? p[2] * p[4] : 0); row(0, l.end, ~0ull);
    } else if (kind == 5) {
        const uint64_t n = p[0]; const ZskOpenLayout l = zsk_open_layout((size_t)n);
        for (uint64_t k = 0; k < 3; k++) row(0, k * l.col, (n + 1) * 8);
        row(0, l.prefixBytes, ~0ull);
        for (uint64_t k = 0; k < 6; k++) row(1, k * l.part, part);
        row(1, l.metaBytes, ~0ull);
    }
    return rows;
}

// the host checks: the code, and the text as zhip_last_error would return it (text holds 256 bytes)
static int put_text(int rc, const std::string& msg, char* text) { snprintf(text, 256, "%s", msg.c_str()); return rc; }
extern "C" int emu_check_compress(int pointers, uint64_t srcSize, uint32_t frameSize, int flags, char* text)
{
    std::string msg; return put_text(zsk_compress_check(pointers != 0, srcSize, frameSize, flags, msg), msg, text);
}
extern "C" int emu_check_records(int pointers, const void* records, uint64_t nRecords, uint64_t maxRecord, int flags, char* text)
{
    std::string msg; return put_text(zsk_records_check(pointers != 0, records, (size_t)nRecords, maxRecord, flags, msg), msg, text);
}
extern "C" int emu_check_range(uint64_t offset, uint64_t length, uint64_t contentSize, char* text)
{
    std::string msg; return put_text(zsk_range_check(offset, length, contentSize, msg), msg, text);
}
extern "C" int emu_check_ranges(int pointers, const uint64_t* rg, uint64_t R, uint64_t contentSize, const void* dst, uint64_t dstCapacity, char* text)
{
    std::string msg; size_t bad = 0; bool any = false;
    return put_text(zsk_ranges_check(pointers != 0, rg, (size_t)R, contentSize, dst, dstCapacity, &bad, &any, msg), msg, text);
}
// old (NULL: none) is opened first; inPlace (where given) receives the decision
extern "C" int emu_check_edit(int pointers, const uint8_t* old, uint64_t oldSize, const uint32_t* picks, uint64_t nPicks, const void* records, uint64_t nRecords, uint64_t maxRecord, int flags,
                              const void* dst, uint64_t dstCapacity, uint32_t* inPlaceOut, char* text)
{
    Opened o;
    if (old) if (int e = open_stream(old, oldSize, &o)) return -e;
    std::string msg; bool inPlace = false; size_t bad = 0;
    const int rc = zsk_edit_call_check(pointers != 0, old ? &o : nullptr, (const ZskEditPick*)picks, (size_t)nPicks, records, (size_t)nRecords, maxRecord, flags, dst, dstCapacity, &inPlace, &bad, msg);
    if (inPlaceOut) *inPlaceOut = inPlace;
    return put_text(rc, msg, text);
}

// The whole edit call, the records' front half included: the batch stand-in "compresses" record j to givenSizes[j] bytes of (31 * j + i) & 0xFF with status
// givenStatus[j]. Returns the library's code or the open's error code (negative); info[0] = the stream size, info[1] = the go word, info[2] = 1 + the first item
// whose segments the batch stand-in refused
extern "C" int emu_calls_edit(const uint8_t* old, uint64_t oldSize, const uint32_t* picks, uint64_t nPicks, const uint8_t* src, uint64_t srcSize, const uint64_t* records, uint64_t nRecords,
                              uint64_t maxContent, uint64_t maxRecord, uint32_t checksum, const uint64_t* givenSizes, const int32_t* givenStatus, uint8_t* dst, uint64_t dstCapacity,
                              int32_t* outStatus, uint64_t* info)
{
    memset(info, 0, 4 * sizeof(uint64_t));
    Opened o;
    if (old) if (int e = open_stream(old, oldSize, &o)) return -e;
    EmuBackend& b = o.b; b.givenSizes = givenSizes; b.givenStatus = givenStatus; b.srcSize = srcSize;
    uint64_t streamSize = ~0ull;
    const int rc = zsk_edit(b, true, old ? &o : nullptr, (const ZskEditPick*)picks, (size_t)nPicks, src, srcSize, (const zhip_segment*)records, (size_t)nRecords, maxContent, maxRecord,
                            checksum ? ZHIP_SEEKABLE_CHECKSUM : 0, dst, dstCapacity, &streamSize, outStatus);
    if (rc || b.traceOnly) return rc;
    info[0] = streamSize; info[1] = *b.sawEdit.v.go; info[2] = b.refused;
    return 0;
}
