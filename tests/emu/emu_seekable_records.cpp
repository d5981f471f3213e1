// tests/emu/emu_seekable_records.cpp -- one frame per record (zhip_seekable_compress_records_device) and reads by frame index (zhip_seekable_frame_offsets,
// zhip_seekable_decompress_frames_device) on the host wave emulator: the two record modes of the scan, the pre-check's verdict, the segment writer and the table
// writer of python-zstandard_amd/csrc/zhip_seekable.hpp under the library's own sequence (zsk_compress_records of zhip_seekable_calls.hpp), with the batch call
// and the compaction replaced by the backend's stand-ins that refuse a segment outside its buffer; the index -> range mapping through the library's own plan.
// Test infrastructure only (tests/test_emu_seekable_records.py, built by tests/seekable_record_cases.py). With -DZSK_RECORDS_MAIN this is a stand-alone
// program that runs the cases of a file (see main) -- the form the sanitizer build takes.
#include "emu_seekable_ranges.cpp"     // open_stream, run_scan, emu_gather_run

// one of the two record modes of the scan (3: lengths with the per-record checks, 4: slot strides); records = [n][2] (offset, length). Returns the lowest bad record
extern "C" uint64_t emu_records_scan(const uint64_t* records, uint32_t n, uint32_t mode, uint64_t limit64, uint64_t srcSize, uint64_t* offs)
{
    ZskScanArgs s; memset(&s, 0, sizeof s);
    s.in = (const uint8_t*)records + 8; s.stride = 16; s.mode = mode; s.n = n; s.limit64 = limit64; s.srcSize = srcSize; s.offs = offs;
    return run_scan(s);
}

// The whole compress call. The stand-in for the batch "compresses" item i to givenSizes[i] bytes of (31 * i + j) & 0xFF with status givenStatus[i] -- after
// it has checked that the item's source segment lies inside the source and its slot inside the slot area, which has exactly the bytes the host formula
// reserves; the stand-in for the compaction copies slot i to dst + offs[i] where status[i] is 0. dst holds dstCapacity bytes. Returns the stream size;
// outStatus[2] the status; srcSegs / slotSegs [n][2] what the batch was handed; info[0] = the slot area's bytes, info[1] = the pre-check's go word,
// info[2] = 0 or 1 + the first item whose segments the batch stand-in refused, info[3] = how many statuses were 0 behind the table writer.
extern "C" uint64_t emu_records_compress(const uint8_t* src, uint64_t srcSize, const uint64_t* records, uint32_t n, uint64_t maxContent, uint64_t maxRecord, uint32_t checksum,
                                         const uint64_t* givenSizes, const int32_t* givenStatus, uint8_t* dst, uint64_t dstCapacity, uint64_t* srcSegs, uint64_t* slotSegs,
                                         int32_t* outStatus, uint64_t* info)
{
    memset(info, 0, 4 * sizeof(uint64_t));
    EmuBackend b; b.givenSizes = givenSizes; b.givenStatus = givenStatus; b.srcSize = srcSize;
    uint64_t streamSize = ~0ull;
    if (zsk_compress_records(b, true, src, srcSize, (const zhip_segment*)records, n, maxContent, maxRecord, checksum ? ZHIP_SEEKABLE_CHECKSUM : 0, dst, dstCapacity, &streamSize, outStatus)) return ~0ull;
    info[0] = b.areas[ZSK_A_SK_SLOTS].bytes; info[2] = b.refused; info[3] = b.copied;
    if (b.traceOnly) return streamSize;
    info[1] = *b.sawRecords.pre;
    if (n) { memcpy(srcSegs, b.sawRecords.srcSegs, (size_t)n * 16); memcpy(slotSegs, b.sawRecords.slotSegs, (size_t)n * 16); }
    return streamSize;
}

extern "C" uint64_t emu_records_bound(uint64_t maxContent, uint64_t n, int checksum) { return zsk_records_bound(maxContent, n, checksum); }

// zhip_seekable_frame_offsets on a stream in host memory: 0, ZHIP_ERR_SIZE_MISMATCH or the open's error code
extern "C" int emu_frame_offsets(const uint8_t* stream, uint64_t size, uint32_t first, uint32_t count, uint64_t* out)
{
    Opened o;
    if (int e = open_stream(stream, size, &o)) return e;
    return zsk_frame_offsets(o.dOff.data(), o.lay.n, first, count, out) ? 0 : ZHIP_ERR_SIZE_MISMATCH;
}

// zhip_seekable_decompress_frames_device with the decoder replaced by a copy (emu_gather_run): the indices become ranges -- rgOut (where given) [nFrames][3] --
// and the many-ranges path runs them. Returns what emu_gather_run returns, or ZHIP_ERR_SIZE_MISMATCH with stats[7] = the position of an index that is no frame of the table
extern "C" int emu_frames_run(const uint8_t* stream, uint64_t size, const uint8_t* content, const uint32_t* frames, uint64_t nFrames, const uint64_t* dstOffsets, uint8_t* dst,
                              uint64_t dstCapacity, uint64_t limit, int32_t* outStatus, uint64_t* stats, uint64_t* rgOut, uint64_t* itemsOut, uint64_t itemCap)
{
    Opened o;
    if (int e = open_stream(stream, size, &o)) return e;
    memset(stats, 0, 8 * sizeof(uint64_t));
    std::vector<uint64_t> rg(3 * (size_t)nFrames + 3);
    const size_t bad = zsk_frames_to_ranges(o.dOff.data(), o.lay.n, frames, (size_t)nFrames, dstOffsets, rg.data());
    if (bad != nFrames) { stats[7] = bad; return ZHIP_ERR_SIZE_MISMATCH; }
    if (rgOut) memcpy(rgOut, rg.data(), 3 * (size_t)nFrames * 8);
    return emu_gather_run(stream, size, content, rg.data(), nFrames, dst, dstCapacity, limit, -1, -1, 0, outStatus, stats, itemsOut, itemCap);
}

#ifdef ZSK_RECORDS_MAIN
// emu_seekable_records <file>: the cases of the file back to back, little-endian, every buffer of exactly the size the call is given.
//   {u64 1, u64 srcSize, src, u64 n, records [n][2], u64 maxContent, u64 maxRecord, u64 checksum, sizes [n], u64 dstCapacity, u64 wantCode, u64 wantIndex}
//       the compress call: the status is {wantCode, wantIndex}; a stream that succeeds holds the stand-in's frames and a table whose entries are the records'
//       lengths (and checksums); one that fails leaves dst as it was; the batch stand-in refused no segment
//   {u64 2, u64 streamSize, stream, u64 contentSize, content, u64 n, u32 frames [n], u64 limit}
//       the read by index, back to back: every status is 0 and every record holds its frame's content
// Exit 0: every case held.
static bool rd(FILE* f, void* p, size_t n) { return !n || fread(p, 1, n, f) == n; }
static bool rd_blob(FILE* f, std::vector<uint8_t>* v) { uint64_t n; if (!rd(f, &n, 8)) return false; v->assign((size_t)n, 0); return rd(f, v->data(), v->size()); }
int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s <cases>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int cases = 0;
    for (uint64_t kind; fread(&kind, 8, 1, f) == 1; cases++) {
        if (kind == 1) {
            std::vector<uint8_t> src; uint64_t n = 0, t[3], w[3];
            if (!rd_blob(f, &src) || !rd(f, &n, 8)) return 2;
            std::vector<uint64_t> records(2 * (size_t)n), sizes((size_t)n), srcSegs(2 * (size_t)n), slotSegs(2 * (size_t)n);
            if (!rd(f, records.data(), records.size() * 8) || !rd(f, t, 24) || !rd(f, sizes.data(), sizes.size() * 8) || !rd(f, w, 24)) return 2;
            std::vector<int32_t> given((size_t)n, 0);
            std::vector<uint8_t> dst((size_t)w[0], 0x5A);
            int32_t status[2] = {-1, -1}; uint64_t info[4];
            const uint64_t size = emu_records_compress(src.data(), src.size(), records.data(), (uint32_t)n, t[0], t[1], (uint32_t)t[2], sizes.data(), given.data(), dst.data(), w[0],
                                                       srcSegs.data(), slotSegs.data(), status, info);
            if (info[2]) { fprintf(stderr, "case %d: the batch was handed a segment outside its buffer (item %llu)\n", cases, (unsigned long long)info[2] - 1); return 1; }
            if ((uint64_t)status[0] != w[1] || (uint64_t)status[1] != w[2]) { fprintf(stderr, "case %d: status {%d, %d}\n", cases, status[0], status[1]); return 1; }
            if (status[0]) {
                if (size) { fprintf(stderr, "case %d: a failed stream has a size\n", cases); return 1; }
                for (uint8_t b : dst) if (b != 0x5A) { fprintf(stderr, "case %d: a failed stream wrote\n", cases); return 1; }
                continue;
            }
            Opened o;
            if (size > dst.size() || open_stream(dst.data(), size, &o) || o.lay.n != n) { fprintf(stderr, "case %d: the stream does not open\n", cases); return 1; }
            for (size_t i = 0; i < (size_t)n; i++) {
                const uint8_t* e = dst.data() + o.lay.tableOffset + ZSK_HEADER + i * o.lay.entry;
                bool ok = zsk_rd32(e) == sizes[i] && zsk_rd32(e + 4) == records[2 * i + 1];
                if (ok && t[2]) ok = zsk_rd32(e + 8) == (uint32_t)ze_xxh64(src.data() + records[2 * i], (uint32_t)records[2 * i + 1]);
                for (uint64_t j = 0; ok && j < sizes[i]; j++) ok = dst[(size_t)(o.cOff[i] + j)] == (uint8_t)(31 * i + j);
                if (!ok) { fprintf(stderr, "case %d: record %zu\n", cases, i); return 1; }
            }
        } else if (kind == 2) {
            std::vector<uint8_t> stream, content; uint64_t n = 0, limit = 0;
            if (!rd_blob(f, &stream) || !rd_blob(f, &content) || !rd(f, &n, 8)) return 2;
            std::vector<uint32_t> frames((size_t)n);
            if (!rd(f, frames.data(), frames.size() * 4) || !rd(f, &limit, 8)) return 2;
            Opened o;
            if (open_stream(stream.data(), stream.size(), &o)) return 2;
            uint64_t need = 0;
            for (uint32_t x : frames) if (x < o.lay.n) need += o.dOff[x + 1] - o.dOff[x];
            std::vector<uint8_t> dst((size_t)need, 0x5A);
            std::vector<int32_t> status(2 + 2 * (size_t)n, -1);
            std::vector<uint64_t> rg(3 * (size_t)n);
            uint64_t stats[8];
            const int rc = emu_frames_run(stream.data(), stream.size(), content.data(), frames.data(), n, nullptr, dst.data(), need, limit, status.data(), stats, rg.data(), nullptr, 0);
            if (rc) { fprintf(stderr, "case %d: the call returned %d\n", cases, rc); return 1; }
            for (int32_t s : status) if (s) { fprintf(stderr, "case %d: a status is %d\n", cases, s); return 1; }
            for (size_t k = 0; k < (size_t)n; k++)
                if (rg[3 * k + 1] && memcmp(dst.data() + rg[3 * k + 2], content.data() + rg[3 * k], (size_t)rg[3 * k + 1])) { fprintf(stderr, "case %d: position %zu differs\n", cases, k); return 1; }
        } else return 2;
    }
    fclose(f);
    printf("%d cases\n", cases);
    return cases ? 0 : 2;
}
#endif
