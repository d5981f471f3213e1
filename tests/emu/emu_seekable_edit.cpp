// tests/emu/emu_seekable_edit.cpp -- the edit call (zhip_seekable_edit_device) on the host wave emulator: the library's own host checks (zsk_edit_check,
// zsk_edit_is_append, zsk_edit_bound) and the bodies of its kernels -- pick sizes, the two scans, the verdict, the tiled copy, the table writer -- of
// python-zstandard_amd/csrc/zhip_seekable.hpp, under the library's own per-pick sequence (zsk_edit_picks of zhip_seekable_calls.hpp). The kernels do not look inside
// a frame, so any bytes serve as frames; the records' front half is the test's: it says what the batch wrote (sizes, statuses, slots) and what the pre-check found.
// Test infrastructure only (tests/test_emu_seekable_edit.py, built by tests/seekable_edit_cases.py). With -DZSK_EDIT_MAIN this is a stand-alone program that
// runs the cases of a file (see main) -- the form the sanitizer build takes.
#include "emu_seekable_records.cpp"     // open_stream, run_scan

// the copy tile's bytes, and the copy's grid at its cap (the library's formula for the emulator's one CU)
extern "C" void emu_edit_tiles(uint32_t* out) { out[0] = ZSK_COPY_TILE; out[1] = zsk_edit_copy_grid(1, ~0ull, 0); }

// mode 5 of the scan alone: the copy tiles in front of every item
extern "C" void emu_edit_tile_scan(const uint64_t* sizes, uint32_t n, uint64_t* offs)
{
    ZskScanArgs s; memset(&s, 0, sizeof s);
    s.in = (const uint8_t*)sizes; s.mode = 5; s.n = n; s.offs = offs;
    run_scan(s);
}

extern "C" uint64_t emu_edit_bound(const uint8_t* old, uint64_t oldSize, const uint32_t* picks, uint64_t nPicks, uint64_t maxRecord, int checksum)
{
    Opened o;
    if (old && open_stream(old, oldSize, &o)) return 0;
    if (old && o.lay.checksum != checksum) return 0;
    size_t bad = 0;
    if (nPicks > ZSK_MAX_FRAMES || maxRecord > ZSK_MAX_CONTENT || zsk_edit_check((const ZskEditPick*)picks, (size_t)nPicks, old != nullptr, old ? o.lay.n : 0, ZSK_MAX_FRAMES, &bad)) return 0;
    return zsk_edit_bound((const ZskEditPick*)picks, (size_t)nPicks, old ? o.cOff.data() : nullptr, maxRecord, checksum);
}

// The call behind the records' front half. old / oldSize: the opened stream (NULL: none; in place it IS dst). picks [nPicks][2] = (from, index). The records:
// src and records [nRecords][2] for the table's lengths and checksums; slots / slotSegs [nRecords][2], recSizes, recStatus [nRecords]: what the batch wrote;
// pre: -1 = no pre-check ran (no records), else its go word with preStatus[2]. dst holds dstCapacity bytes. poison: in place, the kept frames' bytes are set
// to 0xC3 once the old entries are stashed -- they are neither read nor written from there on.
// Returns 0, or the library's code (zsk_edit_call_check; info[7] = the position it names) where the host refuses -- nothing is written then --, or the
// open's error code. outStatus[2]; offsOut / tileOffsOut (where given) [nPicks + 1]; info[0] = the stream size, info[1] = the go word, info[2] = 1: in place.
extern "C" int emu_edit_run(const uint8_t* old, uint64_t oldSize, const uint32_t* picks, uint32_t nPicks, const uint8_t* src, const uint64_t* records, uint32_t nRecords,
                            const uint8_t* slots, const uint64_t* slotSegs, const uint64_t* recSizes, const int32_t* recStatus, int32_t pre, const int32_t* preStatus,
                            uint32_t checksum, uint8_t* dst, uint64_t dstCapacity, uint32_t poison, int32_t* outStatus, uint64_t* offsOut, uint64_t* tileOffsOut, uint64_t* info)
{
    memset(info, 0, 8 * sizeof(uint64_t));
    Opened o;
    if (old) if (int e = open_stream(old, oldSize, &o)) return e;
    EmuBackend& b = o.b;
    const ZskOpened* const opened = old ? &o : nullptr;
    const ZskEditPick* const pk = (const ZskEditPick*)picks;
    bool inPlace = false; size_t bad = 0;
    if (const int rc = zsk_edit_call_check(true, opened, pk, nPicks, records, nRecords, 0, checksum ? ZHIP_SEEKABLE_CHECKSUM : 0, dst, dstCapacity, &inPlace, &bad, b.err)) { info[7] = bad; return rc; }
    info[2] = inPlace;
    const ZskEditLayout l = zsk_edit_layout(nPicks, nRecords, old ? o.lay.n : 0, inPlace, zsk_entry_size((int)checksum));
    uint8_t* pin = nullptr; uint8_t* m = nullptr;
    if (nPicks) b.reserve(ZSK_A_PIN, nPicks * sizeof(ZskEditPick), &pin);
    b.reserve(ZSK_A_SK_META, l.end, &m);
    uint64_t streamSize = ~0ull; uint32_t preWord = pre > 0 ? 1u : 0u;
    ZskEditArgs e; memset(&e, 0, sizeof e);               // the records' results: the test's
    if (nRecords) { e.src = src; e.records = records; e.slots = slots; e.slotSegs = slotSegs; e.recSizes = recSizes; e.recStatus = recStatus; }
    if (pre >= 0) { e.pre = &preWord; e.preStatus = preStatus; }
    if (inPlace && poison) { b.poisonAt = dst; b.poisonBytes = (size_t)o.lay.tableOffset; }
    if (const int rc = zsk_edit_picks(b, opened, pk, nPicks, inPlace, checksum, l, m, pin, e, dst, dstCapacity, &streamSize, outStatus)) return rc;
    if (b.traceOnly) return 0;
    info[0] = streamSize; info[1] = *b.sawEdit.v.go;
    if (offsOut) memcpy(offsOut, b.sawEdit.v.offs, ((size_t)nPicks + 1) * 8);
    if (tileOffsOut) memcpy(tileOffsOut, b.sawEdit.tileOffs, ((size_t)nPicks + 1) * 8);
    return 0;
}

#ifdef ZSK_EDIT_MAIN
// emu_seekable_edit <file>: the cases of the file back to back, little-endian, every buffer of exactly the size the call is given:
//   {blob old (length 0: none), u64 nPicks, u32 picks [nPicks][2], blob src, u64 nRecords, u64 records [nRecords][2], blob slots, u64 slotSegs [nRecords][2],
//    u64 recSizes [nRecords], i32 recStatus [nRecords], i64 pre, i32 preStatus [2], u64 checksum, u64 dstCapacity, u64 inPlace, u64 poison, u64 wantRc,
//    i32 want [2], blob wantStream}
// A call that succeeds leaves exactly wantStream at the start of dst; one that fails or is refused leaves dst as it was (in place: the old stream, 0x5A behind
// it; else 0x5A) and, where it ran, the size 0 and the status `want`. Exit 0: every case held.
static bool rd(FILE* f, void* p, size_t n) { return !n || fread(p, 1, n, f) == n; }
static bool rd_blob(FILE* f, std::vector<uint8_t>* v) { uint64_t n; if (!rd(f, &n, 8)) return false; v->assign((size_t)n, 0); return rd(f, v->data(), v->size()); }
int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s <cases>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int cases = 0;
    for (;; cases++) {
        std::vector<uint8_t> old, src, slots, want;
        uint64_t nPicks = 0, nRecords = 0, t[5]; int64_t pre = 0; int32_t preStatus[2], wantStatus[2];
        if (!rd_blob(f, &old)) break;
        if (!rd(f, &nPicks, 8)) return 2;
        std::vector<uint32_t> picks(2 * (size_t)nPicks);
        if (!rd(f, picks.data(), picks.size() * 4) || !rd_blob(f, &src) || !rd(f, &nRecords, 8)) return 2;
        std::vector<uint64_t> records(2 * (size_t)nRecords), slotSegs(2 * (size_t)nRecords), recSizes((size_t)nRecords);
        std::vector<int32_t> recStatus((size_t)nRecords);
        if (!rd(f, records.data(), records.size() * 8) || !rd_blob(f, &slots) || !rd(f, slotSegs.data(), slotSegs.size() * 8) || !rd(f, recSizes.data(), recSizes.size() * 8) ||
            !rd(f, recStatus.data(), recStatus.size() * 4) || !rd(f, &pre, 8) || !rd(f, preStatus, 8) || !rd(f, t, 40) || !rd(f, wantStatus, 8) || !rd_blob(f, &want)) return 2;
        const uint64_t checksum = t[0], capacity = t[1], inPlace = t[2], poison = t[3], wantRc = t[4];
        std::vector<uint8_t> dst((size_t)capacity, 0x5A);
        if (inPlace) { if (old.size() > dst.size()) return 2; memcpy(dst.data(), old.data(), old.size()); }
        const std::vector<uint8_t> was = dst;
        const uint8_t* const o = old.empty() ? nullptr : inPlace ? dst.data() : old.data();
        int32_t status[2] = {-1, -1}; uint64_t info[8];
        const int rc = emu_edit_run(o, old.size(), picks.data(), (uint32_t)nPicks, src.data(), records.data(), (uint32_t)nRecords, slots.data(), slotSegs.data(), recSizes.data(),
                                    recStatus.data(), (int32_t)pre, preStatus, (uint32_t)checksum, dst.data(), capacity, (uint32_t)poison, status, nullptr, nullptr, info);
        if ((uint64_t)rc != wantRc) { fprintf(stderr, "case %d: the call returned %d\n", cases, rc); return 1; }
        if (rc) { if (dst != was) { fprintf(stderr, "case %d: a refused call wrote\n", cases); return 1; } continue; }
        if (status[0] != wantStatus[0] || status[1] != wantStatus[1]) { fprintf(stderr, "case %d: status {%d, %d}\n", cases, status[0], status[1]); return 1; }
        if (status[0]) {
            if (info[0] || info[1]) { fprintf(stderr, "case %d: a failed stream has a size\n", cases); return 1; }
            if (dst != was) { fprintf(stderr, "case %d: a failed stream wrote\n", cases); return 1; }
            continue;
        }
        std::vector<uint8_t> expect = was;
        if (inPlace && poison) { Opened op; if (open_stream(old.data(), old.size(), &op)) return 2; memset(expect.data(), 0xC3, (size_t)op.lay.tableOffset); memset(want.data(), 0xC3, (size_t)op.lay.tableOffset); }
        if (info[0] != want.size() || want.size() > expect.size()) { fprintf(stderr, "case %d: the stream has %llu bytes, not %zu\n", cases, (unsigned long long)info[0], want.size()); return 1; }
        memcpy(expect.data(), want.data(), want.size());
        if (dst != expect) { fprintf(stderr, "case %d: the stream differs\n", cases); return 1; }
    }
    fclose(f);
    printf("%d cases\n", cases);
    return cases ? 0 : 2;
}
#endif
