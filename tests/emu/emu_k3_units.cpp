// tests/emu/emu_k3_units.cpp -- the decode pipeline (K1 -> K2 -> K3) of the host wave emulator over the frames of tests/golden/k3_units.bin, as a stand-alone PROGRAM:
// tests/emu/build_asan_k3_units.sh builds it with -fsanitize=address,undefined (its own main; nothing is loaded into python, no LD_PRELOAD). The frames are
// tests/k3units.py's (python -m tests.k3units --write-fixture): long items in 16-byte units at every count around the 64 lanes, the hand-off record's fields at
// their largest, sources against the LDS history, above 2^17 and in a dictionary, slots below the 32 bytes of slack. Every frame must decode to the bytes whose
// hash the fixture carries (or be refused where it says so), frames of one block through the pipeline as they are, the others in the several-block mode.
//
// fixture, little-endian: "K3U1", u32 dictionary size, the dictionary (raw content), u32 count, then per frame: u32 flags (1: several-block mode, 2: with the
// dictionary), u32 frame size, u32 slot size, u32 expected size (0xFFFFFFFF: must be refused), u64 FNV-1a of the expected bytes, the frame.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

extern "C" int emu_decompress_pipeline(const uint8_t* src, const uint64_t* srcSegs, uint32_t n, uint8_t* dst, const uint64_t* dstSegs, uint64_t* outSizes, int32_t* status,
                                       uint32_t nBlocks, uint32_t chunk);
extern "C" void emu_set_blocks(uint32_t perFrame);
extern "C" int emu_set_ddict(const uint8_t* dict, uint32_t size, int rawContent);

#ifdef EMU_K3_UNITS_MAIN
struct Item { uint32_t flags, size, cap, want; uint64_t hash; size_t at; };

static uint64_t fnv1a(const uint8_t* p, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}
static uint32_t rd32(const std::vector<uint8_t>& b, size_t& at)
{
    uint32_t v; memcpy(&v, b.data() + at, 4); at += 4; return v;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s tests/golden/k3_units.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> b;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) b.insert(b.end(), buf, buf + n);
    fclose(f);
    if (b.size() < 12 || memcmp(b.data(), "K3U1", 4)) { fprintf(stderr, "not a k3_units fixture\n"); return 2; }
    size_t at = 4;
    const uint32_t dictSize = rd32(b, at);
    const size_t dictAt = at; at += dictSize;
    const uint32_t count = rd32(b, at);
    std::vector<Item> items(count);
    for (auto& it : items) {
        it.flags = rd32(b, at); it.size = rd32(b, at); it.cap = rd32(b, at); it.want = rd32(b, at);
        memcpy(&it.hash, b.data() + at, 8); at += 8;
        it.at = at; at += it.size;
        if (at > b.size()) { fprintf(stderr, "truncated fixture\n"); return 2; }
    }
    int bad = 0; uint32_t ran = 0;
    for (uint32_t group = 0; group < 4; group++) {
        std::vector<uint8_t> src; std::vector<uint64_t> srcSegs, dstSegs; std::vector<const Item*> mine;
        uint64_t room = 0;
        for (const auto& it : items) if (it.flags == group) {
            srcSegs.push_back(src.size()); srcSegs.push_back(it.size);
            src.insert(src.end(), b.begin() + (long)it.at, b.begin() + (long)(it.at + it.size));
            dstSegs.push_back(room); dstSegs.push_back(it.cap); room += it.cap;
            mine.push_back(&it);
        }
        if (mine.empty()) continue;
        src.resize(src.size() + 16);                                    // (the harness's own slack behind the last frame, as tests/emulib.py lays it out)
        std::vector<uint8_t> dst(room + 16);
        std::vector<uint64_t> outSizes(mine.size()); std::vector<int32_t> status(mine.size(), -1);
        if (emu_set_ddict(group & 2 ? b.data() + dictAt : nullptr, group & 2 ? dictSize : 0u, 1) != 0) { fprintf(stderr, "the dictionary was refused\n"); return 1; }
        emu_set_blocks(group & 1 ? 16u : 0u);
        const int handedOn = emu_decompress_pipeline(src.data(), srcSegs.data(), (uint32_t)mine.size(), dst.data(), dstSegs.data(), outSizes.data(), status.data(), 3, 0);
        emu_set_blocks(0); emu_set_ddict(nullptr, 0, 0);
        if (handedOn != 0) { fprintf(stderr, "group %u: %d frames went to the generic kernel\n", group, handedOn); bad++; }
        for (size_t i = 0; i < mine.size(); i++) {
            const Item& it = *mine[i];
            const bool ok = it.want == 0xFFFFFFFFu ? status[i] != 0
                                                   : status[i] == 0 && outSizes[i] == it.want && fnv1a(dst.data() + dstSegs[2 * i], it.want) == it.hash;
            if (!ok) { fprintf(stderr, "group %u frame %zu: status %d, %llu bytes (expected %u)\n", group, i, status[i], (unsigned long long)outSizes[i], it.want); bad++; }
            ran++;
        }
    }
    printf("k3 units: %u frames, %d wrong\n", ran, bad);
    return bad ? 1 : 0;
}
#endif
