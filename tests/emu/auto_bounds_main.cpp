// tests/emu/auto_bounds_main.cpp -- bounds check of the classifier of ZHIP_FINDER_AUTO (ze_classify_body) and of the split behind it as a stand-alone PROGRAM (its own main;
// nothing is loaded into python, no LD_PRELOAD). Built by tests/emu/build_auto_bounds.sh with -fsanitize=address,undefined together with zhemu.cpp and emu_auto_finder.cpp.
// Every argument is a file holding one source: it is read into a heap block of EXACTLY its size, so that the source ends where its allocation ends -- the last window of the
// sample ends there, and a 4-byte hash load, an 8-byte step of the length count or a fed position that reached past the source (or in front of it) is reported. The source is
// classified alone, with statistics, then compressed alone under the emulated "auto" with checksum and content size into a heap block of exactly zhip_compress_bound's size.
// Prints "ok: N sources ..." and the choices; exit status 0 when every status is 0 and both runs chose the same.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

extern "C" void emu_auto_classify(const uint8_t* src, const uint64_t* srcSegs, uint32_t n, uint8_t* choice, uint32_t* stats, uint32_t nBlocks, uint32_t chunk);
extern "C" int emu_auto_frames(const uint8_t* src, const uint64_t* srcSegs, uint32_t n, uint8_t* dst, const uint64_t* dstSegs, uint64_t* outSizes, int32_t* status,
                               int level, const int32_t* ov, uint32_t flags, uint32_t nBlocks, uint32_t echunk, int finder, uint8_t* choiceOut, uint32_t* statsOut, uint32_t* launches);
extern "C" uint64_t emu_auto_bound(uint64_t n);

int main(int argc, char** argv)
{
    int bad = 0;
    char* choices = (char*)calloc((size_t)argc * 2 + 1, 1);
    for (int k = 1; k < argc; k++) {
        FILE* f = fopen(argv[k], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[k]); return 2; }
        fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
        uint8_t* src = (uint8_t*)malloc((size_t)n);                  // exactly the source (a zero-byte block for the empty one)
        if (n && fread(src, 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "cannot read %s\n", argv[k]); return 2; }
        fclose(f);
        const uint64_t ssegs[2] = {0, (uint64_t)n};
        uint8_t alone = 9; uint32_t stats[4];
        emu_auto_classify(src, ssegs, 1, &alone, stats, 1, 0);
        const uint64_t cap = emu_auto_bound((uint64_t)n);            // zhip_compress_bound, by the product's own function: not a byte more
        uint8_t* dst = (uint8_t*)malloc(cap);
        const uint64_t dsegs[2] = {0, cap};
        uint64_t size = 0; int32_t st = -1; const int32_t ov[7] = {0, 0, 0, 0, 0, 0, 0};
        uint8_t inCall = 9;
        const int rc = emu_auto_frames(src, ssegs, 1, dst, dsegs, &size, &st, 3, ov, 1 | 2, 1, 0, 4, &inCall, nullptr, nullptr);
        if (rc || st || size > cap || alone > 1 || alone != inCall) { fprintf(stderr, "%s: rc %d status %d size %llu choice %d / %d\n", argv[k], rc, st, (unsigned long long)size, alone, inCall); bad++; }
        choices[2 * (k - 1)] = ' '; choices[2 * (k - 1) + 1] = (char)('0' + alone);
        free(dst); free(src);
    }
    printf("%s: %d sources, %d failed; choices:%s\n", bad ? "FAILED" : "ok", argc - 1, bad, choices);
    free(choices);
    return bad ? 1 : 0;
}
