// tests/emu/none_bounds_main.cpp -- bounds check of the literals-only kernel (ze_none_body, ZHIP_FINDER_NONE) as a stand-alone PROGRAM (its own main; nothing is loaded
// into python, no LD_PRELOAD). Built by tests/emu/build_none_bounds.sh with -fsanitize=address,undefined together with zhemu.cpp and emu_none_finder.cpp. Every argument
// is a file holding one source: it is read into a heap block of EXACTLY its size, so a load of the literal coder (histogram, bit count, emit: each reads the source, which
// IS the literals here), of the raw-block copy or of the trailer kernel past (or before) the source is reported, and compressed alone at levels 3, 1 and -1, with checksum
// and content size, into a heap block of exactly zhip_compress_bound's size (ze_compress_bound, asked of the emulator library), which is also the capacity the kernel is
// told. The kernel gets no arena and no workspace (null pointers in its arguments). Exit status 0 and "ok" when every status is 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

extern "C" int emu_none_frames(const uint8_t* src, const uint64_t* srcSegs, uint32_t n, uint8_t* dst, const uint64_t* dstSegs, uint64_t* outSizes, int32_t* status,
                               int level, const int32_t* ov, uint32_t flags, uint32_t nBlocks, int path, uint32_t echunk, uint32_t* metaOut);
extern "C" uint64_t emu_none_bound(uint64_t n);

int main(int argc, char** argv)
{
    int bad = 0; long runs = 0;
    const bool quick = argc > 1 && !strcmp(argv[1], "-q");            // -q (the test suite's run): levels 3 and -1
    for (int k = quick ? 2 : 1; k < argc; k++) {
        FILE* f = fopen(argv[k], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[k]); return 2; }
        fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
        uint8_t* src = (uint8_t*)malloc((size_t)n);                  // exactly the source (a zero-byte block for the empty one)
        if (n && fread(src, 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "cannot read %s\n", argv[k]); return 2; }
        fclose(f);
        const uint64_t cap = emu_none_bound((uint64_t)n);            // zhip_compress_bound, by the product's own function: not a byte more
        static const int levels[3] = {3, -1, 1};
        for (int l = 0; l < (quick ? 2 : 3); l++) {
            uint8_t* dst = (uint8_t*)malloc(cap);
            const uint64_t ssegs[2] = {0, (uint64_t)n}, dsegs[2] = {0, cap};
            uint64_t size = 0; int32_t st = -1; const int32_t ov[7] = {0, 0, 0, 0, 0, 0, 0};
            const int rc = emu_none_frames(src, ssegs, 1, dst, dsegs, &size, &st, levels[l], ov, 1 | 2, 1, 1, 0, nullptr);
            if (rc || st || size > cap) { fprintf(stderr, "%s: level %d: rc %d status %d size %llu\n", argv[k], levels[l], rc, st, (unsigned long long)size); bad++; }
            free(dst); runs++;
        }
        free(src);
    }
    printf("%s: %d sources, %ld runs, %d failed\n", bad ? "FAILED" : "ok", argc - (quick ? 2 : 1), runs, bad);
    return bad ? 1 : 0;
}
