// tests/emu/ncount_bounds_main.cpp -- bounds check of the FSE distribution parser (zd_read_ncount_to: K1 runs it on lane 0 over an LDS copy, K0 on every lane over the
// block where it lies) as a stand-alone PROGRAM (its own main; nothing is loaded into python, no LD_PRELOAD). Built by tests/emu/build_ncount_bounds.sh with
// -fsanitize=address,undefined. Its argument is tests/golden/fse_descriptions.bin (<- python -m tests.fsefamilies --write-fixture): every sequence-table description the
// families of tests/fsefamilies.py write -- count, then kind, alphabet limit, length, bytes each. Every description, and every proper prefix of it, is copied into a heap
// block of EXACTLY its size and parsed there into a heap block of exactly the 64 counts the parser may write, so a load past the description or a store past the counts is
// reported. A result is checked against itself only: bytes used within the block, the last symbol within the alphabet, the counts totalling 2^log. Exit status 0 and "ok".
#define ZHIP_EMU 1
extern "C" { long zd_trace_pos = -1; long zd_cur_frame = -1; long zd_stat[16]; }
#include "../../python-zstandard_amd/csrc/zhip_decode_kernel.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s fse_descriptions.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    fseek(f, 0, SEEK_END); const long size = ftell(f); fseek(f, 0, SEEK_SET);
    uint8_t* all = (uint8_t*)malloc((size_t)size);
    if (fread(all, 1, (size_t)size, f) != (size_t)size) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fclose(f);
    uint32_t count; memcpy(&count, all, 4);
    long at = 4, runs = 0, accepted = 0; int bad = 0;
    for (uint32_t d = 0; d < count; d++) {
        const uint32_t kind = all[at], maxSym = all[at + 1], len = all[at + 2] | (all[at + 3] << 8);
        at += 4;
        for (uint32_t n = 0; n <= len; n++) {                          // every proper prefix (the empty one too), then the whole
            uint8_t* src = (uint8_t*)malloc(n);                        // exactly the bytes the parser is told of
            memcpy(src, all + at, n);
            int16_t* norm = (int16_t*)malloc(64 * sizeof(int16_t));     // what ZdLDS.norm and ZpPre.norm[kind] hold
            uint32_t ms = maxSym, tl = 0;
            const int r = zd_read_ncount_to(norm, src, src + n, &ms, &tl);
            runs++;
            if (r >= 0) {
                accepted++;
                long total = 0;
                for (uint32_t s = 0; s <= ms && s < 64; s++) total += norm[s] < 0 ? 1 : norm[s];
                if ((uint32_t)r > n || r < 1 || ms > maxSym || tl < 5 || tl > 15 || total != (1l << tl)) {
                    fprintf(stderr, "description %u (kind %u), %u of %u bytes: used %d, last symbol %u, log %u, total %ld\n", d, kind, n, len, r, ms, tl, total); bad++;
                }
            }
            free(norm); free(src);
        }
        at += len;
    }
    if (at != size) { fprintf(stderr, "fixture: %ld bytes read of %ld\n", at, size); bad++; }
    printf("%s: %u descriptions, %ld runs, %ld accepted, %d failed\n", bad ? "FAILED" : "ok", count, runs, accepted, bad);
    free(all);
    return bad ? 1 : 0;
}
