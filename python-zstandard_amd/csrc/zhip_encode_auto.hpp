// zhip_encode_auto.hpp -- the match finder chosen per source (ZHIP_FINDER_AUTO): a classify kernel decides, from a bounded sample of every source, between the
// literals-only frame (ZHIP_FINDER_NONE, zhip_encode_none.hpp) and the default search (ZHIP_FINDER_LIBZSTD); the batch is split in device memory by that decision and
// the two parts run through those two paths as they are. Every frame is therefore byte for byte what one of the two pure finders writes for its source.
//
// The decision is a pure function of the source's bytes, in integer arithmetic (tests/auto_model.py restates it in numpy; the emulator and the device must agree with
// it exactly): not of the level, the batch, the launch shape, the chunking or the device. Lanes that compete for a table cell publish with an atomic max after every lane
// of the trip has read its candidate, as the wave match finder does (zhip_encode_wave.hpp), so the highest position wins whichever lane's store lands last.
//
// The sample ("the finder chosen per frame"): a source of up to ZA_ALL bytes is one window, all of it. A longer one has ZA_NWIN windows of ZA_WIN bytes, window
// w at (n - ZA_WIN) * (w + 1) / ZA_NWIN -- the last one ends at the source's end -- and in front of each window a stretch of up to ZA_FEED bytes (not reaching back into the
// window before) whose every ZA_STRIDE-th position is put into the table without being probed: matches in text lie further back than a window sees. 4 x 1 536 window bytes and
// 4 x 512 x 4 fed bytes are 14 KiB of a 128 KiB source, below an eighth of it.
//   * the windows' 256-bin byte histogram gives the literal cost: sum of count x (log2 total - log2 count) in 1/256 bit by za_log2fp (exponent + a quadratic for the mantissa),
//     at least one bit a byte (a Huffman code spends that);
//   * every window position probes the 4-byte hash table; a candidate's length L is measured up to ZA_CAP. A match is credited only where it is cheaper than its bytes as
//     literals: with hb the literal cost per byte and cost = (ZA_SEQ_BITS + log2 of the offset) bits, the position earns (L x hb - cost) / L where that is positive -- the saving
//     per covered byte -- once where the candidate was put in by a window (its neighbours were too, so every byte of the match earns by itself) and min(L, ZA_STRIDE) times
//     where it was fed sparsely (one position in ZA_STRIDE of such a match can hit);
//   * the search is chosen where credit x ZA_DEN > literal bits x ZA_NUM; a tie is the literals-only frame, the cheaper one to make.
// Unsampled: a source above one block (the literals-only kernel refuses it) and one below ZA_MIN bytes go to the search.
//
// Included after zhip_encode_kernel.hpp (ZF_BLOCK_MAX) and zhip_encode_plan.hpp (ZePlanIn, ze_none_refusal); the emulator includes tests/emu/zhip_device_emu_wave.hpp in front
// (zh_lds_atomic_max).
#pragma once

#define ZA_MIN 64u
#define ZA_ALL 8192u
#define ZA_NWIN 4u
#define ZA_WIN 1536u
#define ZA_FEED 4096u
#define ZA_STRIDE 8u
#define ZA_HLOG 12
#define ZA_CAP 32u
#define ZA_SEQ_BITS 14u
#define ZA_NUM 1u
#define ZA_DEN 64u
#define ZA_SEARCH 0u
#define ZA_LITERALS 1u
#define ZA_TILE 1024u          // sources per trip of the partition kernel: 16 choice bytes a lane

struct ZaLDS { uint32_t table[1u << ZA_HLOG]; uint32_t hist[256]; uint32_t misc[4]; };
// counter: one zeroed cell per launch (sources are claimed from it); choice: a byte per source; stats (may be null): 4 words per source -- window bytes, literal bits and
// credit in 1/256 bit, positions with a candidate of at least 4 bytes (all 0 for a source that was not sampled)
struct ZhipClassifyArgs { const uint8_t* src; const uint64_t* srcSegs; uint32_t first, count; uint8_t* choice; uint32_t* stats; uint32_t* counter; };
// the split: perm holds the indices of the sources that go to the search, in order, then those of the literals-only sources, in order; counts = {search, literals only}.
// Gathered tables and results are in perm's order, so the search's sub-batch is their first counts[0] entries and the other one the rest.
struct ZhipSplitArgs {
    const uint8_t* choice; uint32_t n; uint32_t* perm; uint32_t* counts;
    const uint64_t* srcSegs; const uint64_t* dstSegs; uint64_t* gSrcSegs; uint64_t* gDstSegs;      // gather
    uint64_t* outSizes; int32_t* status; const uint64_t* gOutSizes; const int32_t* gStatus;       // scatter
};

// ---- host side, free of HIP: what the call refuses, its grids and its scratch (owned by the context like its other buffers)
static inline const char* ze_auto_refusal(const ZeRows& rows, bool hasDict)      // ze_none_refusal's predicate: either part may be the literals-only kernel's
{
    if (!ze_none_refusal(rows, hasDict)) return nullptr;
    return hasDict ? "the match finder chosen per source (ZHIP_FINDER_AUTO, match finder \"auto\") does not take a dictionary"
                   : "the match finder chosen per source (ZHIP_FINDER_AUTO, match finder \"auto\") serves the levels whose one-block row is fast or double-fast (levels <= 4, negative levels, explicit strategy 1 / 2)";
}
struct ZeAutoPlan {
    size_t chunk = 0; uint32_t grid = 0, gridMove = 0;          // sources per classify launch and its waves; workgroups of the gather and scatter kernels (the partition kernel is one wave)
    size_t offChoice = 0, offPerm = 0, offSrcSegs = 0, offDstSegs = 0, offOutSizes = 0, offStatus = 0, bytes = 0;      // the scratch: [0] the classify counter, [4] the two counts, then these
};
static inline ZeAutoPlan ze_auto_plan(const ZePlanIn& in, int classifyPerCU)
{
    ZeAutoPlan s;
    const size_t n = in.n;
    s.chunk = n < 65536 ? n : 65536;
    if (in.knob.echunk && in.knob.echunk < s.chunk) s.chunk = in.knob.echunk;
    const size_t gmax = (size_t)in.dev.numCU * (size_t)(classifyPerCU > 0 ? classifyPerCU : 1);
    s.grid = (uint32_t)(s.chunk < gmax ? s.chunk : gmax);
    const size_t wg = (n + 63) / 64, wgMax = (size_t)in.dev.numCU * 8;
    s.gridMove = (uint32_t)(wg < wgMax || !wgMax ? wg : wgMax);
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    s.offChoice = 64;
    s.offPerm = s.offChoice + up(n);
    s.offSrcSegs = s.offPerm + up(4 * n);
    s.offDstSegs = s.offSrcSegs + 16 * n;
    s.offOutSizes = s.offDstSegs + 16 * n;
    s.offStatus = s.offOutSizes + 8 * n;
    s.bytes = s.offStatus + up(4 * n);
    return s;
}

// ---- device side
// log2 of x >= 1 (x < 2^23) in 1/256 bit: the exponent, and for the mantissa f = x / 2^e - 1 in 1/256 the polynomial f + 88 f (256 - f) / 65536 (at most 0.01 bit off)
ZH_DEV uint32_t za_log2fp(uint32_t x)
{
    const uint32_t e = (uint32_t)zh_highbit32(x), f = ((x << 8) >> e) - 256u;
    return (e << 8) + f + ((88u * f * (256u - f)) >> 16);
}
ZH_DEV uint32_t za_hash(uint32_t v) { return (v * 2654435761u) >> (32 - ZA_HLOG); }
// equal bytes of src[p ...] and src[c ...], c < p, at most lim (p + lim <= the source's size: nothing past the source is read)
ZH_DEV uint32_t za_count(const uint8_t* src, uint32_t p, uint32_t c, uint32_t lim)
{
    uint32_t n = 0;
    while (n + 8 <= lim) {
        const uint64_t x = zh_ld64(src + p + n) ^ zh_ld64(src + c + n);
        if (x) return n + ((uint32_t)zh_ctz64(x) >> 3);
        n += 8;
    }
    while (n < lim && src[p + n] == src[c + n]) n++;
    return n;
}
ZH_DEV uint32_t za_wave_sum(uint32_t v) { return zh_bcast(zh_scan_add(v), 63); }
ZH_DEV uint32_t za_win_start(uint32_t n, uint32_t w) { return n <= ZA_ALL ? 0u : (n - ZA_WIN) * (w + 1) / ZA_NWIN; }

// One wave per source, sources of the launch claimed from the work counter as ze_none_body claims them.
ZH_DEVFN void ze_classify_body(const ZhipClassifyArgs& a, ZaLDS& L)
{
    const uint32_t lane = zh_lane();
    for (;;) {
        const uint32_t got = zh_atomic_add(a.counter, lane == 0 ? 1u : 0u);
        if (zh_opaque(lane) == 0) L.misc[0] = got;
        zh_sync();
        const uint32_t i = zh_first(L.misc[0]);
        zh_sync();
        if (i >= a.count) break;
        const size_t f = (size_t)a.first + i;
        const uint8_t* const src = a.src + a.srcSegs[2 * f];
        const uint64_t n64 = a.srcSegs[2 * f + 1];
        uint32_t choice = ZA_SEARCH, total = 0, bits = 0, credit = 0, hits = 0;
        if (n64 >= ZA_MIN && n64 <= ZF_BLOCK_MAX) {
            const uint32_t n = (uint32_t)n64;
            const uint32_t nwin = n <= ZA_ALL ? 1u : ZA_NWIN, wlen = n <= ZA_ALL ? n : ZA_WIN;
            for (uint32_t k = lane; k < (1u << ZA_HLOG); k += 64) L.table[k] = 0;
            for (uint32_t k = lane; k < 256; k += 64) L.hist[k] = 0;
            zh_wave_fence();
            // ---- the windows' histogram and the literal cost
            for (uint32_t w = 0; w < nwin; w++) {
                const uint8_t* const win = src + za_win_start(n, w);
                for (uint32_t k = lane; k < wlen; k += 64) zh_lds_atomic_inc(&L.hist[win[k]]);
            }
            zh_wave_fence();
            total = nwin * wlen;
            const uint32_t lt = za_log2fp(total);
            uint32_t part = 0;
            for (uint32_t k = lane; k < 256; k += 64) { const uint32_t c = L.hist[k]; if (c) part += c * (lt - za_log2fp(c)); }
            bits = za_wave_sum(part);
            if (bits < total * 256u) bits = total * 256u;
            const uint32_t hb = bits / total;
            // ---- the probe
            uint32_t end = 0;
            for (uint32_t w = 0; w < nwin; w++) {
                const uint32_t start = za_win_start(n, w);
                if (nwin > 1) {
                    // the stretch in front of the window, every ZA_STRIDE-th position: published, not probed (bit 0 of the cell: fed sparsely)
                    const uint32_t lo = start - end < ZA_FEED ? end : start - ZA_FEED, cnt = (start - lo) / ZA_STRIDE, first = start - cnt * ZA_STRIDE;
                    for (uint32_t k = lane; k < cnt; k += 64) {
                        const uint32_t q = first + k * ZA_STRIDE;
                        zh_lds_atomic_max(&L.table[za_hash(zh_ld32(src + q))], ((q + 1) << 1) | 1u);
                    }
                    zh_wave_fence();
                }
                end = start + wlen;
                for (uint32_t base = start; base < end; base += 64) {
                    const uint32_t p = base + lane;
                    const bool valid = p < end && p + 4 <= n;             // (a position whose 4-byte load would cross the source's end neither probes nor publishes)
                    const uint32_t h = za_hash(valid ? zh_ld32(src + p) : 0u);
                    const uint32_t cell = valid ? L.table[h] : 0u;
                    zh_wave_fence();                                       // every lane has read its candidate ...
                    if (valid) zh_lds_atomic_max(&L.table[h], (p + 1) << 1);      // ... before any lane publishes: the table does not depend on the lanes' order
                    zh_wave_fence();
                    if (cell) {
                        const uint32_t c = (cell >> 1) - 1, lim = n - p < ZA_CAP ? n - p : ZA_CAP;
                        const uint32_t len = za_count(src, p, c, lim);
                        if (len >= 4) {
                            hits++;
                            const uint32_t cost = (ZA_SEQ_BITS + (uint32_t)zh_highbit32(p - c)) << 8, lit = len * hb;
                            if (lit > cost) credit += (lit - cost) / len * ((cell & 1u) ? (len < ZA_STRIDE ? len : ZA_STRIDE) : 1u);
                        }
                    }
                }
            }
            credit = za_wave_sum(credit); hits = za_wave_sum(hits);
            choice = (uint64_t)credit * ZA_DEN > (uint64_t)bits * ZA_NUM ? ZA_SEARCH : ZA_LITERALS;
        }
        if (zh_opaque(lane) == 0) {
            a.choice[f] = (uint8_t)choice;
            if (a.stats) { uint32_t* const s = a.stats + 4 * f; s[0] = total; s[1] = bits; s[2] = credit; s[3] = hits; }
        }
    }
}

// The stable partition of the source indices by the choice byte: ONE wave, ZA_TILE sources a trip, 16 bytes a lane -- a pass that counts the search's sources, which is
// where the literals-only indices begin in perm, and a pass that writes. (A batch of a million sources is a thousand trips.)
ZH_DEVFN void ze_auto_partition_body(const ZhipSplitArgs& a)
{
    const uint32_t lane = zh_lane();
    uint32_t zeros = 0;
    for (uint32_t k = lane; k < a.n; k += 64) zeros += a.choice[k] == ZA_SEARCH ? 1u : 0u;
    const uint32_t n0 = za_wave_sum(zeros);
    uint32_t at0 = 0, at1 = n0;
    for (uint32_t base = 0; base < a.n; base += ZA_TILE) {
        const uint32_t lo = base + 16 * lane;
        uint32_t mask = 0, valid = 0;                                          // bit j: source lo + j exists / goes to the literals-only kernel
        for (uint32_t j = 0; j < 16; j++) if (lo + j < a.n) { valid |= 1u << j; if (a.choice[lo + j] != ZA_SEARCH) mask |= 1u << j; }
        const uint32_t c1 = (uint32_t)zh_popc64(mask), c0 = (uint32_t)zh_popc64(valid) - c1;
        const uint32_t s0 = zh_scan_add(c0), s1 = zh_scan_add(c1);
        uint32_t w0 = at0 + s0 - c0, w1 = at1 + s1 - c1;
        for (uint32_t j = 0; j < 16; j++) if ((valid >> j) & 1u) { if ((mask >> j) & 1u) a.perm[w1++] = lo + j; else a.perm[w0++] = lo + j; }
        at0 += zh_bcast(s0, 63); at1 += zh_bcast(s1, 63);
    }
    if (zh_opaque(lane) == 0) { a.counts[0] = n0; a.counts[1] = a.n - n0; }
}
// the source and destination segment tables in perm's order
ZH_DEVFN void ze_auto_gather_body(const ZhipSplitArgs& a)
{
    for (uint32_t k = zh_block() * 64 + zh_lane(); k < a.n; k += zh_nblocks() * 64) {
        const size_t i = a.perm[k];
        a.gSrcSegs[2 * (size_t)k] = a.srcSegs[2 * i]; a.gSrcSegs[2 * (size_t)k + 1] = a.srcSegs[2 * i + 1];
        a.gDstSegs[2 * (size_t)k] = a.dstSegs[2 * i]; a.gDstSegs[2 * (size_t)k + 1] = a.dstSegs[2 * i + 1];
    }
}
// sizes and statuses of the two runs back to the sources' own indices
ZH_DEVFN void ze_auto_scatter_body(const ZhipSplitArgs& a)
{
    for (uint32_t k = zh_block() * 64 + zh_lane(); k < a.n; k += zh_nblocks() * 64) {
        const size_t i = a.perm[k];
        a.outSizes[i] = a.gOutSizes[k]; a.status[i] = a.gStatus[k];
    }
}
