// zhip_encode_wave.hpp -- the wave-parallel match finder (ZHIP_FINDER_WAVE): one WAVE per source, the hash table in LDS, 64 positions probed per trip.
//
// Every other search of this code base keeps libzstd's table contents, which makes it one lane's chain of dependent table round trips per source.
// This one does not: its frames are valid zstd that any decoder reads, NOT libzstd's bytes. What it leaves behind is what the flat searches leave -- ZE_SEQ_PACKed
// sequences in the source's arena slot and ZeMeta{nbSeq, mode 4} (mode 1 below 7 bytes, mode 2 for what ze_frame refuses) -- so the entropy kernel and the trailer
// kernel run unchanged behind it (launch_entropy).
//
// The output is a pure function of (source, parameters, H): a trip READS its 64 candidates before any lane publishes its own position, and positions are published
// with an atomic max, so the table never depends on which lane's store lands last; everything after the probe is wave-uniform. The host emulator runs this same body
// (tests/emu/emu_wave_finder.cpp) and the tests compare the two byte for byte.
//
// Included after zhip_encode_kernel.hpp (ZePar, ze_get_cparams, ZeMeta, ZE_SEQ_PACK).
#pragma once

#define ZW_CAP 64u            // a lane extends its own hit by at most this many bytes; a selected match that reached it is extended by the whole wave

ZH_DEV uint32_t zw_hash(uint64_t v, bool five, int H)
{
    // (libzstd's multiplicative hashes of 4 and of 5 bytes -- ZSTD_hash4 / ZSTD_hash5)
    return five ? (uint32_t)(((v << 24) * 889523592379ull) >> (64 - H)) : ((uint32_t)v * 2654435761u) >> (32 - H);
}

// equal bytes of src[p ...] and src[c ...], c < p, at most lim (p + lim <= srcSize: nothing past the source is read)
ZH_DEV uint32_t zw_count(const uint8_t* src, uint32_t p, uint32_t c, uint32_t lim)
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

// One wave per source, sources of the chunk in a grid-stride loop. table: 1 << H cells of LDS, a cell holds position + 1 (0: empty).
template <int H>
ZH_DEVFN void ze_match_wave_body(const ZhipEncodeArgs& a, uint32_t* table)
{
    const uint32_t lane = zh_lane();
    for (uint32_t i = zh_block(); i < a.count; i += zh_nblocks()) {
        const uint32_t f = a.first + i;
        ZeMeta m; m.nbSeq = 0; m.litSize = 0; m.mode = 2; m.pad = 0;
        const uint8_t* const src = a.src + a.srcSegs[2 * (size_t)f];
        const uint64_t srcSize64 = a.srcSegs[2 * (size_t)f + 1];
        const uint32_t srcSize = (uint32_t)srcSize64;
        ZePar cp;
        // refused here = refused by ze_frame with the same test (status 40): several blocks, a row that is not fast / double-fast, a window that does not cover the source,
        // table logs the entropy kernel refuses, any dictionary
        const bool ok = srcSize64 <= ZF_BLOCK_MAX && !a.cdict && ze_get_cparams(cp, a.rows, srcSize) == 0 && cp.hlog <= ZE_MAX_HLOG && cp.clog <= ZE_MAX_HLOG;
        if (!ok || srcSize < 7) {
            if (ok) m.mode = 1;
            if (zh_opaque(lane) == 0) a.meta[i] = m;
            continue;
        }
        const bool five = cp.mml >= 5;
        const uint32_t mm = cp.mml < 4 ? 4u : cp.mml > 7 ? 7u : (uint32_t)cp.mml;
        for (uint32_t k = lane; k < (1u << H); k += 64) table[k] = 0;
        zh_wave_fence();
        uint64_t* const seqs = (uint64_t*)(a.arena + (size_t)i * a.arenaStride + ZE_ARENA_SEQ);
        uint32_t rep0 = 1, rep1 = 4, rep2 = 8, anchor = 0, nseq = 0;
        for (uint32_t base = 0; base + 8 <= srcSize; ) {
            // ---- probe: lane l at position base + l. No match starts where its 8-byte load would cross the end of the source.
            const uint32_t p = base + lane;
            const bool valid = p + 8 <= srcSize;
            const uint64_t cur = valid ? zh_ld64(src + p) : 0;
            const uint32_t h = zw_hash(cur, five, H);
            const uint32_t cand = valid ? table[h] : 0u;
            zh_wave_fence();                                                   // every lane has read its candidate ...
            if (valid) zh_lds_atomic_max(table + h, p + 1);                    // ... before any lane publishes: the table does not depend on the lanes' order
            zh_wave_fence();
            const uint32_t lim = !valid ? 0u : srcSize - p < ZW_CAP ? srcSize - p : ZW_CAP;
            uint32_t len = 0, off = 0;
            if (cand) {
                len = zw_count(src, p, cand - 1, lim);
                off = p - (cand - 1);
                if (len < mm) len = 0;
            }
            // the most recent emitted offset (wave-uniform) at every position: finds the matches of a period below 64, which read-before-write cannot see inside a trip
            if (valid && p >= rep0) {
                const uint32_t rl = zw_count(src, p, p - rep0, lim);
                if (rl >= mm) { len = rl; off = rep0; }                    // (taken whenever it is long enough, as libzstd's fast search takes it: the offset costs a code, not 17 bits)
            }
            // ---- selection, wave-uniform: the lowest lane with a match at or after the anchor, again behind each match taken
            uint64_t hits = zh_ballot(len != 0);
            while (hits) {
                uint32_t l = (uint32_t)zh_ctz64(hits);
                // a repeat-offset match one position on wins over a table match here, as in libzstd's fast search (which tests the repeat offset at ip + 1 before the
                // table's candidate at ip): one literal more, an offset that costs a code instead of 17 bits, and a match that does not copy what ended the last one
                if (l < 63 && ((hits >> (l + 1)) & 1) && zh_bcast(off, l + 1) == rep0 && zh_bcast(off, l) != rep0) l++;
                uint32_t start = base + l, mlen = zh_bcast(len, l), moff = zh_bcast(off, l);
                if (l == 63 && moff != rep0 && start + 9 <= srcSize && start + 1 >= rep0) {
                    // (the trip's last lane has no neighbour to ask: the same test, by every lane at once, so that the parse does not depend on where the trips fall)
                    const uint32_t lim1 = srcSize - start - 1 < ZW_CAP ? srcSize - start - 1 : ZW_CAP;
                    const uint32_t rl = zw_count(src, start + 1, start + 1 - rep0, lim1);
                    if (rl >= mm) { start++; mlen = rl; moff = rep0; }
                }
                if (mlen == ZW_CAP) {
                    // the lane stopped at its cap: the whole wave extends, 8 bytes per lane per trip, a ballot finds the first difference
                    while (start + mlen < srcSize) {
                        const uint32_t q = start + mlen + 8 * lane;
                        uint32_t n = 0;
                        if (q + 8 <= srcSize) { const uint64_t x = zh_ld64(src + q) ^ zh_ld64(src + q - moff); n = x ? (uint32_t)zh_ctz64(x) >> 3 : 8u; }
                        else while (q + n < srcSize && src[q + n] == src[q + n - moff]) n++;
                        const uint64_t full = zh_ballot(n == 8);
                        if (~full == 0) { mlen += 512; continue; }
                        const uint32_t fl = (uint32_t)zh_ctz64(~full);
                        mlen += 8 * fl + zh_bcast(n, fl);
                        break;
                    }
                }
                while (start > anchor && start > moff && src[start - 1] == src[start - 1 - moff]) { start--; mlen++; }      // catch up backwards to the anchor
                // ---- repeat codes, decided here where the order of the sequences is known (ZSTD_finalizeOffBase / ZSTD_updateRep)
                const uint32_t ll = start - anchor;
                uint32_t offBase = moff + 3;
                if (ll) {
                    if (moff == rep0) offBase = 1;
                    else if (moff == rep1) { offBase = 2; rep1 = rep0; rep0 = moff; }
                    else if (moff == rep2) { offBase = 3; rep2 = rep1; rep1 = rep0; rep0 = moff; }
                    else { rep2 = rep1; rep1 = rep0; rep0 = moff; }
                } else {
                    if (moff == rep1) { offBase = 1; rep1 = rep0; rep0 = moff; }
                    else if (moff == rep2) { offBase = 2; rep2 = rep1; rep1 = rep0; rep0 = moff; }
                    else if (moff == rep0 - 1 && moff) { offBase = 3; rep2 = rep1; rep1 = rep0; rep0 = moff; }
                    else { rep2 = rep1; rep1 = rep0; rep0 = moff; }
                }
                if (zh_opaque(lane) == 0) seqs[nseq] = ZE_SEQ_PACK(offBase, ll, mlen);
                nseq++;
                anchor = start + mlen;
                hits = anchor - base >= 64 ? 0ull : hits & (~0ull << (anchor - base));
            }
            base = anchor > base + 64 ? anchor : base + 64;
        }
        m.nbSeq = nseq; m.mode = 4;                                           // sequences only: the entropy kernel gathers the literals
        if (zh_opaque(lane) == 0) a.meta[i] = m;
    }
}
