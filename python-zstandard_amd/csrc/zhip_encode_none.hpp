// zhip_encode_none.hpp -- no match search at all (ZHIP_FINDER_NONE): every source becomes a literals-only frame, one WAVE per source, ONE kernel per chunk in place of
// both the match kernel and the entropy kernel.
//
// The frame is the one the entropy kernel writes behind an empty sequence list (zhip_compress_sequences_device with count 0), byte for byte what libzstd's
// ZSTD_compressSequences writes for the list that is only the block delimiter: a literals section (Huffman, raw or RLE) and the byte "0 sequences", or a raw block where
// that does not gain ZSTD_minGain. What differs is what it costs: the literals ARE the source, so ZePre::lits points at the source itself -- no arena slot, no literal
// workspace and no gather copy (ze_gather_literals under ZeMeta.mode 4), no tables. With pre->lits set and nbSeq 0, ze_compress_block reads pre->lits and nothing of
// pre->seqs or its workspace; it still FORMS addresses from the workspace pointer, so that pointer is the library's idle pad (valid, never dereferenced) rather than null.
//
// It leaves behind what a match kernel and the entropy kernel leave together: status and size per source, and ZeMeta{nbSeq 0, mode 4} (mode 1 below 7 bytes, mode 2 for
// what ze_frame refuses -- several blocks, a row that is not fast / double-fast, a window that does not cover the source: status 40), so the trailer kernel
// (ze_trailer_body) and everything else that reads ZhipEncodeArgs.meta runs unchanged behind it.
//
// Included after zhip_encode_kernel.hpp (ZeLDS, ZePre, ZeMeta, ze_frame).
#pragma once

// Sources are claimed from the chunk's work counter as ze_entropy_body claims them (ZhipEncodeArgs.counter + 1), so the grid is the entropy kernel's.
ZH_DEVFN void ze_none_body(const ZhipEncodeArgs& a, ZeLDS& L)
{
    const uint32_t lane = zh_lane();
    uint8_t* const ws = const_cast<uint8_t*>(a.idle);                      // never dereferenced (above)
    for (;;) {
        const uint32_t got = zh_atomic_add(a.counter + 1, lane == 0 ? 1u : 0u);
        if (zh_opaque(lane) == 0) L.misc[15] = got;
        zh_sync();
        const uint32_t i = zh_first(L.misc[15]);
        zh_sync();
        if (i >= a.count) break;
        const uint32_t f = a.first + i;
        const uint64_t srcSize64 = a.srcSegs[2 * (size_t)f + 1];
        ZePre pre; pre.seqs = nullptr; pre.lits = a.src + a.srcSegs[2 * (size_t)f]; pre.nbSeq = 0; pre.litSize = (uint32_t)srcSize64;
        uint64_t produced = 0;
        const int err = ze_frame<false>(a, L, f, ws, &produced, &pre);      // (below 7 bytes ze_compress_block stores raw before it looks at `pre`; an empty source never reaches it)
        zh_sync();
        if (zh_opaque(lane) == 0) {
            ZeMeta m; m.nbSeq = 0; m.litSize = 0; m.pad = 0;
            m.mode = err ? 2u : srcSize64 < 7 ? 1u : 4u;
            if (m.mode == 4) m.litSize = (uint32_t)srcSize64;
            a.meta[i] = m;
            a.status[f] = err; a.outSizes[f] = err ? 0 : produced;
        }
    }
}
