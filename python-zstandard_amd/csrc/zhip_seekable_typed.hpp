// zhip_seekable_typed.hpp -- typed seekable streams: a tensor of k-byte elements (k = 2, 4, 8) stored as one BYTE PLANE per frame, so that every byte position
// of the elements gets entropy tables of its own. The source is cut into groups of frameSize elements (a shorter last one, e elements); group g
// becomes the k frames g * k + p, p = 0 .. k - 1, frame g * k + p holding byte p of every element of the group in element order. Behind the last plane frame
// stands the MARKER, a skippable frame of 24 bytes with a seek-table entry of its own (Compressed_Size 24, Decompressed_Size 0):
//
//     0x184D2A5D | Frame_Size = 16 | 'Z' 'H' 'P' 'L' | version = 1 | element_size | filter << 8 | frame_size          (all little-endian words)
//
// filter 0: the planes are those of the elements; filter 1 (delta): those of the differences of neighbouring elements within the group;
// filter 4 (xor with a base): those of x[i] ^ b[i], b a BASE tensor of the same size that the caller holds -- the previous checkpoint. The stream
// does NOT name its base: reading it with another base returns wrong elements with status 0.
// The standard seek table comes last: the stream is an ordinary seekable stream whose content is the PLANAR bytes.
// What is here: the two transposition kernels (interleaved -> planar with the record table of the plane frames, planar -> interleaved driven by a job table),
// their forms under the delta and xor filters and through a chain of links, the two kernels that seal a stream the records call has written, the status reducers
// of the typed reads, and the host plan of a read. Every filter has kernels of its own, instantiated from ONE split tile loop (zsk_split_tiles), ONE job lookup
// (zsk_join_job) and ONE transposition (zsk_planar_word) -- DESIGN.md 9.9 says which source forms keep the kernels' registers and which do not. One-wave
// workgroups written against zhip_device.hpp like zhip_seekable.hpp, so the same bodies run under the host wave emulator (tests/emu/emu_seekable_typed.cpp).
#pragma once
#include <type_traits>
#include "zhip_seekable.hpp"

#define ZSK_PLANES_MAGIC 0x184D2A5Du
#define ZSK_PLANES_TAG 0x4C50485Au           // 'Z' 'H' 'P' 'L'
#define ZSK_PLANES_VERSION 1u
#define ZSK_MARKER 24u                       // the marker frame: magic, Frame_Size, four words
#define ZSK_XXH_EMPTY 0x51D8E999u            // the low word of XXH64 of nothing: the marker's checksum word
#define ZSK_PLANE_TILE 1024u                 // elements of one group a workgroup takes per step: 16 per lane
#define ZSK_MAX_PLANE_FRAMES (ZSK_MAX_FRAMES - 1)      // the marker is a frame of the table too

// the marker's word at +16 is element_size | filter << 8: what was done to a group's elements before the plane split
#define ZSK_FILTER_NONE 0u
#define ZSK_FILTER_DELTA 1u                  // d[0] = x[0], d[i] = x[i] - x[i - 1] mod 2^(8k) on the elements' bit patterns as unsigned little-endian integers, per group
#define ZSK_FILTER_XOR_BASE 4u               // d[i] = x[i] ^ b[i] bytewise, b the caller's base at the same content offset (2 and 3 are no filters: refused everywhere)

ZSK_HD bool zsk_element_ok(uint32_t k) { return k == 2 || k == 4 || k == 8; }
ZSK_HD bool zsk_filter_ok(uint32_t filter) { return filter == ZSK_FILTER_NONE || filter == ZSK_FILTER_DELTA || filter == ZSK_FILTER_XOR_BASE; }
ZSK_HD bool zsk_typed_args_ok(uint64_t srcSize, uint32_t frameSize, uint32_t k)
{
    return zsk_element_ok(k) && srcSize % k == 0 && frameSize >= 1 && frameSize <= ZSK_MAX_CONTENT && zsk_frame_count(srcSize / k, frameSize) * k <= ZSK_MAX_PLANE_FRAMES;
}
// the records bound for the n * k plane frames, the marker and its entry
ZSK_HD uint64_t zsk_typed_bound(uint64_t srcSize, uint32_t frameSize, uint32_t k, int checksum)
{
    if (!zsk_typed_args_ok(srcSize, frameSize, k)) return 0;
    return zsk_records_bound(srcSize, zsk_frame_count(srcSize / k, frameSize) * k, checksum) + ZSK_MARKER + zsk_entry_size(checksum);
}
// the 24 bytes a probe read where the last entry says (24, 0) -> 0: no marker (a plain stream), 1: a marker this reader understands, -1: a marker it does not.
// The word at +16 holds the element size in bits 0 .. 7 and the filter above; a caller that takes no filter understands unfiltered streams only
static inline int zsk_parse_marker(const uint8_t* m, uint32_t* k, uint32_t* frameSize, uint32_t* filter = nullptr)
{
    if (zsk_rd32(m) != ZSK_PLANES_MAGIC || zsk_rd32(m + 4) != 16 || zsk_rd32(m + 8) != ZSK_PLANES_TAG) return 0;
    const uint32_t word = zsk_rd32(m + 16), f = word >> 8;
    *k = word & 0xFFu; *frameSize = zsk_rd32(m + 20);
    if (filter) *filter = f;
    return zsk_rd32(m + 12) == ZSK_PLANES_VERSION && zsk_element_ok(*k) && (filter ? zsk_filter_ok(f) : f == ZSK_FILTER_NONE) && *frameSize >= 1 && *frameSize <= ZSK_MAX_CONTENT ? 1 : -1;
}
// the shape a marker promises, against the table's decompressed offsets D [n + 1] (the marker is frame n - 1): k frames of one size per group, that size
// frameSize but for the last group's, which is 1 ... frameSize. Returns n, or the first frame that does not fit
static inline uint32_t zsk_typed_shape(const uint64_t* D, uint32_t n, uint32_t k, uint32_t frameSize)
{
    const uint32_t planes = n - 1;
    if (planes % k) return planes;
    for (uint32_t f = 0; f < planes; f++) {
        const uint64_t size = D[f + 1] - D[f];
        const bool last = f / k == planes / k - 1;
        if (f % k ? size != D[f] - D[f - 1] : last ? size < 1 || size > frameSize : size != frameSize) return f;
    }
    return n;
}

// ------------------------------------------------------------------------------------------------ byte moves in registers
// v_perm_b32: byte n of the result is byte sel[n] of the eight bytes {hi, lo} (0 .. 3: lo's, 4 .. 7: hi's), 0x0c: zero
#ifndef ZHIP_EMU
ZH_DEV uint32_t zsk_perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
#else
ZH_DEV uint32_t zsk_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int n = 0; n < 4; n++) { const uint32_t s = (sel >> (8 * n)) & 0xFF; r |= (s < 8 ? (uint32_t)(both >> (8 * s)) & 0xFFu : s == 0x0C ? 0u : 0xFFu) << (8 * n); }
    return r;
}
#endif
// byte b of the words a, b1, c, d, in that order: two picks of a byte pair, one merge
ZH_DEV uint32_t zsk_byte_of4(uint32_t a, uint32_t b1, uint32_t c, uint32_t d, uint32_t b)
{
    const uint32_t sel = 0x0C0C0000u | ((4 + b) << 8) | b;
    return zsk_perm(zsk_perm(d, c, sel), zsk_perm(b1, a, sel), 0x05040100u);
}
ZH_DEV void zsk_words(zh_v16 v, uint32_t* w) { w[0] = (uint32_t)v.lo; w[1] = (uint32_t)(v.lo >> 32); w[2] = (uint32_t)v.hi; w[3] = (uint32_t)(v.hi >> 32); }
ZH_DEV zh_v16 zsk_v16(const uint32_t* w) { zh_v16 v; v.lo = w[0] | ((uint64_t)w[1] << 32); v.hi = w[2] | ((uint64_t)w[3] << 32); return v; }

// 16 elements at s -> 16 bytes to each of the K planes, plane p at d + p * plane: K loads and K stores of 16 bytes
// (the loads and the stores are functions of their own: the delta kernels work on the words between them)
template <int K> ZH_DEV void zsk_load16(const uint8_t* s, uint32_t* w)
{
#pragma unroll
    for (int j = 0; j < K; j++) zsk_words(zh_ld128(s + 16 * j), w + 4 * j);
}
template <int K> ZH_DEV void zsk_split16_store(const uint32_t* w, uint8_t* d, uint64_t plane)
{
#pragma unroll
    for (int p = 0; p < K; p++) {
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {                  // elements 4q .. 4q + 3
            if (K == 2) o[q] = zsk_perm(w[2 * q + 1], w[2 * q], p ? 0x07050301u : 0x06040200u);
            else { const int W = K / 4, at = 4 * q * W + (p >> 2); o[q] = zsk_byte_of4(w[at], w[at + W], w[at + 2 * W], w[at + 3 * W], p & 3); }
        }
        zh_st128(d + p * plane, zsk_v16(o));
    }
}
template <int K> ZH_DEV void zsk_split16(const uint8_t* s, uint8_t* d, uint64_t plane)
{
    uint32_t w[4 * K];
    zsk_load16<K>(s, w);
    zsk_split16_store<K>(w, d, plane);
}
// the mirror image: 16 bytes of each of the K planes (plane p at s + p * plane) -> 16 elements. In three steps: the K planes' words as they lie (plane p's
// four at w + 4 p), their transposition into the 4 K words of the 16 elements, and the store -- the filters work on the words between the steps
template <int K> ZH_DEV void zsk_planar_load16(const uint8_t* s, uint64_t plane, uint32_t* w)
{
#pragma unroll
    for (int p = 0; p < K; p++) zsk_words(zh_ld128(s + p * plane), w + 4 * p);
}
// output word W, bytes 4W .. 4W + 3 of the 16 elements: THE transposition, written once
template <int K> ZH_DEV uint32_t zsk_planar_word(const uint32_t* w, int W)
{
    if constexpr (K == 2) return zsk_perm(w[4 + (W >> 1)], w[W >> 1], W & 1 ? 0x07030602u : 0x05010400u);
    else { const int per = K / 4, i = W / per, p0 = (W % per) * 4, at = 4 * p0 + (i >> 2); return zsk_byte_of4(w[at], w[at + 4], w[at + 8], w[at + 12], i & 3); }
}
template <int K> ZH_DEV void zsk_planar_words(const uint32_t* w, uint32_t* o)
{
#pragma unroll
    for (int W = 0; W < 4 * K; W++) o[W] = zsk_planar_word<K>(w, W);
}
template <int K> ZH_DEV void zsk_store16(const uint32_t* o, uint8_t* d)
{
#pragma unroll
    for (int j = 0; j < K; j++) zh_st128(d + 16 * j, zsk_v16(o + 4 * j));
}
template <int K> ZH_DEV void zsk_join16_words(const uint8_t* s, uint64_t plane, uint32_t* o)
{
    uint32_t w[4 * K];
    zsk_planar_load16<K>(s, plane, w);
    zsk_planar_words<K>(w, o);
}
// the plain join's: 16 bytes go out as soon as their four words stand (all 4 K words first would cost it 24 VGPRs: DESIGN.md 9.9)
template <int K> ZH_DEV void zsk_join16(const uint8_t* s, uint64_t plane, uint8_t* d)
{
    uint32_t w[4 * K];
    zsk_planar_load16<K>(s, plane, w);
#pragma unroll
    for (int j = 0; j < K; j++) {
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; q++) o[q] = zsk_planar_word<K>(w, 4 * j + q);
        zh_st128(d + 16 * j, zsk_v16(o));
    }
}

// ------------------------------------------------------------------------------------------------ split: interleaved -> planar, and the plane frames' records
struct ZskPlanesArgs {
    const uint8_t* src; uint8_t* dst;            // `elements` elements of k bytes; group g's plane p goes to dst + g * k * group + p * e_g
    uint64_t elements; uint32_t k, group, nGroups;
    uint64_t* records;                          // [nGroups * k][2]: (offset, length) of every plane in dst (NULL: not wanted)
};
ZH_DEV uint32_t zsk_group_len(uint64_t elements, uint32_t group, uint64_t g) { const uint64_t left = elements - g * group; return left < group ? (uint32_t)left : group; }
// a lane's share of a tile: elements i0 .. i0 + 15 of a group of e (s: the group's elements, d: its planes). Whole: the 16-byte body; the group's last
// elements, fewer than 16: byte by byte
template <int K> ZH_DEV void zsk_split_lane(const uint8_t* s, uint8_t* d, uint32_t e, uint32_t i0)
{
    if (i0 >= e) return;
    if (e - i0 >= 16) { zsk_split16<K>(s + (uint64_t)i0 * K, d + i0, e); return; }
    for (uint32_t i = i0; i < e; i++) for (uint32_t p = 0; p < K; p++) d[(uint64_t)p * e + i] = s[(uint64_t)i * K + p];
}
ZH_DEV void zsk_planes_records(const ZskPlanesArgs& a)
{
    if (!a.records) return;
    for (uint64_t i = (uint64_t)zh_block() * 64 + zh_lane(); i < (uint64_t)a.nGroups * a.k; i += (uint64_t)zh_nblocks() * 64) {
        const uint64_t g = i / a.k, e = zsk_group_len(a.elements, a.group, g);
        a.records[2 * i] = g * a.group * a.k + (i % a.k) * e; a.records[2 * i + 1] = e;
    }
}
// THE split tile loop, of all three split kernels: a workgroup per tile of ZSK_PLANE_TILE elements of one group (grid-stride over the tiles of all groups),
// lane(K, at, e, i0) on every lane of the wave -- K the element size as a type, at the group's byte offset in the source, the base and the planes, e its
// elements, i0 the lane's first one; no lane leaves in front of it (the delta lane shuffles). Then a lane per plane frame writes its record
template <class F> ZH_DEV void zsk_split_tiles(const ZskPlanesArgs& a, F lane)
{
    const uint32_t tpg = (a.group + ZSK_PLANE_TILE - 1) / ZSK_PLANE_TILE;
    const uint64_t tiles = (uint64_t)a.nGroups * tpg;
    for (uint64_t t = zh_block(); t < tiles; t += zh_nblocks()) {
        const uint64_t g = t / tpg, at = g * a.group * a.k;
        const uint32_t e = zsk_group_len(a.elements, a.group, g), i0 = (uint32_t)(t % tpg) * ZSK_PLANE_TILE + zh_lane() * 16;
        if (a.k == 2) lane(std::integral_constant<int, 2>(), at, e, i0);
        else if (a.k == 4) lane(std::integral_constant<int, 4>(), at, e, i0);
        else lane(std::integral_constant<int, 8>(), at, e, i0);
    }
    zsk_planes_records(a);
}
ZH_DEV void zsk_planes_split_body(const ZskPlanesArgs& a)
{
    zsk_split_tiles(a, [&](auto K, uint64_t at, uint32_t e, uint32_t i0) { zsk_split_lane<K()>(a.src + at, a.dst + at, e, i0); });
}

// ------------------------------------------------------------------------------------------------ split with the delta filter
// The subtraction is done on the words between the split's loads and its stores: no pass of its own over the source. A lane needs the element in front of its
// 16: lanes 1 .. 63 take it from the lane below with a DPP move (that lane's 16 are whole wherever this lane has any), lane 0 loads it, and the group's first element has 0 in front.
#ifndef ZHIP_EMU
typedef uint16_t zsk_u16x2 __attribute__((ext_vector_type(2)));
ZH_DEV uint32_t zsk_sub16x2(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_bit_cast(zsk_u16x2, a) - __builtin_bit_cast(zsk_u16x2, b)); }      // v_pk_sub_u16
ZH_DEV uint32_t zsk_add16x2(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_bit_cast(zsk_u16x2, a) + __builtin_bit_cast(zsk_u16x2, b)); }      // v_pk_add_u16
#else
ZH_DEV uint32_t zsk_sub16x2(uint32_t a, uint32_t b) { return ((a - b) & 0xFFFFu) | (((a >> 16) - (b >> 16)) << 16); }
ZH_DEV uint32_t zsk_add16x2(uint32_t a, uint32_t b) { return ((a + b) & 0xFFFFu) | (((a >> 16) + (b >> 16)) << 16); }
#endif
template <int K> ZH_DEV uint64_t zsk_ld_element(const uint8_t* p) { if constexpr (K == 2) return zh_ld16(p); else if constexpr (K == 4) return zh_ld32(p); else return zh_ld64(p); }
// w: the 4 K words of 16 elements, before: the words of the element in front of them (K = 2: in the high half of before[0]) -> the 16 differences, in place
template <int K> ZH_DEV void zsk_delta16(uint32_t* w, const uint32_t* before)
{
    if constexpr (K == 2) {                        // a word is two elements: what stands in front of them is the pair one element down
#pragma unroll
        for (int j = 7; j >= 0; j--) w[j] = zsk_sub16x2(w[j], zh_alignbit(w[j], j ? w[j - 1] : before[0], 16));
    } else if constexpr (K == 4) {
#pragma unroll
        for (int i = 15; i >= 0; i--) w[i] -= i ? w[i - 1] : before[0];
    } else {
#pragma unroll
        for (int i = 15; i >= 0; i--) {
            const uint64_t x = w[2 * i] | ((uint64_t)w[2 * i + 1] << 32), y = i ? w[2 * i - 2] | ((uint64_t)w[2 * i - 1] << 32) : before[0] | ((uint64_t)before[1] << 32), dl = x - y;
            w[2 * i] = (uint32_t)dl; w[2 * i + 1] = (uint32_t)(dl >> 32);
        }
    }
}
// a lane's share of a tile, as zsk_split_lane. EVERY lane of the wave calls (the lane shuffle); the group's last elements, fewer than 16: element by element
template <int K> ZH_DEV void zsk_split_delta_lane(const uint8_t* s, uint8_t* d, uint32_t e, uint32_t i0)
{
    constexpr int B = K == 8 ? 2 : 1;              // the words of the element in front
    const bool whole = i0 < e && e - i0 >= 16;
    uint32_t w[4 * K], before[B];
    // the tile's first element: the one in front is the last of the tile below, or nothing. Lane 0's load goes out WITH its 16 elements' loads: behind the
    // shuffle it would be a second memory round trip per tile. (K = 2: the WORD that ends with that element -- lane 0's i0 is a multiple of the tile, so two
    // elements stand in front of it -- since a 16-bit load is waited for where it is issued, which is that second round trip again)
    const uint64_t x = !(whole && zh_lane() == 0 && i0) ? 0 : K == 2 ? zh_ld32(s + (uint64_t)(i0 - 2) * 2) : zsk_ld_element<K>(s + (uint64_t)(i0 - 1) * K);
    if (whole) zsk_load16<K>(s + (uint64_t)i0 * K, w);
#pragma unroll
    for (int q = 0; q < B; q++) before[q] = zh_lane_below(whole ? w[4 * K - B + q] : 0u);
    if (whole) {
        if (zh_lane() == 0) {
            before[0] = (uint32_t)x;
            if constexpr (K == 8) before[1] = (uint32_t)(x >> 32);
        }
        zsk_delta16<K>(w, before);
        zsk_split16_store<K>(w, d + i0, e);
        return;
    }
    if (i0 >= e) return;
    uint64_t y = i0 ? zsk_ld_element<K>(s + (uint64_t)(i0 - 1) * K) : 0;
    for (uint32_t i = i0; i < e; i++) {
        const uint64_t x = zsk_ld_element<K>(s + (uint64_t)i * K), dl = x - y;
        for (uint32_t p = 0; p < K; p++) d[(uint64_t)p * e + i] = (uint8_t)(dl >> (8 * p));
        y = x;
    }
}
ZH_DEV void zsk_planes_split_delta_body(const ZskPlanesArgs& a)
{
    zsk_split_tiles(a, [&](auto K, uint64_t at, uint32_t e, uint32_t i0) { zsk_split_delta_lane<K()>(a.src + at, a.dst + at, e, i0); });
}

// ------------------------------------------------------------------------------------------------ split with the xor-with-base filter
// The XOR is done on the words between the split's loads and its stores, as the delta filter's subtraction: no pass of its own over the source. The base's 16
// elements stand at the source's offset, so a lane issues its 2 K loads of 16 bytes -- K of the source, K of the base -- back to back and waits once: a base
// load behind the first XOR would be a second memory round trip per tile. Bytewise, so no carries, no neighbours, no shuffle: a lane beyond the group's end returns.
struct ZskPlanesXorArgs { ZskPlanesArgs p; const uint8_t* base; };      // base: `elements` elements of k bytes, as src (ZskPlanesArgs keeps its layout)
template <int K> ZH_DEV void zsk_split_xor_lane(const uint8_t* s, const uint8_t* b, uint8_t* d, uint32_t e, uint32_t i0)
{
    if (i0 >= e) return;
    if (e - i0 >= 16) {
        uint32_t w[4 * K], x[4 * K];
        zsk_load16<K>(s + (uint64_t)i0 * K, w);
        zsk_load16<K>(b + (uint64_t)i0 * K, x);
#pragma unroll
        for (int j = 0; j < 4 * K; j++) w[j] ^= x[j];
        zsk_split16_store<K>(w, d + i0, e);
        return;
    }
    for (uint32_t i = i0; i < e; i++) for (uint32_t p = 0; p < K; p++) d[(uint64_t)p * e + i] = s[(uint64_t)i * K + p] ^ b[(uint64_t)i * K + p];
}
ZH_DEV void zsk_planes_split_xor_body(const ZskPlanesXorArgs& x)
{
    const ZskPlanesArgs& a = x.p;
    zsk_split_tiles(a, [&](auto K, uint64_t at, uint32_t e, uint32_t i0) { zsk_split_xor_lane<K()>(a.src + at, x.base + at, a.dst + at, e, i0); });
}

// ------------------------------------------------------------------------------------------------ join: planar -> interleaved, by jobs
// A job: m elements whose planes lie at planar + p * m; output byte j in [h, m * k - t) -- byte j % k of element j / k -- goes to dst[j - h]. h, t < k trim
// the first and the last element of a range that starts or ends inside one. Without a job table the jobs are the groups of a whole buffer.
// Under the delta filter a job starts at its group's first element, and `skip` elements in front of the output feed the sums only: the output is byte j in
// [skip * k + h, m * k - t), at dst[j - skip * k - h]. The plain join knows no skip (0 in all its jobs).
struct ZskJoinJob { uint64_t planar, m, dst, tilePrefix; uint32_t h, t; uint64_t skip; };      // planar, dst: offsets from the two bases; tilePrefix: the launch's tiles in front
struct ZskJoinArgs {
    const uint8_t* planar; uint8_t* dst;
    const ZskJoinJob* jobs; uint32_t nJobs; uint64_t tiles;
    uint32_t k, group; uint64_t elements;       // jobs NULL: the whole buffer, group g one job
    uint64_t* tileSums;                         // the delta kernels': [tiles], a tile's sum, then the sum of the job's tiles in front of it (NULL: the plain join)
};
ZSK_HD uint64_t zsk_join_tiles(uint64_t m) { return (m + ZSK_PLANE_TILE - 1) / ZSK_PLANE_TILE; }
template <int K> ZH_DEV void zsk_join_lane(const uint8_t* s, uint8_t* d, uint64_t m, uint32_t h, uint32_t t, uint64_t i0)
{
    if (i0 >= m) return;
    const uint64_t n = m - i0 < 16 ? m - i0 : 16, lo = i0 * K, hi = (i0 + n) * K, end = m * K - t;
    const uint64_t from = lo < h ? h : lo, to = hi > end ? end : hi;
    if (n == 16 && from == lo && to == hi) { zsk_join16<K>(s + i0, m, d + (lo - h)); return; }
    for (uint64_t j = from; j < to; j++) d[j - h] = s[(j % K) * m + j / K];      // a job's trimmed first / last element, its last elements, fewer than 16
}
// THE job lookup, of every join kernel: the job of the launch's tile t. content(j) is called with the job's index where there is a job table -- what stands
// parallel to the jobs (the xor joins' content offsets) is fetched there; of a whole buffer's group it is job.planar
template <class C> ZH_DEV ZskJoinJob zsk_join_job(const ZskJoinArgs& a, uint32_t tpg, uint64_t t, C content)
{
    ZskJoinJob job;
    if (a.jobs) {
        uint32_t lo = 0, hi = a.nJobs;                                      // the last job whose tilePrefix <= t
        while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (a.jobs[mid].tilePrefix <= t) lo = mid; else hi = mid; }
        job = a.jobs[lo];
        content(lo);
    } else {
        const uint64_t g = t / tpg;
        job.planar = job.dst = g * a.group * a.k; job.m = zsk_group_len(a.elements, a.group, g); job.tilePrefix = g * tpg; job.h = job.t = 0; job.skip = 0;
    }
    return job;
}
ZH_DEV ZskJoinJob zsk_join_job(const ZskJoinArgs& a, uint32_t tpg, uint64_t t) { return zsk_join_job(a, tpg, t, [](uint32_t) {}); }
ZH_DEV void zsk_planes_join_body(const ZskJoinArgs& a)
{
    const uint32_t tpg = (a.group + ZSK_PLANE_TILE - 1) / ZSK_PLANE_TILE;
    for (uint64_t t = zh_block(); t < a.tiles; t += zh_nblocks()) {
        const ZskJoinJob job = zsk_join_job(a, tpg, t);
        const uint64_t i0 = (t - job.tilePrefix) * ZSK_PLANE_TILE + zh_lane() * 16;
        if (a.k == 2) zsk_join_lane<2>(a.planar + job.planar, a.dst + job.dst, job.m, job.h, job.t, i0);
        else if (a.k == 4) zsk_join_lane<4>(a.planar + job.planar, a.dst + job.dst, job.m, job.h, job.t, i0);
        else zsk_join_lane<8>(a.planar + job.planar, a.dst + job.dst, job.m, job.h, job.t, i0);
    }
}

// ------------------------------------------------------------------------------------------------ join with the delta filter: three launches
// The inverse is the inclusive prefix sum of a job's elements mod 2^(8k), which crosses tiles. It crosses them at kernel boundaries only -- no workgroup waits
// for another one inside a launch:
//     zsk_delta_sums     a workgroup per tile joins the tile's planes in registers and stores the sum of its elements, tileSums[tile]
//     zsk_delta_offsets  a wave per job turns its tiles' sums into their exclusive prefix sums, in place, 64 tiles a trip with a running carry
//     zsk_planes_join_delta   a workgroup per tile joins again, sums a lane's 16 elements serially, adds the wave's exclusive sum of the lane totals and the
//                        tile's offset, truncates to 8k bits and stores, trimmed as the plain join
// All sums are 64 bits wide whatever k is: truncation commutes with addition. The planar bytes are read twice.
template <int K> ZH_DEV uint64_t zsk_ld_planar(const uint8_t* s, uint64_t m, uint64_t i)
{
    uint64_t v = 0;
#pragma unroll
    for (int p = 0; p < K; p++) v |= (uint64_t)s[(uint64_t)p * m + i] << (8 * p);
    return v;
}
// element i of the 4 K words of 16 elements
template <int K> ZH_DEV uint64_t zsk_word_element(const uint32_t* o, int i)
{
    if constexpr (K == 2) return (o[i >> 1] >> (16 * (i & 1))) & 0xFFFFu; else if constexpr (K == 4) return o[i]; else return o[2 * i] | ((uint64_t)o[2 * i + 1] << 32);
}
// the sum of a lane's share of a tile: elements i0 .. i0 + 15 of a job of m; whole in registers, the job's last elements one by one
template <int K> ZH_DEV uint64_t zsk_delta_lane_sum(const uint8_t* s, uint64_t m, uint64_t i0)
{
    uint64_t sum = 0;
    if (i0 >= m) return 0;
    if (m - i0 >= 16) {
        uint32_t o[4 * K];
        zsk_join16_words<K>(s + i0, m, o);
#pragma unroll
        for (int i = 0; i < 16; i++) sum += zsk_word_element<K>(o, i);
        return sum;
    }
    for (uint64_t i = i0; i < m; i++) sum += zsk_ld_planar<K>(s, m, i);
    return sum;
}
ZH_DEV void zsk_delta_sums_body(const ZskJoinArgs& a)
{
    const uint32_t tpg = (a.group + ZSK_PLANE_TILE - 1) / ZSK_PLANE_TILE;
    for (uint64_t t = zh_block(); t < a.tiles; t += zh_nblocks()) {
        const ZskJoinJob job = zsk_join_job(a, tpg, t);
        const uint64_t i0 = (t - job.tilePrefix) * ZSK_PLANE_TILE + zh_lane() * 16;
        const uint8_t* const s = a.planar + job.planar;
        const uint64_t sum = zh_scan_add64(a.k == 2 ? zsk_delta_lane_sum<2>(s, job.m, i0) : a.k == 4 ? zsk_delta_lane_sum<4>(s, job.m, i0) : zsk_delta_lane_sum<8>(s, job.m, i0));
        if (zh_lane() == 63) a.tileSums[t] = sum;
    }
}
ZH_DEV void zsk_delta_offsets_body(const ZskJoinArgs& a)
{
    const uint32_t tpg = (a.group + ZSK_PLANE_TILE - 1) / ZSK_PLANE_TILE, nJobs = a.jobs ? a.nJobs : (uint32_t)zsk_frame_count(a.elements, a.group);
    for (uint32_t j = zh_block(); j < nJobs; j += zh_nblocks()) {
        const uint64_t first = a.jobs ? a.jobs[j].tilePrefix : (uint64_t)j * tpg, n = a.jobs ? zsk_join_tiles(a.jobs[j].m) : tpg;      // (a shorter last group has a group's tiles too, the empty ones summing to 0)
        uint64_t carry = 0;
        for (uint64_t at = 0; at < n; at += 64) {
            const uint64_t i = at + zh_lane(), v = i < n ? a.tileSums[first + i] : 0, incl = zh_scan_add64(v);
            if (i < n) a.tileSums[first + i] = carry + incl - v;
            carry += zsk_shfl64(incl, 63);
        }
    }
}
// EVERY lane of the wave calls (the scan of the lane totals). offset: the sum of the job's elements in front of the tile
template <int K> ZH_DEV void zsk_join_delta_lane(const uint8_t* s, uint8_t* d, const ZskJoinJob& job, uint64_t i0, uint64_t offset)
{
    const uint64_t m = job.m, n = i0 >= m ? 0 : m - i0 < 16 ? m - i0 : 16;
    const uint64_t lo = i0 * K, hi = (i0 + n) * K, first = job.skip * K + job.h, end = m * K - job.t;
    const uint64_t from = lo < first ? first : lo, to = hi > end ? end : hi;
    uint32_t o[4 * K];
    uint64_t total = 0;
    if (n == 16) {                                 // the lane's inclusive sums, truncated, in the words' place
        zsk_join16_words<K>(s + i0, m, o);
#pragma unroll
        for (int i = 0; i < 16; i++) {
            total += zsk_word_element<K>(o, i);
            if constexpr (K == 2) o[i >> 1] = i & 1 ? (o[i >> 1] & 0xFFFFu) | ((uint32_t)total << 16) : (o[i >> 1] & 0xFFFF0000u) | ((uint32_t)total & 0xFFFFu);
            else if constexpr (K == 4) o[i] = (uint32_t)total;
            else { o[2 * i] = (uint32_t)total; o[2 * i + 1] = (uint32_t)(total >> 32); }
        }
    } else for (uint64_t i = i0; i < i0 + n; i++) total += zsk_ld_planar<K>(s, m, i);
    const uint64_t base = offset + zh_scan_add64(total) - total;      // what stands in front of the lane's first element
    if (from >= to) return;
    if (n == 16 && from == lo && to == hi) {
#pragma unroll
        for (int W = 0; W < 4 * K; W++) {
            if constexpr (K == 2) o[W] = zsk_add16x2(o[W], ((uint32_t)base & 0xFFFFu) * 0x10001u);
            else if constexpr (K == 4) o[W] += (uint32_t)base;
            else if (!(W & 1)) { const uint64_t x = (o[W] | ((uint64_t)o[W + 1] << 32)) + base; o[W] = (uint32_t)x; o[W + 1] = (uint32_t)(x >> 32); }
        }
        zsk_store16<K>(o, d + (lo - first));
        return;
    }
    uint64_t sum = base;                           // a job's trimmed first / last element, the lane the skip ends in, its last elements, fewer than 16
    for (uint64_t i = i0; i < i0 + n; i++) {
        sum += zsk_ld_planar<K>(s, m, i);
        for (uint32_t p = 0; p < K; p++) { const uint64_t j = i * K + p; if (j >= from && j < to) d[j - first] = (uint8_t)(sum >> (8 * p)); }
    }
}
ZH_DEV void zsk_planes_join_delta_body(const ZskJoinArgs& a)
{
    const uint32_t tpg = (a.group + ZSK_PLANE_TILE - 1) / ZSK_PLANE_TILE;
    for (uint64_t t = zh_block(); t < a.tiles; t += zh_nblocks()) {
        const ZskJoinJob job = zsk_join_job(a, tpg, t);
        const uint64_t tile = t - job.tilePrefix, i0 = tile * ZSK_PLANE_TILE + zh_lane() * 16;
        if ((tile + 1) * ZSK_PLANE_TILE <= job.skip) continue;         // inside the skip: it fed the sums, it stores nothing
        const uint64_t offset = a.tileSums[t];
        if (a.k == 2) zsk_join_delta_lane<2>(a.planar + job.planar, a.dst + job.dst, job, i0, offset);
        else if (a.k == 4) zsk_join_delta_lane<4>(a.planar + job.planar, a.dst + job.dst, job, i0, offset);
        else zsk_join_delta_lane<8>(a.planar + job.planar, a.dst + job.dst, job, i0, offset);
    }
}

// ------------------------------------------------------------------------------------------------ join with the xor-with-base filter: one launch
// The plain join on the same jobs, tiles and grids, with the base's bytes XORed in between the join's words and their store. The base's bytes stand at the
// job's place in the CONTENT -- (g0 + lo) * k for a range's job, g * group * k for a whole buffer's group -- which `dst` does not give (a range's destination
// is the caller's): content[j], parallel to jobs[j], carries it (ZskJoinJob keeps its layout). Byte j of a job is XORed with base[content + j], the trimmed
// first and last element and the tails byte by byte at the same offsets; nothing of the base outside the bytes that are stored is read.
struct ZskJoinXorArgs { ZskJoinArgs j; const uint8_t* base; const uint64_t* content; };      // content [j.nJobs] (jobs NULL: not read)
template <int K> ZH_DEV void zsk_join_xor_lane(const uint8_t* s, const uint8_t* b, uint8_t* d, uint64_t m, uint32_t h, uint32_t t, uint64_t i0)
{
    if (i0 >= m) return;
    const uint64_t n = m - i0 < 16 ? m - i0 : 16, lo = i0 * K, hi = (i0 + n) * K, end = m * K - t;
    const uint64_t from = lo < h ? h : lo, to = hi > end ? end : hi;
    if (n == 16 && from == lo && to == hi) {
        uint32_t o[4 * K], x[4 * K];
        zsk_load16<K>(b + lo, x);                      // the base's loads go out with the planes': one wait for both
        zsk_join16_words<K>(s + i0, m, o);
#pragma unroll
        for (int j = 0; j < 4 * K; j++) o[j] ^= x[j];
        zsk_store16<K>(o, d + (lo - h));
        return;
    }
    for (uint64_t j = from; j < to; j++) d[j - h] = s[(j % K) * m + j / K] ^ b[j];
}
ZH_DEV void zsk_planes_join_xor_body(const ZskJoinXorArgs& x)
{
    const ZskJoinArgs& a = x.j;
    const uint32_t tpg = (a.group + ZSK_PLANE_TILE - 1) / ZSK_PLANE_TILE;
    for (uint64_t t = zh_block(); t < a.tiles; t += zh_nblocks()) {
        uint64_t content;
        const ZskJoinJob job = zsk_join_job(a, tpg, t, [&](uint32_t j) { content = x.content[j]; });
        if (!a.jobs) content = job.planar;
        const uint64_t i0 = (t - job.tilePrefix) * ZSK_PLANE_TILE + zh_lane() * 16;
        if (a.k == 2) zsk_join_xor_lane<2>(a.planar + job.planar, x.base + content, a.dst + job.dst, job.m, job.h, job.t, i0);
        else if (a.k == 4) zsk_join_xor_lane<4>(a.planar + job.planar, x.base + content, a.dst + job.dst, job.m, job.h, job.t, i0);
        else zsk_join_xor_lane<8>(a.planar + job.planar, x.base + content, a.dst + job.dst, job.m, job.h, job.t, i0);
    }
}

// ------------------------------------------------------------------------------------------------ join through a chain of xor-with-base links: one launch
// Version n of a tensor written as [full stream or base, v1 ^ v0, ..., vn ^ v(n-1)]: every link's planar buffer has the SAME layout -- the same
// jobs, job.planar offsets and tiles, one plan made once -- so byte j of a job is planar[0][..] ^ ... ^ planar[nLinks - 1][..], joined, ^ base[content + j]
// where there is a base. XOR is bytewise and commutes with the transposition: the links' PLANAR 16-byte words are XORed and transposed ONCE, K loads and 4 K
// XORs per link and 16 elements. The link loop's trip count is a run-time value (the pointers are read from the kernel's arguments by a wave-uniform index);
// it takes two links a trip, their 2 K loads issued before the first XOR, and the base's and link 0's loads stand in front of the loop. The trimmed first and
// last element and the tails go byte by byte; nothing of the base or of a planar buffer outside the stored bytes is read.
#define ZSK_CHAIN_MAX 16u
struct ZskJoinChainArgs { ZskJoinArgs j; const uint8_t* planar[ZSK_CHAIN_MAX]; uint32_t nLinks; const uint8_t* base; const uint64_t* content; };      // j.planar is not read; base NULL: none, content not read
// at: the job's offset in every planar buffer; b: the base at the job's content offset, or NULL
template <int K> ZH_DEV void zsk_join_chain_lane(const ZskJoinChainArgs& x, uint64_t at, const uint8_t* b, uint8_t* d, uint64_t m, uint32_t h, uint32_t t, uint64_t i0)
{
    if (i0 >= m) return;
    const uint64_t n = m - i0 < 16 ? m - i0 : 16, lo = i0 * K, hi = (i0 + n) * K, end = m * K - t;
    const uint64_t from = lo < h ? h : lo, to = hi > end ? end : hi;
    const uint32_t links = x.nLinks;
    if (n == 16 && from == lo && to == hi) {
        uint32_t w[4 * K], o[4 * K], xb[4 * K];
        if (b) zsk_load16<K>(b + lo, xb);              // the base's loads go out with link 0's: one wait for both
        zsk_planar_load16<K>(x.planar[0] + at + i0, m, w);
        uint32_t i = 1;
        for (; i + 1 < links; i += 2) {
            uint32_t u[4 * K], v[4 * K];
            zsk_planar_load16<K>(x.planar[i] + at + i0, m, u);
            zsk_planar_load16<K>(x.planar[i + 1] + at + i0, m, v);
#pragma unroll
            for (int j = 0; j < 4 * K; j++) w[j] ^= u[j] ^ v[j];
        }
        if (i < links) {
            uint32_t u[4 * K];
            zsk_planar_load16<K>(x.planar[i] + at + i0, m, u);
#pragma unroll
            for (int j = 0; j < 4 * K; j++) w[j] ^= u[j];
        }
        zsk_planar_words<K>(w, o);
        if (b) {
#pragma unroll
            for (int j = 0; j < 4 * K; j++) o[j] ^= xb[j];
        }
        zsk_store16<K>(o, d + (lo - h));
        return;
    }
    for (uint64_t j = from; j < to; j++) {             // a job's trimmed first / last element, its last elements, fewer than 16
        uint8_t v = b ? b[j] : 0;
        for (uint32_t i = 0; i < links; i++) v ^= x.planar[i][at + (j % K) * m + j / K];
        d[j - h] = v;
    }
}
ZH_DEV void zsk_planes_join_chain_body(const ZskJoinChainArgs& x)
{
    const ZskJoinArgs& a = x.j;
    const uint32_t tpg = (a.group + ZSK_PLANE_TILE - 1) / ZSK_PLANE_TILE;
    for (uint64_t t = zh_block(); t < a.tiles; t += zh_nblocks()) {
        uint64_t content = 0;
        const ZskJoinJob job = zsk_join_job(a, tpg, t, [&](uint32_t j) { if (x.base) content = x.content[j]; });
        if (!a.jobs) content = job.planar;
        const uint64_t i0 = (t - job.tilePrefix) * ZSK_PLANE_TILE + zh_lane() * 16;
        const uint8_t* const b = x.base ? x.base + content : nullptr;
        if (a.k == 2) zsk_join_chain_lane<2>(x, job.planar, b, a.dst + job.dst, job.m, job.h, job.t, i0);
        else if (a.k == 4) zsk_join_chain_lane<4>(x, job.planar, b, a.dst + job.dst, job.m, job.h, job.t, i0);
        else zsk_join_chain_lane<8>(x, job.planar, b, a.dst + job.dst, job.m, job.h, job.t, i0);
    }
}

// ------------------------------------------------------------------------------------------------ seal: the marker behind a stream the records call wrote
// The records call leaves n plane frames, the table behind them and *streamSize (0: it failed, and so does the typed call). The marker goes where the table
// starts and the table 24 bytes further on, one entry longer; the two overlap, so the first kernel keeps the stream size and the old entries aside.
struct ZskSealArgs {
    uint8_t* dst; uint64_t dstCapacity; uint64_t* streamSize; int32_t* outStatus;
    uint8_t* stash;                             // 16 bytes (the records call's stream size) + the n entries
    uint32_t n, checksum, elementSize, frameSize;      // elementSize: the marker's word at +16 as it is written, element size | filter << 8
};
#define ZSK_SEAL_HEAD 16u
ZSK_HD uint64_t zsk_seal_stash_bytes(uint64_t n, int checksum) { return ZSK_SEAL_HEAD + n * zsk_entry_size(checksum); }
// entries are 8 or 12 bytes: whole 16-byte pieces, then words
ZH_DEV void zsk_copy_words(uint8_t* d, const uint8_t* s, uint64_t bytes)
{
    const uint64_t whole = bytes & ~(uint64_t)15, lane = (uint64_t)zh_block() * 64 + zh_lane(), lanes = (uint64_t)zh_nblocks() * 64;
    for (uint64_t j = lane * 16; j < whole; j += lanes * 16) zh_st128(d + j, zh_ld128(s + j));
    if (lane < (bytes - whole) / 4) zh_st32(d + whole + lane * 4, zh_ld32(s + whole + lane * 4));
}
ZH_DEV void zsk_seal_stash_body(const ZskSealArgs& a)
{
    const uint64_t size = *a.streamSize;
    if (zh_block() == 0 && zh_lane() == 0) zh_st64(a.stash, size);
    if (!size) return;
    const uint64_t bytes = (uint64_t)a.n * zsk_entry_size((int)a.checksum);
    zsk_copy_words(a.stash + ZSK_SEAL_HEAD, a.dst + size - ZSK_FOOTER - bytes, bytes);
}
ZH_DEV void zsk_seal_body(const ZskSealArgs& a)
{
    const uint64_t size = zh_ld64(a.stash);
    if (!size) return;
    const uint32_t entry = zsk_entry_size((int)a.checksum);
    const uint64_t bytes = (uint64_t)a.n * entry, need = size + ZSK_MARKER + entry;
    const bool first = zh_block() == 0 && zh_lane() == 0;
    if (need > a.dstCapacity) {                 // the frames and their table fit, the marker and its entry do not: the last frame's index, as where only the table does not fit
        if (first) { a.outStatus[0] = ZSK_ERR_DSTSIZE; a.outStatus[1] = a.n ? (int32_t)(a.n - 1) : 0; *a.streamSize = 0; }
        return;
    }
    uint8_t* const marker = a.dst + size - zsk_table_size(a.n, (int)a.checksum);
    uint8_t* const table = marker + ZSK_MARKER;
    zsk_copy_words(table + ZSK_HEADER, a.stash + ZSK_SEAL_HEAD, bytes);
    if (!first) return;
    zh_st32(marker, ZSK_PLANES_MAGIC); zh_st32(marker + 4, 16); zh_st32(marker + 8, ZSK_PLANES_TAG); zh_st32(marker + 12, ZSK_PLANES_VERSION);
    zh_st32(marker + 16, a.elementSize); zh_st32(marker + 20, a.frameSize);
    zh_st32(table, ZSK_SKIP_MAGIC); zh_st32(table + 4, (a.n + 1) * entry + ZSK_FOOTER);
    uint8_t* const e = table + ZSK_HEADER + bytes;
    zh_st32(e, ZSK_MARKER); zh_st32(e + 4, 0);
    if (a.checksum) zh_st32(e + 8, ZSK_XXH_EMPTY);
    uint8_t* const f = e + entry;
    zh_st32(f, a.n + 1); f[4] = a.checksum ? 0x80 : 0; zh_st32(f + 5, ZSK_SEEK_MAGIC);
    *a.streamSize = need;
}

// ------------------------------------------------------------------------------------------------ the typed read: plan and status
// User range r became the planar ranges q0 .. q1 - 1 of the many-ranges calls (one per pass); planar range q's status pair lies at status + pairAt[q].
// A user range's pair is the pair of its first failing planar range; the overall pair names the lowest user range that failed.
struct ZskTypedStatusArgs { const uint32_t* owner; const uint32_t* pairAt; const int32_t* status; uint32_t nRanges; int32_t* outStatus; };
ZH_DEV uint32_t zsk_typed_first_bad(const ZskTypedStatusArgs& a, uint64_t r)      // ~0: none
{
    for (uint32_t q = a.owner[2 * r]; q < a.owner[2 * r + 1]; q++) if (a.status[a.pairAt[q]]) return q;
    return ~0u;
}
ZH_DEV void zsk_typed_status_body(const ZskTypedStatusArgs& a)
{
    for (uint64_t r = (uint64_t)zh_block() * 64 + zh_lane(); r < a.nRanges; r += (uint64_t)zh_nblocks() * 64) {
        const uint32_t q = zsk_typed_first_bad(a, r);
        a.outStatus[2 + 2 * r] = q != ~0u ? a.status[a.pairAt[q]] : 0; a.outStatus[3 + 2 * r] = q != ~0u ? a.status[a.pairAt[q] + 1] : 0;
    }
    if (zh_block() != 0) return;
    uint64_t first = ZSK_NONE;
    for (uint32_t r = zh_lane(); r < a.nRanges; r += 64) if (first == ZSK_NONE && zsk_typed_first_bad(a, r) != ~0u) first = r;
    first = zsk_wave_min64(first);
    if (zh_lane() == 0) { a.outStatus[0] = first != ZSK_NONE ? a.status[a.pairAt[zsk_typed_first_bad(a, first)]] : 0; a.outStatus[1] = first != ZSK_NONE ? (int32_t)first : 0; }
}

// The same over a chain's links: every link ran the same planar ranges into a status area of its own, laid out alike (status[i] + pairAt[q]). A user range
// fails if any link's frames under it failed; where several links fail, the EARLIEST link in chain order is reported, with its first failing planar range's
// pair -- the frame index is that link's own. outLink [1 + R] (NULL: not wanted): the link reported, -1 where none failed; [0] goes with the overall pair
struct ZskTypedStatusChainArgs { ZskTypedStatusArgs s; const int32_t* status[ZSK_CHAIN_MAX]; uint32_t nLinks; int32_t* outLink; };      // s.status is not read
ZH_DEV bool zsk_typed_chain_first_bad(const ZskTypedStatusChainArgs& c, uint64_t r, uint32_t* link, uint32_t* q)
{
    for (uint32_t i = 0; i < c.nLinks; i++)
        for (uint32_t p = c.s.owner[2 * r]; p < c.s.owner[2 * r + 1]; p++) if (c.status[i][c.s.pairAt[p]]) { *link = i; *q = p; return true; }
    return false;
}
ZH_DEV void zsk_typed_status_chain_body(const ZskTypedStatusChainArgs& c)
{
    const ZskTypedStatusArgs& a = c.s;
    uint32_t link = 0, q = 0;
    for (uint64_t r = (uint64_t)zh_block() * 64 + zh_lane(); r < a.nRanges; r += (uint64_t)zh_nblocks() * 64) {
        const bool bad = zsk_typed_chain_first_bad(c, r, &link, &q);
        a.outStatus[2 + 2 * r] = bad ? c.status[link][a.pairAt[q]] : 0; a.outStatus[3 + 2 * r] = bad ? c.status[link][a.pairAt[q] + 1] : 0;
        if (c.outLink) c.outLink[1 + r] = bad ? (int32_t)link : -1;
    }
    if (zh_block() != 0) return;
    uint64_t first = ZSK_NONE;
    for (uint32_t r = zh_lane(); r < a.nRanges; r += 64) if (first == ZSK_NONE && zsk_typed_chain_first_bad(c, r, &link, &q)) first = r;
    first = zsk_wave_min64(first);
    if (zh_lane() == 0) {
        const bool bad = first != ZSK_NONE && zsk_typed_chain_first_bad(c, first, &link, &q);
        a.outStatus[0] = bad ? c.status[link][a.pairAt[q]] : 0; a.outStatus[1] = bad ? (int32_t)first : 0;
        if (c.outLink) c.outLink[0] = bad ? (int32_t)link : -1;
    }
}

// The plan. A user range covers elements E0 .. E1 (rounded out to whole elements; h and t bytes of the first and the last are not its own). Group by group:
// a group it covers whole is the group's k frames, contiguous in the planar content -- neighbouring whole groups are ONE planar range, and one join job each;
// a group it covers in part is k planar ranges, elements lo .. hi - 1 of every plane, laid back to back in the planar buffer P -- one join job. P is filled
// from 0 in every pass; a pass closes where the next piece would take P beyond the limit (a piece above the limit is alone in its pass).
// Under the delta filter an element is the sum of everything in front of it in its group, so a group covered in part is fetched FROM ITS FIRST ELEMENT: its
// planar ranges are elements 0 .. hi - 1 of every plane, and the job gets m = hi and skip = lo -- the tiles inside the skip feed the sums and store nothing.
// The plane frames are decoded whole either way, so the decode costs what it did; what grows is the copy out of the decode scratch and the join, by the lo
// elements in front. Whole groups, merged runs, passes and the limit work as without a filter, and with filter 0 the plan is that one field for field.
// Under the xor-with-base filter the plan is the unfiltered one (no skip: a byte needs its base byte and nothing in front), and `content` gets, per job, the
// content offset of the job's first element -- where its base bytes stand. With filter 0 or 1 `content` stays empty.
struct ZskTypedPass { uint32_t q0, q1, job0, job1; uint64_t bytes, tiles; };
struct ZskTypedPlan {
    std::vector<uint64_t> planar;               // [Q][3]: what the many-ranges call is handed, (offset, length, offset in P)
    std::vector<ZskJoinJob> jobs; std::vector<ZskTypedPass> passes;
    std::vector<uint32_t> owner;                // [R][2]
    std::vector<uint64_t> content;              // [J] under ZSK_FILTER_XOR_BASE, else empty
    uint64_t pMax = 0;
};
// D = dOff of the opened stream; rg = [R][3], checked (zsk_gather_check); limit 0 = ZSK_SCRATCH_DEFAULT
static inline void zsk_typed_plan(const uint64_t* D, uint32_t k, uint32_t group, const uint64_t* rg, size_t R, uint64_t limit, ZskTypedPlan* out, uint32_t filter = ZSK_FILTER_NONE)
{
    if (!limit) limit = ZSK_SCRATCH_DEFAULT;
    *out = ZskTypedPlan();
    out->owner.resize(2 * R);
    ZskTypedPass cur; memset(&cur, 0, sizeof cur);
    uint64_t used = 0;
    bool merge = false;                         // the last planar range is a run of whole groups of this range and this pass: the next whole group extends it
    auto close = [&]() {
        cur.q1 = (uint32_t)(out->planar.size() / 3); cur.job1 = (uint32_t)out->jobs.size(); cur.bytes = used;
        if (cur.q1 > cur.q0) { out->passes.push_back(cur); if (used > out->pMax) out->pMax = used; }
        memset(&cur, 0, sizeof cur); cur.q0 = (uint32_t)(out->planar.size() / 3); cur.job0 = (uint32_t)out->jobs.size(); used = 0; merge = false;
    };
    for (size_t r = 0; r < R; r++) {
        const uint64_t a = rg[3 * r], len = rg[3 * r + 1], to = rg[3 * r + 2];
        out->owner[2 * r] = (uint32_t)(out->planar.size() / 3);
        merge = false;
        if (len) {
            const uint64_t E0 = a / k, E1 = (a + len - 1) / k;
            for (uint64_t g = E0 / group; g <= E1 / group; g++) {
                const uint64_t f = g * k, e = D[f + 1] - D[f], g0 = g * group;          // the group's first frame, its elements, its first element
                const uint64_t lo = E0 > g0 ? E0 - g0 : 0, hi = E1 + 1 < g0 + e ? E1 + 1 - g0 : e;
                const uint64_t skip = filter == ZSK_FILTER_DELTA && hi - lo != e ? lo : 0, m = hi - lo + skip, from = lo - skip;      // what is fetched: elements from .. hi - 1
                if (used && used + m * k > limit) close();
                ZskJoinJob job;
                job.planar = used; job.m = m; job.skip = skip; job.h = g0 + lo == E0 ? (uint32_t)(a - E0 * k) : 0; job.t = g0 + hi == E1 + 1 ? (uint32_t)((E1 + 1) * k - (a + len)) : 0;
                job.dst = to + ((g0 + lo) * k + job.h - a); job.tilePrefix = cur.tiles;
                cur.tiles += zsk_join_tiles(m);
                out->jobs.push_back(job);
                if (filter == ZSK_FILTER_XOR_BASE) out->content.push_back((g0 + lo) * k);
                if (hi - lo == e) {
                    if (merge) out->planar[out->planar.size() - 2] += e * k;
                    else { out->planar.push_back(D[f]); out->planar.push_back(e * k); out->planar.push_back(used); }
                    merge = true;
                } else {
                    for (uint32_t p = 0; p < k; p++) { out->planar.push_back(D[f + p] + from); out->planar.push_back(m); out->planar.push_back(used + p * m); }
                    merge = false;
                }
                used += m * k;
            }
        }
        out->owner[2 * r + 1] = (uint32_t)(out->planar.size() / 3);
    }
    close();
}

#ifndef ZHIP_EMU
__global__ __launch_bounds__(64) void zhip_seekable_planes_split_kernel(ZskPlanesArgs a) { zsk_planes_split_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_planes_join_kernel(ZskJoinArgs a) { zsk_planes_join_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_seal_stash_kernel(ZskSealArgs a) { zsk_seal_stash_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_seal_kernel(ZskSealArgs a) { zsk_seal_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_typed_status_kernel(ZskTypedStatusArgs a) { zsk_typed_status_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_planes_split_delta_kernel(ZskPlanesArgs a) { zsk_planes_split_delta_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_delta_sums_kernel(ZskJoinArgs a) { zsk_delta_sums_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_delta_offsets_kernel(ZskJoinArgs a) { zsk_delta_offsets_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_planes_join_delta_kernel(ZskJoinArgs a) { zsk_planes_join_delta_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_planes_split_xor_kernel(ZskPlanesXorArgs a) { zsk_planes_split_xor_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_planes_join_xor_kernel(ZskJoinXorArgs a) { zsk_planes_join_xor_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_planes_join_chain_kernel(ZskJoinChainArgs a) { zsk_planes_join_chain_body(a); }
__global__ __launch_bounds__(64) void zhip_seekable_typed_status_chain_kernel(ZskTypedStatusChainArgs a) { zsk_typed_status_chain_body(a); }
#endif
