// zhip_seekable_typed.hpp -- typed seekable streams: a tensor of k-byte elements (k = 2, 4, 8) stored as one BYTE PLANE per frame, so that every byte position
// of the elements gets entropy tables of its own. The source is cut into groups of frameSize elements (a shorter last one, e elements); group g
// becomes the k frames g * k + p, p = 0 .. k - 1, frame g * k + p holding byte p of every element of the group in element order. Behind the last plane frame
// stands the MARKER, a skippable frame of 24 bytes with a seek-table entry of its own (Compressed_Size 24, Decompressed_Size 0):
//
//     0x184D2A5D | Frame_Size = 16 | 'Z' 'H' 'P' 'L' | version = 1 | element_size | frame_size          (all little-endian words)
//
// and the standard seek table comes last: the stream is an ordinary seekable stream whose content is the PLANAR bytes.
// What is here: the two transposition kernels (interleaved -> planar with the record table of the plane frames, planar -> interleaved driven by a job table),
// the two kernels that seal a stream the records call has written, the status reducer of the typed read, and the host plan of that read. One-wave
// workgroups written against zhip_device.hpp like zhip_seekable.hpp, so the same bodies run under the host wave emulator (tests/emu/emu_seekable_typed.cpp).
#pragma once
#include "zhip_seekable.hpp"

#define ZSK_PLANES_MAGIC 0x184D2A5Du
#define ZSK_PLANES_TAG 0x4C50485Au           // 'Z' 'H' 'P' 'L'
#define ZSK_PLANES_VERSION 1u
#define ZSK_MARKER 24u                       // the marker frame: magic, Frame_Size, four words
#define ZSK_XXH_EMPTY 0x51D8E999u            // the low word of XXH64 of nothing: the marker's checksum word
#define ZSK_PLANE_TILE 1024u                 // elements of one group a workgroup takes per step: 16 per lane
#define ZSK_MAX_PLANE_FRAMES (ZSK_MAX_FRAMES - 1)      // the marker is a frame of the table too

ZSK_HD bool zsk_element_ok(uint32_t k) { return k == 2 || k == 4 || k == 8; }
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
// the 24 bytes a probe read where the last entry says (24, 0) -> 0: no marker (a plain stream), 1: a marker this reader understands, -1: a marker it does not
static inline int zsk_parse_marker(const uint8_t* m, uint32_t* k, uint32_t* frameSize)
{
    if (zsk_rd32(m) != ZSK_PLANES_MAGIC || zsk_rd32(m + 4) != 16 || zsk_rd32(m + 8) != ZSK_PLANES_TAG) return 0;
    *k = zsk_rd32(m + 16); *frameSize = zsk_rd32(m + 20);
    return zsk_rd32(m + 12) == ZSK_PLANES_VERSION && zsk_element_ok(*k) && *frameSize >= 1 && *frameSize <= ZSK_MAX_CONTENT ? 1 : -1;
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
template <int K> ZH_DEV void zsk_split16(const uint8_t* s, uint8_t* d, uint64_t plane)
{
    uint32_t w[4 * K];
#pragma unroll
    for (int j = 0; j < K; j++) zsk_words(zh_ld128(s + 16 * j), w + 4 * j);
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
// the mirror image: 16 bytes of each of the K planes (plane p at s + p * plane) -> 16 elements at d
template <int K> ZH_DEV void zsk_join16(const uint8_t* s, uint64_t plane, uint8_t* d)
{
    uint32_t w[K][4];
#pragma unroll
    for (int p = 0; p < K; p++) zsk_words(zh_ld128(s + p * plane), w[p]);
#pragma unroll
    for (int j = 0; j < K; j++) {
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int W = 4 * j + q;                   // the output word: bytes 4W .. 4W + 3 of the 16 elements
            if (K == 2) o[q] = zsk_perm(w[1][W >> 1], w[0][W >> 1], W & 1 ? 0x07030602u : 0x05010400u);
            else { const int per = K / 4, i = W / per, p0 = (W % per) * 4; o[q] = zsk_byte_of4(w[p0][i >> 2], w[p0 + 1][i >> 2], w[p0 + 2][i >> 2], w[p0 + 3][i >> 2], i & 3); }
        }
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
// a workgroup per tile of ZSK_PLANE_TILE elements of one group (grid-stride over the tiles of all groups); a lane per plane frame writes its record
ZH_DEV void zsk_planes_split_body(const ZskPlanesArgs& a)
{
    const uint32_t tpg = (a.group + ZSK_PLANE_TILE - 1) / ZSK_PLANE_TILE;
    const uint64_t tiles = (uint64_t)a.nGroups * tpg;
    for (uint64_t t = zh_block(); t < tiles; t += zh_nblocks()) {
        const uint64_t g = t / tpg, at = g * a.group * a.k;
        const uint32_t e = zsk_group_len(a.elements, a.group, g), i0 = (uint32_t)(t % tpg) * ZSK_PLANE_TILE + zh_lane() * 16;
        if (a.k == 2) zsk_split_lane<2>(a.src + at, a.dst + at, e, i0);
        else if (a.k == 4) zsk_split_lane<4>(a.src + at, a.dst + at, e, i0);
        else zsk_split_lane<8>(a.src + at, a.dst + at, e, i0);
    }
    if (!a.records) return;
    for (uint64_t i = (uint64_t)zh_block() * 64 + zh_lane(); i < (uint64_t)a.nGroups * a.k; i += (uint64_t)zh_nblocks() * 64) {
        const uint64_t g = i / a.k, e = zsk_group_len(a.elements, a.group, g);
        a.records[2 * i] = g * a.group * a.k + (i % a.k) * e; a.records[2 * i + 1] = e;
    }
}

// ------------------------------------------------------------------------------------------------ join: planar -> interleaved, by jobs
// A job: m elements whose planes lie at planar + p * m; output byte j in [h, m * k - t) -- byte j % k of element j / k -- goes to dst[j - h]. h, t < k trim
// the first and the last element of a range that starts or ends inside one. Without a job table the jobs are the groups of a whole buffer.
struct ZskJoinJob { uint64_t planar, m, dst, tilePrefix; uint32_t h, t; };      // planar, dst: offsets from the two bases; tilePrefix: the launch's tiles in front
struct ZskJoinArgs {
    const uint8_t* planar; uint8_t* dst;
    const ZskJoinJob* jobs; uint32_t nJobs; uint64_t tiles;
    uint32_t k, group; uint64_t elements;       // jobs NULL: the whole buffer, group g one job
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
ZH_DEV void zsk_planes_join_body(const ZskJoinArgs& a)
{
    const uint32_t tpg = (a.group + ZSK_PLANE_TILE - 1) / ZSK_PLANE_TILE;
    for (uint64_t t = zh_block(); t < a.tiles; t += zh_nblocks()) {
        ZskJoinJob job;
        if (a.jobs) {
            uint32_t lo = 0, hi = a.nJobs;                                  // the last job whose tilePrefix <= t
            while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (a.jobs[mid].tilePrefix <= t) lo = mid; else hi = mid; }
            job = a.jobs[lo];
        } else {
            const uint64_t g = t / tpg;
            job.planar = job.dst = g * a.group * a.k; job.m = zsk_group_len(a.elements, a.group, g); job.tilePrefix = g * tpg; job.h = job.t = 0;
        }
        const uint64_t i0 = (t - job.tilePrefix) * ZSK_PLANE_TILE + zh_lane() * 16;
        if (a.k == 2) zsk_join_lane<2>(a.planar + job.planar, a.dst + job.dst, job.m, job.h, job.t, i0);
        else if (a.k == 4) zsk_join_lane<4>(a.planar + job.planar, a.dst + job.dst, job.m, job.h, job.t, i0);
        else zsk_join_lane<8>(a.planar + job.planar, a.dst + job.dst, job.m, job.h, job.t, i0);
    }
}

// ------------------------------------------------------------------------------------------------ seal: the marker behind a stream the records call wrote
// The records call leaves n plane frames, the table behind them and *streamSize (0: it failed, and so does the typed call). The marker goes where the table
// starts and the table 24 bytes further on, one entry longer; the two overlap, so the first kernel keeps the stream size and the old entries aside.
struct ZskSealArgs {
    uint8_t* dst; uint64_t dstCapacity; uint64_t* streamSize; int32_t* outStatus;
    uint8_t* stash;                             // 16 bytes (the records call's stream size) + the n entries
    uint32_t n, checksum, elementSize, frameSize;
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

// The plan. A user range covers elements E0 .. E1 (rounded out to whole elements; h and t bytes of the first and the last are not its own). Group by group:
// a group it covers whole is the group's k frames, contiguous in the planar content -- neighbouring whole groups are ONE planar range, and one join job each;
// a group it covers in part is k planar ranges, elements lo .. hi - 1 of every plane, laid back to back in the planar buffer P -- one join job. P is filled
// from 0 in every pass; a pass closes where the next piece would take P beyond the limit (a piece above the limit is alone in its pass).
struct ZskTypedPass { uint32_t q0, q1, job0, job1; uint64_t bytes, tiles; };
struct ZskTypedPlan {
    std::vector<uint64_t> planar;               // [Q][3]: what the many-ranges call is handed, (offset, length, offset in P)
    std::vector<ZskJoinJob> jobs; std::vector<ZskTypedPass> passes;
    std::vector<uint32_t> owner;                // [R][2]
    uint64_t pMax = 0;
};
// D = dOff of the opened stream; rg = [R][3], checked (zsk_gather_check); limit 0 = ZSK_SCRATCH_DEFAULT
static inline void zsk_typed_plan(const uint64_t* D, uint32_t k, uint32_t group, const uint64_t* rg, size_t R, uint64_t limit, ZskTypedPlan* out)
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
                const uint64_t lo = E0 > g0 ? E0 - g0 : 0, hi = E1 + 1 < g0 + e ? E1 + 1 - g0 : e, m = hi - lo;
                if (used && used + m * k > limit) close();
                ZskJoinJob job;
                job.planar = used; job.m = m; job.h = g0 + lo == E0 ? (uint32_t)(a - E0 * k) : 0; job.t = g0 + hi == E1 + 1 ? (uint32_t)((E1 + 1) * k - (a + len)) : 0;
                job.dst = to + ((g0 + lo) * k + job.h - a); job.tilePrefix = cur.tiles;
                cur.tiles += zsk_join_tiles(m);
                out->jobs.push_back(job);
                if (m == e) {
                    if (merge) out->planar[out->planar.size() - 2] += e * k;
                    else { out->planar.push_back(D[f]); out->planar.push_back(e * k); out->planar.push_back(used); }
                    merge = true;
                } else {
                    for (uint32_t p = 0; p < k; p++) { out->planar.push_back(D[f + p] + lo); out->planar.push_back(m); out->planar.push_back(used + p * m); }
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
#endif
