// zhip_seekable_typed_calls.hpp -- HOST side of the typed seekable calls, free of HIP, beside zhip_seekable_calls.hpp: the checks, the layouts and the
// sequences as function templates over a backend. The typed calls are built AROUND the plain ones -- typed compress is the split kernel, the records call on
// the staging buffer and the seal; a typed read is the many-ranges call into a planar buffer, the join kernel and the status reducer -- so zsk_compress_records,
// zsk_open and zsk_ranges run as they are, with their own kernels, areas and traces, and nothing of zhip_seekable_calls.hpp changes. What the filters' entry
// points share is written once: zsk_launch_split picks the split kernel, zsk_typed_read_setup plans a read and uploads its tables.
//
// The backend is one of zhip_seekable_calls.hpp's, extended by:
//     int  reserve_typed(ZskTypedArea, size_t bytes, uint8_t** base)                    as reserve(); the areas are kept between calls like the others
//     void launch_typed(ZskTypedKernel, uint32_t grid, const void* args)                one-wave workgroups
#pragma once
#include "zhip_seekable_calls.hpp"
#include "zhip_seekable_typed.hpp"

#define ZSKT_KERNELS(X) \
    X(PLANES_SPLIT, planes_split, ZskPlanesArgs) X(PLANES_JOIN, planes_join, ZskJoinArgs) X(SEAL_STASH, seal_stash, ZskSealArgs) X(SEAL, seal, ZskSealArgs) \
    X(TYPED_STATUS, typed_status, ZskTypedStatusArgs) \
    X(PLANES_SPLIT_DELTA, planes_split_delta, ZskPlanesArgs) X(DELTA_SUMS, delta_sums, ZskJoinArgs) X(DELTA_OFFSETS, delta_offsets, ZskJoinArgs) \
    X(PLANES_JOIN_DELTA, planes_join_delta, ZskJoinArgs) \
    X(PLANES_SPLIT_XOR, planes_split_xor, ZskPlanesXorArgs) X(PLANES_JOIN_XOR, planes_join_xor, ZskJoinXorArgs) \
    X(PLANES_JOIN_CHAIN, planes_join_chain, ZskJoinChainArgs) X(TYPED_STATUS_CHAIN, typed_status_chain, ZskTypedStatusChainArgs)
#define ZSKT_X(id, name, args) ZSKT_K_##id,
enum ZskTypedKernel { ZSKT_KERNELS(ZSKT_X) ZSKT_K_COUNT };
#undef ZSKT_X
// the context's: the planar staging buffer (the source's bytes), the plane frames' records, the seal's stash; the handle's: the planar buffer of a read
// (at most the scratch limit, or one piece above it), its tables (jobs, owners, status places), the status arrays of its passes. The delta join's tile sums,
// 8 bytes a tile: the handle's for a read, the context's for the join on its own
enum ZskTypedArea { ZSKT_A_STAGING, ZSKT_A_RECORDS, ZSKT_A_STASH, ZSKT_A_PLANAR, ZSKT_A_TABLES, ZSKT_A_STATUS, ZSKT_A_TILESUMS, ZSKT_A_COUNT };

// what the open call's typed probe adds to a handle: elementSize 1 = a plain stream; filter: ZSK_FILTER_* of the marker
struct ZskTypedOpened : ZskOpened { uint32_t elementSize = 1, groupElements = 0, filter = ZSK_FILTER_NONE; };

// a workgroup per tile, eight waves a CU
static inline uint32_t zsk_tile_grid(int numCU, uint64_t tiles, uint64_t lanes)
{
    const uint64_t w = (lanes + 63) / 64, want = tiles > w ? tiles : w, gm = (uint64_t)(numCU > 0 ? numCU : 1) * 8;
    return (uint32_t)(want < 1 ? 1 : want < gm ? want : gm);
}
static inline uint64_t zsk_planes_tiles(uint64_t elements, uint32_t group) { return zsk_frame_count(elements, group) * ((group + ZSK_PLANE_TILE - 1) / ZSK_PLANE_TILE); }

// base: the call has one (the *_base_ calls: filter 4 and nothing else goes through them)
static inline int zsk_planes_check(bool pointers, uint64_t size, uint32_t k, uint32_t frameSize, std::string& err, uint32_t filter = ZSK_FILTER_NONE, bool base = false)
{
    if (!pointers) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "planes: bad arguments");
    if (!zsk_filter_ok(filter) || (filter == ZSK_FILTER_XOR_BASE) != base)
        return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "planes: the filter must be 0 (none) or 1 (delta); 4 (xor with a base) takes its base through the calls with a base");
    if (!zsk_element_ok(k)) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "planes: the element size must be 2, 4 or 8");
    if (size % k) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "planes: the size must be a multiple of the element size");
    if (frameSize < 1 || frameSize > ZSK_MAX_CONTENT) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "planes: frameSize must be 1 ... 2^30 elements");
    return 0;
}
static inline int zsk_typed_compress_check(bool pointers, uint64_t srcSize, uint32_t frameSize, uint32_t k, int flags, std::string& err, uint32_t filter = ZSK_FILTER_NONE, bool base = false)
{
    if (!pointers || (flags & ~ZHIP_SEEKABLE_CHECKSUM)) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "seekable typed compress: bad arguments");
    if (int rc = zsk_planes_check(true, srcSize, k, frameSize, err, filter, base)) return rc;
    if (zsk_frame_count(srcSize / k, frameSize) * k > ZSK_MAX_PLANE_FRAMES) return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, "seekable typed compress: at most 2^27 - 1 plane frames");
    return 0;
}

// what the calls with a base refuse on top: no base, an element size of 1, a base that shares bytes with the output (the output would change the base under
// the lanes that still have to read it). `bytes` of base, `outBytes` at d_out
static inline bool zsk_overlap(const void* a, uint64_t an, const void* b, uint64_t bn)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return an && bn && x < y + bn && y < x + an;
}
static inline int zsk_base_check(const char* what, const void* d_base, uint64_t bytes, uint32_t k, const void* d_out, uint64_t outBytes, std::string& err)
{
    char buf[200];
    if (!d_base) { snprintf(buf, sizeof buf, "%s: the base is NULL", what); return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, buf); }
    if (k == 1) { snprintf(buf, sizeof buf, "%s: a base needs an element size of 2, 4 or 8", what); return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, buf); }
    if (zsk_overlap(d_base, bytes, d_out, outBytes)) { snprintf(buf, sizeof buf, "%s: the base overlaps the output", what); return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, buf); }
    return 0;
}

// the split kernels' arguments (records, d_base: NULL where there are none), and THE split of a filter: the xor kernel takes the struct, the other two its ZskPlanesArgs
static inline ZskPlanesXorArgs zsk_split_args(const void* d_src, uint64_t size, uint32_t k, uint32_t frameSize, void* d_dst, const void* d_base, uint8_t* records)
{
    ZskPlanesXorArgs x; memset(&x, 0, sizeof x);
    ZskPlanesArgs& a = x.p;
    a.src = (const uint8_t*)d_src; a.dst = (uint8_t*)d_dst; a.elements = size / k; a.k = k; a.group = frameSize; a.nGroups = (uint32_t)zsk_frame_count(a.elements, frameSize);
    a.records = (uint64_t*)records; x.base = (const uint8_t*)d_base;
    return x;
}
template <class B> void zsk_launch_split(B& b, uint32_t filter, const ZskPlanesXorArgs& x, uint32_t grid)
{
    if (filter == ZSK_FILTER_XOR_BASE) b.launch_typed(ZSKT_K_PLANES_SPLIT_XOR, grid, &x);
    else b.launch_typed(filter == ZSK_FILTER_DELTA ? ZSKT_K_PLANES_SPLIT_DELTA : ZSKT_K_PLANES_SPLIT, grid, &x.p);
}
// The whole-buffer kernels on their own: interleaved -> planar (no records) and back. d_base: the *_base_ calls' (filter ZSK_FILTER_XOR_BASE), `size` bytes
template <class B> int zsk_planes_split(B& b, bool ctx, const void* d_src, uint64_t size, uint32_t k, uint32_t frameSize, void* d_dst, uint32_t filter = ZSK_FILTER_NONE, const void* d_base = nullptr)
{
    if (int rc = zsk_planes_check(ctx && (!size || (d_src && d_dst)), size, k, frameSize, b.err, filter, d_base != nullptr)) return rc;
    if (!size) return 0;
    zsk_launch_split(b, filter, zsk_split_args(d_src, size, k, frameSize, d_dst, d_base, nullptr), zsk_tile_grid(b.numCU, zsk_planes_tiles(size / k, frameSize), 0));
    return b.check();
}
template <class B> int zsk_planes_split_base(B& b, bool ctx, const void* d_src, uint64_t size, uint32_t k, uint32_t frameSize, const void* d_base, void* d_dst)
{
    if (int rc = zsk_base_check("planes split", d_base, size, k, d_dst, size, b.err)) return rc;
    return zsk_planes_split(b, ctx, d_src, size, k, frameSize, d_dst, ZSK_FILTER_XOR_BASE, d_base);
}
// the join of the handle's filter: the plain kernel, or the delta filter's three launches over tileSums [a.tiles]
template <class B> void zsk_launch_join(B& b, uint32_t filter, ZskJoinArgs& a, uint64_t nJobs, uint8_t* tileSums)
{
    const uint32_t grid = zsk_tile_grid(b.numCU, a.tiles, 0);
    if (filter != ZSK_FILTER_DELTA) { b.launch_typed(ZSKT_K_PLANES_JOIN, grid, &a); return; }
    a.tileSums = (uint64_t*)tileSums;
    b.launch_typed(ZSKT_K_DELTA_SUMS, grid, &a);
    b.launch_typed(ZSKT_K_DELTA_OFFSETS, zsk_tile_grid(b.numCU, nJobs, 0), &a);
    b.launch_typed(ZSKT_K_PLANES_JOIN_DELTA, grid, &a);
}
// the xor-with-base join: the plain join's grid, one launch. content: the jobs' content offsets on the device (NULL with a.jobs NULL)
template <class B> void zsk_launch_join_xor(B& b, const ZskJoinArgs& a, const void* d_base, const uint8_t* content)
{
    ZskJoinXorArgs x; memset(&x, 0, sizeof x);
    x.j = a; x.base = (const uint8_t*)d_base; x.content = (const uint64_t*)content;
    b.launch_typed(ZSKT_K_PLANES_JOIN_XOR, zsk_tile_grid(b.numCU, a.tiles, 0), &x);
}
template <class B> int zsk_planes_join(B& b, bool ctx, const void* d_src, uint64_t size, uint32_t k, uint32_t frameSize, void* d_dst, uint32_t filter = ZSK_FILTER_NONE, const void* d_base = nullptr)
{
    if (int rc = zsk_planes_check(ctx && (!size || (d_src && d_dst)), size, k, frameSize, b.err, filter, d_base != nullptr)) return rc;
    if (!size) return 0;
    ZskJoinArgs a; memset(&a, 0, sizeof a);
    a.planar = (const uint8_t*)d_src; a.dst = (uint8_t*)d_dst; a.elements = size / k; a.k = k; a.group = frameSize; a.tiles = zsk_planes_tiles(a.elements, frameSize);
    if (filter == ZSK_FILTER_XOR_BASE) { zsk_launch_join_xor(b, a, d_base, nullptr); return b.check(); }
    uint8_t* sums = nullptr;
    if (filter == ZSK_FILTER_DELTA) if (int rc = b.reserve_typed(ZSKT_A_TILESUMS, (size_t)a.tiles * 8, &sums)) return rc;
    zsk_launch_join(b, filter, a, zsk_frame_count(a.elements, frameSize), sums);
    return b.check();
}
template <class B> int zsk_planes_join_base(B& b, bool ctx, const void* d_src, uint64_t size, uint32_t k, uint32_t frameSize, const void* d_base, void* d_dst)
{
    if (int rc = zsk_base_check("planes join", d_base, size, k, d_dst, size, b.err)) return rc;
    return zsk_planes_join(b, ctx, d_src, size, k, frameSize, d_dst, ZSK_FILTER_XOR_BASE, d_base);
}

// Typed compress: the split kernel writes the planar staging buffer and the plane frames' records; the records call compresses them as they are; the seal
// puts the marker in. The records call is handed the capacity less the marker and its entry, so a stream that does not fit fails there (70) with nothing written
template <class B> int zsk_typed_compress(B& b, bool ctx, const void* d_src, uint64_t srcSize, uint32_t frameSize, uint32_t k, int flags, void* d_dst, uint64_t dstCapacity,
                                          uint64_t* d_streamSize, int32_t* d_status, uint32_t filter = ZSK_FILTER_NONE, const void* d_base = nullptr)
{
    if (k == 1 && filter != ZSK_FILTER_NONE) return zsk_refuse(b.err, ZHIP_ERR_UNSUPPORTED, zsk_filter_ok(filter) && filter != ZSK_FILTER_XOR_BASE ? "seekable typed compress: a filter needs an element size of 2, 4 or 8" : "seekable typed compress: the filter must be 0 (none) or 1 (delta)");
    if (k == 1) return zsk_compress(b, ctx, d_src, srcSize, frameSize, flags, d_dst, dstCapacity, d_streamSize, d_status);
    if (int rc = zsk_typed_compress_check(ctx && d_streamSize && d_status && (!srcSize || d_src), srcSize, frameSize, k, flags, b.err, filter, d_base != nullptr)) return rc;
    const int checksum = flags & ZHIP_SEEKABLE_CHECKSUM ? 1 : 0;
    const uint64_t elements = srcSize / k, nGroups = zsk_frame_count(elements, frameSize), n = nGroups * k;
    uint8_t* staging = nullptr; uint8_t* records = nullptr; uint8_t* stash = nullptr;
    if (srcSize) if (int rc = b.reserve_typed(ZSKT_A_STAGING, (size_t)srcSize, &staging)) return rc;
    if (n) if (int rc = b.reserve_typed(ZSKT_A_RECORDS, (size_t)n * 16, &records)) return rc;
    if (int rc = b.reserve_typed(ZSKT_A_STASH, (size_t)zsk_seal_stash_bytes(n, checksum), &stash)) return rc;
    if (n) {
        zsk_launch_split(b, filter, zsk_split_args(d_src, srcSize, k, frameSize, staging, d_base, records), zsk_tile_grid(b.numCU, zsk_planes_tiles(elements, frameSize), n));
        if (int rc = b.check()) return rc;
    }
    const uint64_t extra = ZSK_MARKER + zsk_entry_size(checksum);
    if (int rc = zsk_compress_records(b, ctx, staging, srcSize, (const zhip_segment*)records, (size_t)n, srcSize, elements < frameSize ? elements : frameSize, flags,
                                      d_dst, dstCapacity > extra ? dstCapacity - extra : 0, d_streamSize, d_status)) return rc;
    ZskSealArgs s; memset(&s, 0, sizeof s);
    s.dst = (uint8_t*)d_dst; s.dstCapacity = dstCapacity; s.streamSize = d_streamSize; s.outStatus = d_status; s.stash = stash;
    s.n = (uint32_t)n; s.checksum = (uint32_t)checksum; s.elementSize = k | (filter << 8); s.frameSize = frameSize;
    const uint32_t grid = zsk_lane_grid(b.numCU, n * zsk_entry_size(checksum) / 16 + 1);
    b.launch_typed(ZSKT_K_SEAL_STASH, grid, &s);
    b.launch_typed(ZSKT_K_SEAL, grid, &s);
    return b.check();
}

// the same with the xor-with-base filter: the base is srcSize bytes and may not share a byte with the output
template <class B> int zsk_typed_compress_base(B& b, bool ctx, const void* d_src, uint64_t srcSize, uint32_t frameSize, uint32_t k, const void* d_base, int flags, void* d_dst,
                                               uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status)
{
    if (int rc = zsk_base_check("seekable typed compress", d_base, srcSize, k, d_dst, dstCapacity, b.err)) return rc;
    return zsk_typed_compress(b, ctx, d_src, srcSize, frameSize, k, flags, d_dst, dstCapacity, d_streamSize, d_status, ZSK_FILTER_XOR_BASE, d_base);
}

// Behind zsk_open: a last entry of (24, 0) is looked at -- the one extra copy, and only then. No tag: a plain stream. A tag and the shape it promises:
// a typed stream. A tag and anything else (a version, an element size or a filter this reader does not know, frames that are no groups of planes): corrupt, at the
// first frame that does not fit
template <class B> int zsk_typed_probe(B& b, ZskTypedOpened* h, int* zerr, size_t* index)
{
    h->elementSize = 1; h->groupElements = 0; h->filter = ZSK_FILTER_NONE;
    const uint32_t n = h->lay.n;
    if (!n || h->cOff[n] - h->cOff[n - 1] != ZSK_MARKER || h->dOff[n] != h->dOff[n - 1]) return 0;
    uint8_t m[ZSK_MARKER];
    if (b.copy(m, h->stream + h->cOff[n - 1], ZSK_MARKER, ZSK_COPY_TO_HOST) || b.wait()) return zsk_refuse(b.err, ZHIP_ERR_HIP, "seekable open: reading the last frame failed");
    uint32_t k = 0, frameSize = 0, filter = 0;
    const int kind = zsk_parse_marker(m, &k, &frameSize, &filter);
    if (!kind) return 0;
    const uint32_t bad = kind < 0 ? n - 1 : zsk_typed_shape(h->dOff.data(), n, k, frameSize);
    if (bad != n) { *zerr = ZSK_ERR_CORRUPT; *index = bad; return ZHIP_ERR_ZSTD; }
    h->elementSize = k; h->groupElements = frameSize; h->filter = filter;
    return 0;
}

// the tables a typed read uploads: the join jobs of every pass, the user ranges' planar ranges, every planar range's place in the status area
// (C: the jobs' content offsets, the xor-with-base join's, J of them or none -- behind the rest, so that without them the layout is what it was)
struct ZskTypedReadLayout { size_t oJobs, oOwner, oPairAt, oContent, tableBytes; };
static inline ZskTypedReadLayout zsk_typed_read_layout(size_t J, size_t R, size_t Q, size_t C = 0)
{
    ZskTypedReadLayout l;
    l.oJobs = 0; l.oOwner = zsk_up16(J * sizeof(ZskJoinJob)); l.oPairAt = l.oOwner + zsk_up16(R * 8); l.oContent = l.oPairAt + zsk_up16(Q * 4); l.tableBytes = l.oContent + zsk_up16(C * 8);
    return l;
}

// THE read setup, of the typed read and of the chain read: the plan under `filter` from h's offsets and scratch limit, the tables' layout, every planar range's place
// in a status area of *statusInts ints (0 on entry), and the tables on the device at *t, uploaded through the pinned area. The other areas are the callers'
template <class B> int zsk_typed_read_setup(B& b, const ZskTypedOpened* h, const uint64_t* rg, size_t R, uint32_t filter, ZskTypedPlan* out, ZskTypedReadLayout* layout, size_t* statusInts, uint8_t** t)
{
    ZskTypedPlan& plan = *out; size_t& ints = *statusInts;
    zsk_typed_plan(h->dOff.data(), h->elementSize, h->groupElements, rg, R, h->scratchLimit, &plan, filter);
    const size_t J = plan.jobs.size(), Q = plan.planar.size() / 3;
    const ZskTypedReadLayout l = *layout = zsk_typed_read_layout(J, R, Q, plan.content.size());
    std::vector<uint32_t> pairAt(Q); uint8_t* pin = nullptr;
    for (const ZskTypedPass& p : plan.passes) { for (uint32_t q = p.q0; q < p.q1; q++) pairAt[q] = (uint32_t)(ints + 2 + 2 * (q - p.q0)); ints += 2 + 2 * (size_t)(p.q1 - p.q0); }
    if (int rc = b.reserve_typed(ZSKT_A_TABLES, l.tableBytes, t)) return rc;
    if (int rc = b.reserve(ZSK_A_PIN, l.tableBytes, &pin)) return rc;
    memcpy(pin + l.oJobs, plan.jobs.data(), J * sizeof(ZskJoinJob));
    memcpy(pin + l.oOwner, plan.owner.data(), R * 8);
    memcpy(pin + l.oPairAt, pairAt.data(), Q * 4);
    memcpy(pin + l.oContent, plan.content.data(), plan.content.size() * 8);
    return b.copy(*t, pin, l.tableBytes, ZSK_COPY_FROM_PIN);
}
// a pass's many-ranges statistics into the typed call's (`passes` is the typed call's own count)
static inline void zsk_add_stats(zhip_seekable_gather_stats* sum, const zhip_seekable_gather_stats& one) { if (sum) { sum->items += one.items; sum->inPlace += one.inPlace; sum->scratchBytes += one.scratchBytes; sum->copyJobs += one.copyJobs; } }

// R user ranges in element order: per pass of the plan the many-ranges call into the planar buffer and the join kernel (the handle's filter picks it: under
// delta the three launches of zsk_launch_join); then the status reducer.
// stats (where given) receives the sums over the passes' many-ranges calls, `passes` counting the typed passes.
// d_base: zsk_typed_ranges_base's, the base of an xor-with-base stream (checked there); such a stream is not read without one
template <class B> int zsk_typed_ranges(B& b, bool ctx, const ZskTypedOpened* h, const uint64_t* rg, size_t R, void* d_dst, uint64_t dstCapacity, int32_t* d_status,
                                        zhip_seekable_gather_stats* stats, size_t* bad, const void* d_base = nullptr)
{
    if (h && h->elementSize == 1) return zsk_refuse(b.err, ZHIP_ERR_UNSUPPORTED, "seekable typed ranges: the stream is a plain one (no byte planes)");
    if (h && h->filter == ZSK_FILTER_XOR_BASE && !d_base)
        return zsk_refuse(b.err, ZHIP_ERR_UNSUPPORTED, "seekable typed ranges: the stream's filter is xor with a base -- its elements need the base (the typed ranges call with a base)");
    bool any = false;
    if (int rc = zsk_ranges_check(ctx && h && d_status, rg, R, h ? h->contentSize : 0, d_dst, dstCapacity, bad, &any, b.err)) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    if (!any) return b.zero(d_status, (2 + 2 * R) * sizeof(int32_t));

    ZskTypedPlan plan; ZskTypedReadLayout l; size_t statusInts = 0; uint8_t* t = nullptr;
    if (int rc = zsk_typed_read_setup(b, h, rg, R, h->filter, &plan, &l, &statusInts, &t)) return rc;
    uint8_t* P = nullptr; uint8_t* st = nullptr;
    if (int rc = b.reserve_typed(ZSKT_A_PLANAR, (size_t)plan.pMax, &P)) return rc;
    if (int rc = b.reserve_typed(ZSKT_A_STATUS, statusInts * 4, &st)) return rc;
    uint8_t* sums = nullptr;
    if (h->filter == ZSK_FILTER_DELTA) {
        uint64_t most = 0;
        for (const ZskTypedPass& p : plan.passes) if (p.tiles > most) most = p.tiles;
        if (int rc = b.reserve_typed(ZSKT_A_TILESUMS, (size_t)most * 8, &sums)) return rc;
    }

    size_t at = 0;
    for (const ZskTypedPass& ps : plan.passes) {
        zhip_seekable_gather_stats one; size_t inner = 0;
        if (int rc = zsk_ranges(b, ctx, h, plan.planar.data() + 3 * (size_t)ps.q0, ps.q1 - ps.q0, P, ps.bytes, (int32_t*)st + at, &one, &inner)) return rc;
        at += 2 + 2 * (size_t)(ps.q1 - ps.q0);
        zsk_add_stats(stats, one);
        if (stats) stats->passes++;
        ZskJoinArgs a; memset(&a, 0, sizeof a);
        a.planar = P; a.dst = (uint8_t*)d_dst; a.jobs = (const ZskJoinJob*)(t + l.oJobs) + ps.job0; a.nJobs = ps.job1 - ps.job0; a.tiles = ps.tiles; a.k = h->elementSize; a.group = h->groupElements;
        if (h->filter == ZSK_FILTER_XOR_BASE) zsk_launch_join_xor(b, a, d_base, t + l.oContent + 8 * (size_t)ps.job0);
        else zsk_launch_join(b, h->filter, a, a.nJobs, sums);
        if (int rc = b.check()) return rc;
    }
    ZskTypedStatusArgs s; memset(&s, 0, sizeof s);
    s.owner = (const uint32_t*)(t + l.oOwner); s.pairAt = (const uint32_t*)(t + l.oPairAt); s.status = (const int32_t*)st; s.nRanges = (uint32_t)R; s.outStatus = d_status;
    b.launch_typed(ZSKT_K_TYPED_STATUS, zsk_lane_grid(b.numCU, R), &s);
    return b.check();
}

// The typed read of an xor-with-base stream: the base is the stream's element content, baseSize bytes of it, and shares no byte with the output. The stream
// does not name its base: another tensor of the right size gives wrong elements with status 0
template <class B> int zsk_typed_ranges_base(B& b, bool ctx, const ZskTypedOpened* h, const void* d_base, uint64_t baseSize, const uint64_t* rg, size_t R, void* d_dst, uint64_t dstCapacity,
                                             int32_t* d_status, zhip_seekable_gather_stats* stats, size_t* bad)
{
    if (!ctx || !h) return zsk_refuse(b.err, ZHIP_ERR_UNSUPPORTED, "seekable typed ranges: bad arguments");
    if (h->elementSize == 1) return zsk_refuse(b.err, ZHIP_ERR_UNSUPPORTED, "seekable typed ranges: the stream is a plain one (no byte planes)");
    if (h->filter != ZSK_FILTER_XOR_BASE) return zsk_refuse(b.err, ZHIP_ERR_UNSUPPORTED, "seekable typed ranges: the stream's filter is not xor with a base -- it is read without one");
    if (baseSize != h->contentSize && d_base) return zsk_refuse(b.err, ZHIP_ERR_UNSUPPORTED, "seekable typed ranges: the base must have the size of the stream's content");
    if (int rc = zsk_base_check("seekable typed ranges", d_base, baseSize, h->elementSize, d_dst, dstCapacity, b.err)) return rc;
    return zsk_typed_ranges(b, ctx, h, rg, R, d_dst, dstCapacity, d_status, stats, bad, d_base);
}

// ------------------------------------------------------------------------------------------------ chains of xor-with-base links
// Version n of a tensor as [a full unfiltered stream, delta 1, ..., delta n], or as [delta 1, ..., delta n] and a base tensor, every delta an xor-with-base
// stream written against its predecessor. No link names its base or its predecessor: a chain in the wrong order, or with a link of another tensor of the
// same shape, reads back wrong elements with status 0. The message of a refusal names the link.
static inline int zsk_chain_refuse(std::string& err, const char* what, size_t link, const char* why)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: link %zu %s", what, link, why);
    return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, buf);
}
static inline int zsk_chain_count_check(const char* what, bool pointers, size_t nLinks, std::string& err)
{
    char buf[160];
    if (nLinks < 1 || nLinks > ZSK_CHAIN_MAX) { snprintf(buf, sizeof buf, "%s: a chain has 1 ... %u links, not %zu", what, ZSK_CHAIN_MAX, nLinks); return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, buf); }
    if (!pointers) { snprintf(buf, sizeof buf, "%s: bad arguments", what); return zsk_refuse(err, ZHIP_ERR_UNSUPPORTED, buf); }
    return 0;
}

// The chain join on its own: nLinks whole planar buffers of `size` bytes with the layout of zsk_planes_split's, XORed, joined and XORed with the base where
// one is given (d_base may be NULL) -- one launch on the plain join's grid
template <class B> int zsk_planes_join_chain(B& b, bool ctx, const void* const* d_planar, size_t nLinks, uint64_t size, uint32_t k, uint32_t frameSize, const void* d_base, void* d_dst)
{
    if (int rc = zsk_chain_count_check("planes join chain", ctx && d_planar, nLinks, b.err)) return rc;
    for (size_t i = 0; i < nLinks; i++) if (size && !d_planar[i]) return zsk_chain_refuse(b.err, "planes join chain", i, "is NULL");
    if (int rc = zsk_planes_check(!size || d_dst, size, k, frameSize, b.err)) return rc;
    if (d_base && zsk_overlap(d_base, size, d_dst, size)) return zsk_refuse(b.err, ZHIP_ERR_UNSUPPORTED, "planes join chain: the base overlaps the output");
    if (!size) return 0;
    ZskJoinChainArgs x; memset(&x, 0, sizeof x);
    ZskJoinArgs& a = x.j;
    a.planar = (const uint8_t*)d_planar[0]; a.dst = (uint8_t*)d_dst; a.elements = size / k; a.k = k; a.group = frameSize; a.tiles = zsk_planes_tiles(a.elements, frameSize);
    for (size_t i = 0; i < nLinks; i++) x.planar[i] = (const uint8_t*)d_planar[i];
    x.nLinks = (uint32_t)nLinks; x.base = (const uint8_t*)d_base;
    b.launch_typed(ZSKT_K_PLANES_JOIN_CHAIN, zsk_tile_grid(b.numCU, a.tiles, 0), &x);
    return b.check();
}

// what a chain read refuses before anything is queued or written (the ranges' own refusals follow in the call)
static inline int zsk_chain_check(bool ctx, const ZskTypedOpened* const* links, size_t nLinks, const void* d_base, uint64_t baseSize, const void* d_dst, uint64_t dstCapacity, std::string& err)
{
    const char* const what = "seekable chain";
    if (int rc = zsk_chain_count_check(what, ctx && links, nLinks, err)) return rc;
    for (size_t i = 0; i < nLinks; i++) {
        if (!links[i]) return zsk_chain_refuse(err, what, i, "is NULL");
        for (size_t j = 0; j < i; j++) if (links[j] == links[i]) return zsk_chain_refuse(err, what, i, "is a handle that stands in the chain already (a link's planar buffer is its handle's)");
        if (links[i]->elementSize == 1) return zsk_chain_refuse(err, what, i, "is a plain stream (no byte planes)");
        if (links[i]->elementSize != links[0]->elementSize || links[i]->groupElements != links[0]->groupElements || links[i]->contentSize != links[0]->contentSize)
            return zsk_chain_refuse(err, what, i, "differs from link 0 in element size, group elements or content size");
        if (i == 0 && links[i]->filter == ZSK_FILTER_DELTA) return zsk_chain_refuse(err, what, i, "has the delta filter (a chain starts with an unfiltered stream, or with an xor-with-base stream and its base)");
        if (i > 0 && links[i]->filter != ZSK_FILTER_XOR_BASE) return zsk_chain_refuse(err, what, i, "is not an xor-with-base stream (every link behind the first is one)");
    }
    if (links[0]->filter == ZSK_FILTER_XOR_BASE && !d_base) return zsk_chain_refuse(err, what, 0, "is an xor-with-base stream: the chain needs its base");
    if (links[0]->filter == ZSK_FILTER_NONE && d_base) return zsk_chain_refuse(err, what, 0, "is an unfiltered stream: the chain takes no base");
    if (d_base && baseSize != links[0]->contentSize) return zsk_chain_refuse(err, what, 0, "has another content size than the base");
    if (d_base && zsk_overlap(d_base, baseSize, d_dst, dstCapacity)) return zsk_chain_refuse(err, what, 0, "has a base that overlaps the output");
    return 0;
}

// R user ranges of version nLinks - 1 (or nLinks, with a base) in one call. bs[i] is the backend over link i's handle: the many-ranges call of link i runs on
// it, unchanged, into THAT handle's planar area and a status area of its own; bs[0] also holds the call's tables and launches the join and the reducer.
// ONE plan, from link 0's offsets and scratch limit (all links of a chain have one decompressed layout); per pass nLinks many-ranges calls and one chain join;
// then the status reducer over all links' status areas. Every link holds at most the limit of planar scratch (or one piece above it), the chain nLinks times
// that. stats sums over all links' many-ranges calls, `passes` counting the typed passes once. d_link [1 + R] may be NULL.
template <class B> int zsk_typed_ranges_chain(B* const* bs, std::string& err, bool ctx, const ZskTypedOpened* const* links, size_t nLinks, const void* d_base, uint64_t baseSize,
                                              const uint64_t* rg, size_t R, void* d_dst, uint64_t dstCapacity, int32_t* d_status, int32_t* d_link, zhip_seekable_gather_stats* stats, size_t* bad)
{
    if (int rc = zsk_chain_check(ctx && bs, links, nLinks, d_base, baseSize, d_dst, dstCapacity, err)) return rc;
    const ZskTypedOpened* const h = links[0];
    bool any = false;
    if (int rc = zsk_ranges_check(d_status != nullptr, rg, R, h->contentSize, d_dst, dstCapacity, bad, &any, err)) return rc;
    B& b = *bs[0];
    if (stats) memset(stats, 0, sizeof *stats);
    ZskTypedStatusChainArgs s; memset(&s, 0, sizeof s);
    s.s.nRanges = (uint32_t)R; s.s.outStatus = d_status; s.outLink = d_link;
    if (!any) {                                    // nothing to read: zeros, and no link anywhere (the reducer over no links writes exactly that)
        if (!d_link) return b.zero(d_status, (2 + 2 * R) * sizeof(int32_t));
        b.launch_typed(ZSKT_K_TYPED_STATUS_CHAIN, zsk_lane_grid(b.numCU, R), &s);
        return b.check();
    }

    ZskTypedPlan plan; ZskTypedReadLayout l; size_t statusInts = 0; uint8_t* t = nullptr;
    if (int rc = zsk_typed_read_setup(b, h, rg, R, d_base ? ZSK_FILTER_XOR_BASE : ZSK_FILTER_NONE, &plan, &l, &statusInts, &t)) return rc;
    uint8_t* P[ZSK_CHAIN_MAX]; uint8_t* st[ZSK_CHAIN_MAX];
    for (size_t i = 0; i < nLinks; i++) {
        if (int rc = bs[i]->reserve_typed(ZSKT_A_PLANAR, (size_t)plan.pMax, &P[i])) return rc;
        if (int rc = bs[i]->reserve_typed(ZSKT_A_STATUS, statusInts * 4, &st[i])) return rc;
    }

    size_t at = 0;
    for (const ZskTypedPass& ps : plan.passes) {
        for (size_t i = 0; i < nLinks; i++) {
            zhip_seekable_gather_stats one; size_t inner = 0;
            if (int rc = zsk_ranges(*bs[i], ctx, links[i], plan.planar.data() + 3 * (size_t)ps.q0, ps.q1 - ps.q0, P[i], ps.bytes, (int32_t*)st[i] + at, &one, &inner)) return rc;
            zsk_add_stats(stats, one);
        }
        at += 2 + 2 * (size_t)(ps.q1 - ps.q0);
        if (stats) stats->passes++;
        ZskJoinChainArgs x; memset(&x, 0, sizeof x);
        ZskJoinArgs& a = x.j;
        a.planar = P[0]; a.dst = (uint8_t*)d_dst; a.jobs = (const ZskJoinJob*)(t + l.oJobs) + ps.job0; a.nJobs = ps.job1 - ps.job0; a.tiles = ps.tiles; a.k = h->elementSize; a.group = h->groupElements;
        for (size_t i = 0; i < nLinks; i++) x.planar[i] = P[i];
        x.nLinks = (uint32_t)nLinks; x.base = (const uint8_t*)d_base; x.content = d_base ? (const uint64_t*)(t + l.oContent) + ps.job0 : nullptr;
        b.launch_typed(ZSKT_K_PLANES_JOIN_CHAIN, zsk_tile_grid(b.numCU, ps.tiles, 0), &x);
        if (int rc = b.check()) return rc;
    }
    s.s.owner = (const uint32_t*)(t + l.oOwner); s.s.pairAt = (const uint32_t*)(t + l.oPairAt);
    for (size_t i = 0; i < nLinks; i++) s.status[i] = (const int32_t*)st[i];
    s.nLinks = (uint32_t)nLinks;
    b.launch_typed(ZSKT_K_TYPED_STATUS_CHAIN, zsk_lane_grid(b.numCU, R), &s);
    return b.check();
}
