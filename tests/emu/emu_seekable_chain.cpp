// tests/emu/emu_seekable_chain.cpp -- chains of xor-with-base links on the host wave emulator: the chain join body, the status reducer over
// several links, and the whole calls of zhip_seekable_typed_calls.hpp -- zsk_planes_join_chain, zsk_typed_ranges_chain -- over one emulator backend per link.
// emu_seekable_xor_base.cpp is included as it is (the way xor_planes_main.cpp includes it), so the entries of before -- emu_xor_join, emu_planes_join,
// emu_xor_compress, emu_delta_compress, ... -- are in this library too: what they return is compared with what the entries here return. Test infrastructure
// only (tests/test_emu_seekable_chain.py; tests/emu/chain_planes_main.cpp is the stand-alone sanitizer program over the same functions).
#include "emu_seekable_xor_base.cpp"

// ------------------------------------------------------------------------------------------------ the body alone
// the chain join on `grid` workgroups over nLinks planar buffers of one layout: jobs [nJobs][6] = planar, m, dst, h, t, content -- or, with jobs NULL, the
// groups of a whole buffer of `size` bytes. base: NULL, or the pointer the kernel adds the content offsets to
extern "C" void emu_chain_join(const uint8_t* const* planars, uint32_t nLinks, const uint8_t* base, uint8_t* dst, const uint64_t* jobs, uint32_t nJobs, uint64_t size, uint32_t k,
                               uint32_t group, uint32_t grid)
{
    std::vector<ZskJoinJob> js(nJobs);
    std::vector<uint64_t> content(nJobs);
    ZskJoinChainArgs x; memset(&x, 0, sizeof x);
    ZskJoinArgs& a = x.j;
    a.dst = dst; a.k = k; a.group = group; a.elements = size / k;
    for (uint32_t i = 0; i < nLinks; i++) x.planar[i] = planars[i];
    x.nLinks = nLinks; x.base = base;
    if (jobs) {
        for (uint32_t j = 0; j < nJobs; j++) {
            const uint64_t* q = jobs + 6 * j;
            js[j].planar = q[0]; js[j].m = q[1]; js[j].dst = q[2]; js[j].h = (uint32_t)q[3]; js[j].t = (uint32_t)q[4]; js[j].skip = 0; content[j] = q[5];
            js[j].tilePrefix = a.tiles; a.tiles += zsk_join_tiles(js[j].m);
        }
        a.jobs = js.data(); a.nJobs = nJobs; x.content = base ? content.data() : nullptr;      // (without a base the kernel may not read them)
    } else a.tiles = zsk_planes_tiles(a.elements, group);
    zhemu::run_grid(grid, planes_join_chain_lane, &x);
}

// the stand-alone call over the backend. baseMode 0: none, 1: `base`, 2: one that shares the destination's last byte. Returns the library's code;
// trace [cap], *traceWords = its words
extern "C" int emu_chain_planes_call(const uint8_t* const* planars, uint64_t nLinks, uint64_t size, uint32_t k, uint32_t group, const uint8_t* base, int baseMode, uint8_t* dst,
                                     uint32_t* trace, uint64_t cap, uint64_t* traceWords, char* text)
{
    EmuTypedBackend b;
    const uint8_t* const bp = baseMode == 0 ? nullptr : baseMode == 1 ? base : dst + (size ? size - 1 : 0);
    const int rc = zsk_planes_join_chain(b, true, (const void* const*)planars, (size_t)nLinks, size, k, group, bp, dst);
    *traceWords = copy_trace(b.trace, trace, (size_t)cap);
    if (text) snprintf(text, 256, "%s", b.text.c_str());
    return rc;
}

// ------------------------------------------------------------------------------------------------ the whole call
// A chain: the opened handles of its links, each with its backend (its areas, its trace), kept between calls as a caller keeps its handles
struct EmuChain { std::vector<std::unique_ptr<TypedOpened>> links; };
// streams [n] / sizes [n] -> the chain, or NULL (*bad = the link that did not open)
extern "C" void* emu_chain_open(const uint8_t* const* streams, const uint64_t* sizes, uint64_t n, uint64_t* bad)
{
    std::unique_ptr<EmuChain> c(new EmuChain());
    for (uint64_t i = 0; i < n; i++) {
        c->links.emplace_back(new TypedOpened());
        size_t index = 0;
        if (open_typed(streams[i], sizes[i], c->links.back().get(), &index)) { *bad = i; return nullptr; }
    }
    return c.release();
}
extern "C" void emu_chain_close(void* chain) { delete (EmuChain*)chain; }
// what link i's handle says: out[4] = element size, group elements, content size, filter
extern "C" void emu_chain_link_info(void* chain, uint64_t i, uint64_t* out)
{
    const TypedOpened& o = *((EmuChain*)chain)->links[(size_t)i];
    out[0] = o.elementSize; out[1] = o.groupElements; out[2] = o.contentSize; out[3] = o.filter;
}
// The chain read over `n` links: pick [n] names the handle of every link (an index into the chain's handles; -1: a NULL link), so a chain may be read in
// part, in another order, or with a handle twice. contents [handles]: every handle's PLANAR content (the decode stand-in's); codeFrames [handles]: the frame
// of that handle that reports `code` and writes nothing (-1: none). limit: the scratch limit set on every handle. outLink may be NULL.
// stats[8] = items, inPlace, scratchBytes, copyJobs, typed passes, the planar bytes link 0 holds, the rejected range's index, the planar bytes all links hold.
// traces [n][cap] / traceWords [n]: what every link's backend launched (the first link's holds the join and the reducer)
extern "C" int emu_chain_ranges(void* chain, const int64_t* pick, uint64_t n, const uint8_t* const* contents, const int64_t* codeFrames, int32_t code, const uint8_t* base, uint64_t baseSize,
                                const uint64_t* rg, uint64_t R, uint8_t* dst, uint64_t dstCapacity, uint64_t limit, int32_t* outStatus, int32_t* outLink, uint64_t* stats, uint32_t* traces,
                                uint64_t cap, uint64_t* traceWords, char* text)
{
    EmuChain& c = *(EmuChain*)chain;
    std::vector<const ZskTypedOpened*> hs; std::vector<EmuTypedBackend*> bs;
    for (size_t i = 0; i < c.links.size(); i++) {
        TypedOpened& o = *c.links[i];
        o.scratchLimit = limit;
        o.b.content = contents[i]; o.b.codeFrame = codeFrames[i]; o.b.code = code; o.b.trace.clear(); o.b.text.clear();
    }
    for (uint64_t i = 0; i < n; i++) {
        TypedOpened* const o = pick[i] < 0 ? nullptr : c.links[(size_t)pick[i]].get();
        hs.push_back(o); bs.push_back(o ? &o->b : nullptr);
    }
    memset(stats, 0, 8 * sizeof(uint64_t));
    zhip_seekable_gather_stats g; memset(&g, 0, sizeof g);
    size_t bad = 0;
    std::string err;
    const int rc = zsk_typed_ranges_chain(bs.data(), err, true, hs.data(), (size_t)n, base, baseSize, rg, (size_t)R, dst, dstCapacity, outStatus, outLink, &g, &bad);
    for (uint64_t i = 0; i < n; i++) traceWords[i] = bs[i] ? copy_trace(bs[i]->trace, traces + i * cap, (size_t)cap) : 0;
    for (size_t i = 0; i < c.links.size(); i++) { bool used = false; for (EmuTypedBackend* b : bs) used |= b == &c.links[i]->b; if (!used && !c.links[i]->b.trace.empty()) return -8; }
    if (text) snprintf(text, 256, "%s", err.c_str());
    stats[0] = g.items; stats[1] = g.inPlace; stats[2] = g.scratchBytes; stats[3] = g.copyJobs; stats[4] = g.passes; stats[6] = bad;
    if (!rc && n && bs[0]) stats[5] = bs[0]->typed[ZSKT_A_PLANAR].bytes;
    if (!rc) for (EmuTypedBackend* b : bs) stats[7] += b->typed[ZSKT_A_PLANAR].bytes;
    return rc;
}
// the single-stream typed read on handle i of the chain, with its base where its filter wants one: emu_xor_ranges / emu_typed_ranges on a handle that is kept
extern "C" int emu_chain_single(void* chain, uint64_t i, const uint8_t* content, const uint8_t* base, uint64_t baseSize, const uint64_t* rg, uint64_t R, uint8_t* dst, uint64_t dstCapacity,
                                uint64_t limit, int32_t* outStatus, uint64_t* stats, uint32_t* trace, uint64_t cap, uint64_t* traceWords)
{
    TypedOpened& o = *((EmuChain*)chain)->links[(size_t)i];
    o.scratchLimit = limit;
    EmuTypedBackend& b = o.b; b.content = content; b.codeFrame = -1; b.code = 0; b.trace.clear();
    zhip_seekable_gather_stats g; memset(&g, 0, sizeof g);
    size_t bad = 0;
    const int rc = base ? zsk_typed_ranges_base(b, true, &o, base, baseSize, rg, (size_t)R, dst, dstCapacity, outStatus, &g, &bad) : zsk_typed_ranges(b, true, &o, rg, (size_t)R, dst, dstCapacity, outStatus, &g, &bad);
    *traceWords = copy_trace(b.trace, trace, (size_t)cap);
    stats[0] = g.items; stats[1] = g.inPlace; stats[2] = g.scratchBytes; stats[3] = g.copyJobs; stats[4] = g.passes; stats[5] = b.typed[ZSKT_A_PLANAR].bytes; stats[6] = bad;
    return rc;
}
