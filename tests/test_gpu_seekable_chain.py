"""Chains of xor-with-base links on the GPU (include/zstd_hip.h, "CHAINS of xor-with-base streams"): the chain join kernel against the numpy
model of tests/chain_model.py, SeekableChain end to end on chains written with seekable_compress(base=) under the default, literals-only and auto finders, one
damaged plane frame in a middle link, the refusals, one context alternating plain, delta, base and chain reads on the same handles, and the host-bytes
functions. All of it fails on a build without the feature: the calls, the class and the kernel do not exist there."""
import numpy as np
import pytest

from tests import chain_model as cm
from tests import xor_model as xm

pytestmark = pytest.mark.gpu

GUARD = 64
ELEMENTS = {1025: 3 * 1025 + 37, 4096: 3 * 4096 + 37}
FINDERS = ["libzstd", "none", "auto"]


@pytest.fixture(scope="module")
def zstd():
    import torch
    import zstandard_amd as z
    import zstandard_amd.device  # noqa: F401
    import zstandard_amd.seekable  # noqa: F401
    assert torch.cuda.is_available()
    return z


@pytest.fixture(scope="module")
def ctx(zstd):
    c = zstd.device.DeviceBatchContext(level=3)
    yield c
    c.close()


@pytest.fixture(scope="module")
def writers(zstd, ctx):
    """a context per match finder (the default one is `ctx`)"""
    cs = {"libzstd": ctx, "none": zstd.device.DeviceBatchContext(level=3, match_finder="none"), "auto": zstd.device.DeviceBatchContext(level=3, match_finder="auto")}
    yield cs
    cs["none"].close(); cs["auto"].close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _host(t):
    return t.cpu().numpy()


def _ranges(k, frame, elements):
    """the range set of tests/test_gpu_seekable_xor_base.py"""
    g, size = frame * k, elements * k
    rg = [(1, 2), (3, k + 2), (100, 999), (g - 5, 11), (g - 3, 2 * g + 9), (50, 0), (100, 999), (500, 2000), (0, size), (size - 3, 3), (g, g), (0, 1), (size, 0), (2 * g + 2, g + 37 * k - 2)]
    return [(o, min(n, size - o)) for o, n in rg]


def _guarded_dev(n, off, fill):
    import torch
    hold = torch.full((n + 2 * GUARD + 1,), fill, dtype=torch.uint8, device="cuda")
    return hold, hold[GUARD + off:GUARD + off + n]


def _guards_intact(hold, n, off, fill):
    h = _host(hold)
    return (h[:GUARD + off] == fill).all() and (h[GUARD + off + n:] == fill).all()


def _write_chain(writer, vs, k, frame, full, checksum=False):
    """the streams that store vs[-1]: (device stream tensors oldest first, the reader's base on the device or None)"""
    sources, base = cm.link_sources(vs, full)
    streams = [writer.seekable_compress(_dev(data), frame_size=frame, element_size=k, checksum=checksum, base=None if b is None else _dev(b)) for data, b in sources]
    return streams, (None if base is None else _dev(base))


# ------------------------------------------------------------------------------------------------ the kernel on its own
@pytest.mark.parametrize("k", [2, 4, 8])
def test_planes_join_chain(zstd, ctx, k):
    """every group size at which the body takes another path with last groups of 1, 15 and 17 elements, 1, 2, 3 and 16 links, with and without a base, tensor
    views at byte offsets 0 and 1, guard bytes around the output; the inputs are unchanged"""
    import torch
    n_case = 0
    for m in xm.GROUP_SIZES:
        for last in xm.LAST_GROUPS:
            if last > m:
                continue
            elements = 2 * m + last
            size = elements * k
            for n_links in cm.LINK_COUNTS:
                data = cm.random_planars(k, elements, n_links, seed=1000 * k + m + n_links)
                off = n_case % 2; n_case += 1
                held = [_guarded_dev(size, (off + i) % 2, 0x5A) for i in range(n_links)]
                for (_, view), d in zip(held, data):
                    view.copy_(torch.from_numpy(d))
                base = xm.source(k, elements, seed=m + last)
                b_hold, b = _guarded_dev(size, 1 - off, 0x5A); b.copy_(torch.from_numpy(base))
                for with_base in (False, True):
                    out_hold, out = _guarded_dev(size, 1 - off, 0xC7)
                    got = ctx.planes_join_chain([v for _, v in held], m, k, out=out, base=b if with_base else None)
                    assert (_host(got) == cm.join_chain(data, base if with_base else None, k, m)).all(), (k, m, last, n_links, with_base)
                    assert _guards_intact(out_hold, size, 1 - off, 0xC7)
                assert all((_host(v) == d).all() and _guards_intact(h, size, (off + i) % 2, 0x5A) for i, ((h, v), d) in enumerate(zip(held, data)))
                assert (_host(b) == base).all() and _guards_intact(b_hold, size, 1 - off, 0x5A)


def test_planes_join_chain_more_tiles_than_waves(zstd, ctx):
    """twice the launch's waves plus one tile in ONE group: the grid-stride loop's later trips; the module function; one link equals planes_join(base=)"""
    import torch
    waves = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    k = 4
    m = (2 * waves + 1) * 1024 + 5
    data = cm.random_planars(k, m, 3, seed=3)
    base = xm.source(k, m, seed=4)
    dev = [_dev(d) for d in data]; b = _dev(base)
    assert (_host(zstd.device.planes_join_chain(dev, m, k, ctx=ctx, base=b)) == cm.join_chain(data, base, k, m)).all()
    assert (_host(zstd.device.planes_join_chain(dev[:2], m, k, ctx=ctx)) == cm.join_chain(data[:2], None, k, m)).all()
    assert torch.equal(ctx.planes_join_chain(dev[:1], m, k, base=b), ctx.planes_join(dev[0], m, k, base=b))
    assert torch.equal(ctx.planes_join_chain(dev[:1], m, k), ctx.planes_join(dev[0], m, k))


# ------------------------------------------------------------------------------------------------ the chain end to end
@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("frame", [1025, 4096])
def test_chain_end_to_end(zstd, ctx, writers, k, frame):
    """[full, d1, d2, d3] and [d1, d2, d3] + base, written under the three finders: a whole read and every range equal the slice of the LAST version, also on a
    caller's stream and under a scratch limit of one group (several passes); guard bytes around `out` stay; a one-link chain equals
    SeekableStream(base=).read_ranges byte for byte"""
    import torch
    elements = ELEMENTS[frame]
    vs = cm.versions(k, elements, 3, seed=40 + k)
    last = vs[-1]
    rg = _ranges(k, frame, elements)
    total = sum(n for _, n in rg)
    side = torch.cuda.Stream()
    for finder in FINDERS:
        for full in (True, False):
            streams, base = _write_chain(writers[finder], vs, k, frame, full)
            with zstd.device.SeekableChain(ctx, streams, base=base) as chain:
                assert (chain.element_size, chain.group_elements, chain.content_size, len(chain.links)) == (k, frame, last.size, 4 if full else 3)
                assert (_host(chain.read()) == last).all(), (finder, full)
                for (o, n), v in zip(rg, chain.read_ranges(rg)):
                    assert _host(v).tobytes() == last[o:o + n].tobytes(), (finder, full, o, n)
                assert chain.last_gather_stats["passes"] == 1
                if finder != "libzstd":
                    continue
                # under a scratch limit of one group, into a guarded destination, on a caller's stream
                chain.set_scratch_limit(frame * k)
                hold, out = _guarded_dev(total, 1, 0xC7)
                offsets = np.cumsum([0] + [n for _, n in rg[:-1]]).tolist()
                side.wait_stream(torch.cuda.current_stream())
                views = chain.read_ranges(rg, out=out, out_offsets=offsets, stream=side)
                side.synchronize()
                assert chain.last_gather_stats["passes"] > 1
                for (o, n), v in zip(rg, views):
                    assert _host(v).tobytes() == last[o:o + n].tobytes(), (full, o, n)
                assert _guards_intact(hold, total, 1, 0xC7)
                assert _host(chain.read(7, 1001, stream=side)).tobytes() == last[7:1008].tobytes()
            if base is not None:
                assert (_host(base) == vs[0]).all()
    # one link: the single-stream read, byte for byte
    d3 = ctx.seekable_compress(_dev(vs[3]), frame_size=frame, element_size=k, base=_dev(vs[2]))
    b = _dev(vs[2])
    with zstd.device.SeekableStream(ctx, d3, base=b) as st, zstd.device.SeekableChain(ctx, [d3], base=b) as chain:
        want = st.read_ranges(rg)
        got = chain.read_ranges(rg)
        assert all(torch.equal(a, c) for a, c in zip(want, got)) and chain.last_gather_stats == st.last_gather_stats
        assert all(_host(v).tobytes() == vs[3][o:o + n].tobytes() for (o, n), v in zip(rg, got))
    full_stream = ctx.seekable_compress(_dev(vs[0]), frame_size=frame, element_size=k)
    with zstd.device.SeekableStream(ctx, full_stream) as st, zstd.device.SeekableChain(ctx, [st]) as chain:      # (an open SeekableStream as a link)
        assert all(torch.equal(a, c) for a, c in zip(st.read_ranges(rg), chain.read_ranges(rg)))
        with chain.extended(ctx.seekable_compress(_dev(vs[1]), frame_size=frame, element_size=k, base=_dev(vs[0]))) as longer:
            assert len(longer.links) == 2 and (_host(longer.read()) == vs[1]).all()
        assert (_host(st.read()) == vs[0]).all()                              # the caller's link stays open behind the chains


# ------------------------------------------------------------------------------------------------ damage
def test_one_damaged_plane_frame_in_a_middle_link(zstd, ctx):
    """with checksum=True: one flipped content byte in plane frame 8 (group 2, plane 0) of link 2 of [full, d1, d2, d3] -- d2's plane 0 is incompressible, so
    the byte is a raw literal -- fails with 22 exactly the ranges that need group 2, naming link 2 and frame 8; the others are right. Python raises, naming
    the link"""
    import torch
    k, frame = 4, 1025
    elements = ELEMENTS[frame]
    v0 = xm.source(k, elements, seed=8)
    v1 = xm.base_of("low_bits", v0, k, seed=1)
    v2 = v1.copy(); v2[::k] = np.random.default_rng(9).integers(0, 256, elements, dtype=np.uint8)
    v3 = xm.base_of("low_bits", v2, k, seed=2)
    vs = [v0, v1, v2, v3]
    streams, _ = _write_chain(ctx, vs, k, frame, True, checksum=True)
    from tests import seekable_cases as sc
    raw = _host(streams[2]).tobytes()
    entries, ck, _ = sc.parse(raw)
    assert ck
    bad = bytearray(raw)
    bad[sum(e[0] for e in entries[:8]) + entries[8][0] // 2] ^= 0x55
    streams[2] = torch.frombuffer(bad, dtype=torch.uint8).cuda()
    g = frame * k
    rg = [(10, 100), (2 * g - 3, 5), (2 * g, g), (3 * g, 37 * k), (0, v3.size), (3 * g - 1, 1), (3 * g, 1), (g + 1, g - 1), (2 * g + 8, 0)]
    touches = [o < 3 * g and o + ln > 2 * g and ln > 0 for o, ln in rg]
    with zstd.device.SeekableChain(ctx, streams) as chain:
        table = np.zeros((len(rg), 3), dtype=np.uint64)
        at = 0
        for i, (o, ln) in enumerate(rg):
            table[i] = (o, ln, at); at += ln
        dst = torch.zeros(at, dtype=torch.uint8, device="cuda")
        status = torch.zeros(2 + 2 * len(rg), dtype=torch.int32, device="cuda"); link = torch.full((1 + len(rg),), -7, dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream()
        import ctypes as C
        handles = (C.c_void_p * 4)(*[x.handle.value for x in chain.links])
        rc = ctx.L.zhip_seekable_decompress_typed_ranges_chain_device(ctx.ctx, handles, 4, None, 0, table.ctypes.data, len(rg), dst.data_ptr(), at, status.data_ptr(), link.data_ptr(), None,
                                                                      s.cuda_stream)
        assert rc == 0
        s.synchronize()
        status, link, got = status.cpu().tolist(), link.cpu().tolist(), _host(dst)
        assert status[:2] == [22, 1] and link[0] == 2
        for r, ((o, ln), touch) in enumerate(zip(rg, touches)):
            assert status[2 + 2 * r:4 + 2 * r] == ([22, 8] if touch else [0, 0]) and link[1 + r] == (2 if touch else -1), r
            if not touch:
                assert got[int(table[r, 2]):int(table[r, 2]) + ln].tobytes() == v3[o:o + ln].tobytes(), r
        with pytest.raises(zstd.ZstdError, match="link 2: frame 8"):
            chain.read(2 * g, 10)
        assert _host(chain.read(10, 100)).tobytes() == v3[10:110].tobytes()


# ------------------------------------------------------------------------------------------------ the refusals
def test_refusals(zstd, ctx):
    """mixed element sizes, delta as link 0, a plain stream as a link, 17 links, a missing base and a superfluous base raise ZstdError that names the link;
    through the C call: UNSUPPORTED (6), the destination and the status words untouched"""
    import ctypes as C
    import torch
    k, frame, elements = 4, 8, 20
    vs = cm.versions(k, elements, 2, seed=1)
    t = [_dev(v) for v in vs]
    full = ctx.seekable_compress(t[0], frame_size=frame, element_size=k)
    d1 = ctx.seekable_compress(t[1], frame_size=frame, element_size=k, base=t[0])
    d2 = ctx.seekable_compress(t[2], frame_size=frame, element_size=k, base=t[1])
    d1_k2 = ctx.seekable_compress(t[1], frame_size=2 * frame, element_size=2, base=t[0])
    delta = ctx.seekable_compress(t[0], frame_size=frame, element_size=k, filter="delta")
    plain = ctx.seekable_compress(t[0], frame_size=frame * k)
    Chain = zstd.device.SeekableChain
    for links, base, word in (([full, d1_k2], None, "link 1"), ([delta, d1], None, "link 0"), ([full, plain], None, "link 1"), ([full] + [d1] * 16, None, "16 links"),
                              ([d1, d2], None, "link 0"), ([full, d1], t[0], "link 0"), ([full, full], None, "link 1"), ([], None, "links"), ([d1, d2], t[0][:-k], "base")):
        with pytest.raises(zstd.ZstdError, match=word):
            Chain(ctx, links, base=base)
    with zstd.device.SeekableStream(ctx, d1) as st:
        with pytest.raises(zstd.ZstdError, match="link 2"):
            Chain(ctx, [full, st, st])                                          # the same handle twice
        dst = torch.full((256,), 0x5A, dtype=torch.uint8, device="cuda")
        status = torch.full((4,), -1, dtype=torch.int32, device="cuda"); link = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        table = np.array([[2, 40, 0]], dtype=np.uint64)
        s = torch.cuda.current_stream().cuda_stream
        L = ctx.L
        one = (C.c_void_p * 1)(st.handle.value)
        for base_ptr, base_size, word in ((None, 0, b"needs its base"), (t[0].data_ptr(), elements * k - k, b"content size"), (dst.data_ptr() + 200, elements * k, b"overlaps")):
            assert L.zhip_seekable_decompress_typed_ranges_chain_device(ctx.ctx, one, 1, base_ptr, base_size, table.ctypes.data, 1, dst.data_ptr(), 256, status.data_ptr(), link.data_ptr(), None, s) == 6
            assert word in L.zhip_last_error() and b"link 0" in L.zhip_last_error()
        assert L.zhip_seekable_decompress_typed_ranges_chain_device(ctx.ctx, one, 0, None, 0, table.ctypes.data, 1, dst.data_ptr(), 256, status.data_ptr(), link.data_ptr(), None, s) == 6
        assert L.zhip_seekable_decompress_typed_ranges_chain_device(ctx.ctx, one, 17, None, 0, table.ctypes.data, 1, dst.data_ptr(), 256, status.data_ptr(), link.data_ptr(), None, s) == 6
        none = (C.c_void_p * 1)(None)
        assert L.zhip_seekable_decompress_typed_ranges_chain_device(ctx.ctx, none, 1, None, 0, table.ctypes.data, 1, dst.data_ptr(), 256, status.data_ptr(), link.data_ptr(), None, s) == 6
        assert b"link 0 is NULL" in L.zhip_last_error()
        two = (C.c_void_p * 2)(t[0].data_ptr(), None)
        assert L.zhip_planes_join_chain_device(ctx.ctx, two, 2, elements * k, k, frame, None, dst.data_ptr(), s) == 6 and b"link 1" in L.zhip_last_error()
        assert L.zhip_planes_join_chain_device(ctx.ctx, two, 17, elements * k, k, frame, None, dst.data_ptr(), s) == 6
        torch.cuda.synchronize()
        assert (_host(dst) == 0x5A).all() and status.tolist() == [-1] * 4 and link.tolist() == [-7] * 2
    for call in (lambda: ctx.planes_join_chain([], frame, k), lambda: ctx.planes_join_chain([t[0]] * 17, frame, k), lambda: ctx.planes_join_chain([t[0], t[1][:-k]], frame, k),
                 lambda: ctx.planes_join_chain([t[0], t[1]], frame, 3), lambda: ctx.planes_join_chain([t[0]], frame, k, base=t[1][:-k]),
                 lambda: ctx.planes_join_chain([t[0]], frame, k, out=t[1], base=t[1])):
        with pytest.raises(zstd.ZstdError):
            call()


# ------------------------------------------------------------------------------------------------ one context, every read
def test_one_context_alternating_reads(zstd, ctx):
    """plain (raw), delta, base and chain reads alternate on ONE context over the SAME open handles, twice: each call's result is what it is alone -- nothing
    of one call (a handle's planar area, its tables, its status arrays) leaks into the next"""
    k, frame = 4, 1025
    elements = ELEMENTS[frame]
    vs = cm.versions(k, elements, 3, seed=31)
    t = [_dev(v) for v in vs]
    streams, _ = _write_chain(ctx, vs, k, frame, True)
    delta = ctx.seekable_compress(t[0], frame_size=frame, element_size=k, filter="delta")
    rg = _ranges(k, frame, elements)
    S = zstd.device.SeekableStream
    with S(ctx, streams[0]) as s0, S(ctx, streams[1], base=t[0]) as s1, S(ctx, streams[2], base=t[1]) as s2, S(ctx, streams[3], base=t[2]) as s3, S(ctx, delta) as sd, \
            S(ctx, streams[2], raw=True) as raw2:
        with zstd.device.SeekableChain(ctx, [s0, s1, s2, s3], scratch_limit=5000) as chain, zstd.device.SeekableChain(ctx, [s1, s2], base=t[0]) as short:
            planar2 = xm.split(vs[2], vs[1], k, frame)
            for name in ("chain", "base", "plain", "short", "delta", "chain", "delta", "short", "base", "plain", "chain"):
                if name == "plain":
                    assert (_host(raw2.read()) == planar2).all()
                    continue
                reader, want = {"chain": (chain, vs[3]), "short": (short, vs[2]), "base": (s2, vs[2]), "delta": (sd, vs[0])}[name]
                for (o, n), v in zip(rg, reader.read_ranges(rg)):
                    assert _host(v).tobytes() == want[o:o + n].tobytes(), (name, o, n)
    assert all((_host(a) == b).all() for a, b in zip(t, vs))


# ------------------------------------------------------------------------------------------------ host bytes
def test_host_bytes(zstd):
    """seekable.decompress_chain / decompress_ranges_chain on bytes, streams written by seekable.compress: the last version's slices"""
    k, frame = 2, 1025
    elements = ELEMENTS[frame]
    vs = [v.tobytes() for v in cm.versions(k, elements, 2, seed=5)]
    zs = zstd.seekable
    full = zs.compress(vs[0], frame_size=frame, element_size=k)
    d1 = zs.compress(vs[1], frame_size=frame, element_size=k, base=vs[0])
    d2 = zs.compress(vs[2], frame_size=frame, element_size=k, base=vs[1])
    rg = [(o, n) for o, n in _ranges(k, frame, elements)]
    want = [vs[2][o:o + n] for o, n in rg]
    assert zs.decompress_ranges_chain([full, d1, d2], rg) == want
    assert zs.decompress_ranges_chain([d1, d2], rg, base=vs[0]) == want
    assert zs.decompress_chain([full, d1, d2]) == vs[2] and zs.decompress_chain([d1, d2], 5, 100, base=vs[0]) == vs[2][5:105]
    assert zs.decompress_chain([full, d1]) == vs[1] and zs.decompress_chain([full]) == vs[0]
    assert zs.decompress_ranges_chain([full, d1, d2], []) == []
    planars = [np.frombuffer(zs.elements_to_planes(vs[0], k, frame), dtype=np.uint8), np.frombuffer(zs.elements_to_planes(vs[1], k, frame, base=vs[0]), dtype=np.uint8),
               np.frombuffer(zs.elements_to_planes(vs[2], k, frame, base=vs[1]), dtype=np.uint8)]
    assert cm.join_chain(planars, None, k, frame).tobytes() == vs[2]          # (the model, on the host module's planes)
    for streams, base in (([d1, d2], None), ([full, d1], vs[0]), ([full, b""], None), ([full, d2, d1, d1, full][:0], None)):
        with pytest.raises(zstd.ZstdError):
            zs.decompress_chain(streams, base=base)
