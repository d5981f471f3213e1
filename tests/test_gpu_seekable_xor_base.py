"""The xor-with-base filter of typed seekable streams on the GPU (include/zstd_hip.h, "ZHIP_FILTER_XOR_BASE"): the split-with-xor and join-with-xor
kernels against the numpy model of tests/xor_model.py, seekable_compress(base=) with every plane frame compared with libzstd 1.5.7's frame of the model's plane
(tests/reflib.checker()), the marker, the reads with a base against slices of the source, the literals-only and auto finders, one damaged plane frame, the
refusals, and one context alternating plain, delta and base calls. All of it fails on a build without the filter: the argument and the calls do not exist
there, and a marker word k | 0x400 opens as corrupt."""
import numpy as np
import pytest

from tests import delta_model as dm
from tests import planes_model as pm
from tests import reflib
from tests import seekable_cases as sc
from tests import xor_model as xm

pytestmark = pytest.mark.gpu

GUARD = 64
ELEMENTS = {1025: 3 * 1025 + 37, 4096: 3 * 4096 + 37}
LITERALS = 1                        # DeviceBatchContext.classify: 0 = the search, 1 = literals only


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


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _host(t):
    return t.cpu().numpy()


def _pair(k, elements, seed=20):
    """(source bytes, base bytes): what two versions of a tensor look like -- byte 0 of every element differs in its low 3 bits, byte 1 of one element in 61 by
    one bit, nothing above: the XOR's plane 0 is noise, plane 1 sparse, the others zeros"""
    src = xm.source(k, elements, seed=seed + k)
    base = xm.base_of("low_bits", src, k, seed=seed)
    base[1::61 * k] ^= 0x10
    return src, base


def _ranges(k, frame, elements):
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


# ------------------------------------------------------------------------------------------------ the kernels on their own
@pytest.mark.parametrize("k", [2, 4, 8])
def test_planes_split_and_join(zstd, ctx, k):
    """every group size at which the bodies take another path with last groups of 1, 15 and 17 elements, the three kinds of base, tensor views at byte offsets
    0 and 1, guard bytes around the outputs; source and base unchanged"""
    import torch
    n_case = 0
    for m in xm.GROUP_SIZES:
        for last in xm.LAST_GROUPS:
            if last > m:
                continue
            elements = 2 * m + last
            kind = xm.BASES[n_case % len(xm.BASES)]; off = n_case % 2; n_case += 1
            src = xm.source(k, elements, seed=1000 * k + m)
            base = xm.base_of(kind, src, k, seed=m)
            want = xm.split(src, base, k, m)
            _, s = _guarded_dev(src.size, off, 0x5A); s.copy_(torch.from_numpy(src))
            _, b = _guarded_dev(src.size, 1 - off, 0x5A); b.copy_(torch.from_numpy(base))
            out_hold, out = _guarded_dev(src.size, 1 - off, 0xC7)
            got = ctx.planes_split(s, m, k, out=out, base=b)
            assert (_host(got) == want).all(), (k, m, last, kind)
            assert _guards_intact(out_hold, src.size, 1 - off, 0xC7) and (kind != "same" or not _host(got).any())
            back_hold, back_out = _guarded_dev(src.size, off, 0xC7)
            back = ctx.planes_join(got, m, k, out=back_out, base=b, filter="xor_base")
            assert (_host(back) == src).all(), (k, m, last, kind)
            assert _guards_intact(back_hold, src.size, off, 0xC7) and (_host(s) == src).all() and (_host(b) == base).all()


def test_planes_more_tiles_than_waves(zstd, ctx):
    """twice the launch's waves plus one tile in ONE group and a short group behind it: the grid-stride loops' later trips; the module functions, element size
    from the dtype, the base a tensor of the dtype"""
    import torch
    waves = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    m = (2 * waves + 1) * 1024 + 5
    src, base = _pair(4, m + 7, seed=3)
    t = torch.from_numpy(src.view(np.int32)).cuda(); b = torch.from_numpy(base.view(np.int32)).cuda()
    planar = zstd.device.planes_split(t, m, ctx=ctx, base=b)
    assert (_host(planar) == xm.split(src, base, 4, m)).all()
    assert (_host(zstd.device.planes_join(planar, m, 4, ctx=ctx, base=b)) == src).all()
    assert (_host(ctx.planes_split(t, m)) == pm.split(src, 4, m)).all()


# ------------------------------------------------------------------------------------------------ compress and the reads
@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("frame,checksum", [(1025, False), (4096, True)])
def test_compress_and_read(zstd, ctx, k, frame, checksum):
    """every plane frame is libzstd's frame of the model's plane; the marker and the table are the model's; read and read_ranges with the base return the
    source's bytes, also under a small scratch limit; libzstd decodes the whole stream to the filtered planar bytes, which planes_to_elements(base=) turns
    into the source; without the base the reads raise, raw=True needs none"""
    elements = ELEMENTS[frame]
    src, base = _pair(k, elements)
    b = _dev(base)
    out = ctx.seekable_compress(_dev(src), frame_size=frame, element_size=k, checksum=checksum, base=b)
    raw = _host(out).tobytes()
    ref = reflib.checker()
    planes = xm.planes(src, base, k, frame)
    frames = [ref.compress(p, level=3) for p in planes]
    entries, ck, table_at = sc.parse(raw)
    assert ck == checksum and len(entries) == len(planes) + 1 and entries[-1][:2] == (24, 0)
    at = 0
    for i, (c, d, x) in enumerate(entries[:-1]):
        assert raw[at:at + c] == frames[i], "plane frame %d is not libzstd's" % i
        assert d == len(planes[i]) and (not checksum or x == sc.xxh64(planes[i]) & 0xFFFFFFFF)
        at += c
    assert raw[at:at + 24] == xm.marker(k, frame) and at + 24 == table_at
    assert raw == xm.stream_of(frames, planes, k, frame, checksum)
    assert raw == _host(ctx.seekable_compress(_dev(src), frame_size=frame, element_size=k, checksum=checksum, filter="xor_base", base=b)).tobytes()
    rg = _ranges(k, frame, elements)
    for limit in (None, 5000):
        with zstd.device.SeekableStream(ctx, out, scratch_limit=limit, base=b) as st:
            assert st.element_size == k and st.group_elements == frame and st.filter == "xor_base" and st.content_size == src.size and st.has_checksums == checksum
            assert (_host(st.read()) == src).all()
            views = st.read_ranges(rg)
            assert (st.last_gather_stats["passes"] == 1) == (limit is None)
            for (o, n), v in zip(rg, views):
                assert _host(v).tobytes() == src[o:o + n].tobytes(), (o, n, limit)
            assert _host(st.read(7, 1001)).tobytes() == src[7:1008].tobytes()
    assert (_host(b) == base).all()
    with zstd.device.SeekableStream(ctx, out) as st:                           # no base: the filter is known, the elements are not to be had
        assert st.filter == "xor_base" and st.element_size == k
        for call in (lambda: st.read(), lambda: st.read(0, 10), lambda: st.read_ranges([(0, 4)])):
            with pytest.raises(zstd.ZstdError, match="base"):
                call()
        with pytest.raises(ValueError):
            st.edit(np.array([[0, 0]]))
    with zstd.device.SeekableStream(ctx, out, raw=True) as st:
        assert st.element_size == 1 and st.filter is None
        planar = _host(st.read()).tobytes()
    whole = b"".join(ref.decompress(raw[a:a + c], d) for (c, d, _), a in zip(entries[:-1], np.cumsum([0] + [e[0] for e in entries[:-2]]).tolist()))
    assert whole == planar == xm.split(src, base, k, frame).tobytes()
    assert zstd.seekable.planes_to_elements(whole, k, frame, base=base.tobytes()) == src.tobytes()
    assert zstd.seekable.elements_to_planes(src.tobytes(), k, frame, base=base.tobytes()) == planar


@pytest.mark.parametrize("finder", ["none", "auto"])
def test_other_match_finders(zstd, ctx, finder):
    """the same under the literals-only and the auto finder (the host-bytes module builds the contexts): every frame is that finder's frame of the model's
    plane -- libzstd's literals-only frame, or under "auto" the one of the two that DeviceBatchContext.classify names for the plane, and in one stream the
    noisy planes take the one and the zero planes the other --, the marker and the table are the model's, the readers with the base return the elements"""
    import torch
    k, frame = 4, 4096
    src, base = _pair(k, ELEMENTS[frame])
    data, bdata = src.tobytes(), base.tobytes()
    planes = xm.planes(src, base, k, frame)
    ref = reflib.checker()
    flags = reflib.F_CONTENTSIZE | reflib.F_DICTID
    if finder == "auto":
        joined = _dev(np.frombuffer(b"".join(planes), dtype=np.uint8))
        offs = np.cumsum([0] + [len(p) for p in planes])
        segs = torch.from_numpy(np.array([(int(o), len(p)) for o, p in zip(offs, planes)], dtype=np.int64)).cuda()
        choice = _host(ctx.classify(joined, segs)).tolist()
        assert 0 < sum(choice) < len(choice), "the data must make both choices occur"
        full = len(planes) - k                                                 # (the last group's planes, 37 bytes each, are below what classify samples)
        assert all(choice[i] == LITERALS for i in range(0, full, k)) and all(choice[i] != LITERALS for i in range(k - 1, full, k))      # noise: literals; zeros: the search
    else:
        choice = [LITERALS] * len(planes)
    frames = [ref.compress_sequences(p, [], len(p), level=3, flags=flags) if c == LITERALS else ref.compress(p, level=3, flags=flags) for p, c in zip(planes, choice)]
    stream = zstd.seekable.compress(data, frame_size=frame, element_size=k, base=bdata, match_finder=finder)
    entries, _, _ = sc.parse(stream)
    at = 0
    for i, ((c, d, _), p) in enumerate(zip(entries[:-1], planes)):
        assert stream[at:at + c] == frames[i], "plane frame %d is not the frame of finder choice %d" % (i, choice[i])
        assert ref.decompress(stream[at:at + c], d) == p
        at += c
    assert stream == xm.stream_of(frames, planes, k, frame, False)
    assert zstd.seekable.decompress(stream, base=bdata) == data
    assert zstd.seekable.decompress(stream, 5, 100, base=bdata) == data[5:105]
    assert zstd.seekable.decompress_ranges(stream, [(3, 9), (frame * k - 1, 2)], base=bdata) == [data[3:12], data[frame * k - 1:frame * k + 1]]
    with pytest.raises(zstd.ZstdError, match="base"):
        zstd.seekable.decompress(stream)


def test_checksums_and_damage(zstd, ctx):
    """with checksum=True: one flipped content byte (a raw literal of plane frame 8: group 2, plane 0 of a k = 4 stream whose byte 0 is XORed with noise) fails
    with 22 exactly the ranges that need group 2, and no others"""
    import torch
    k, frame = 4, 1025
    elements = ELEMENTS[frame]
    src = xm.source(k, elements, seed=8)
    base = src.copy(); base[::k] = np.random.default_rng(9).integers(0, 256, elements, dtype=np.uint8)      # (plane 0 of the XOR is incompressible: raw blocks, so a flipped byte is a content byte)
    b = _dev(base)
    out = ctx.seekable_compress(_dev(src), frame_size=frame, element_size=k, checksum=True, base=b)
    raw = _host(out).tobytes()
    entries, ck, _ = sc.parse(raw)
    planes = xm.planes(src, base, k, frame)
    assert ck and [e[2] for e in entries[:-1]] == [sc.xxh64(p) & 0xFFFFFFFF for p in planes] and entries[-1][2] == pm.XXH_EMPTY
    bad = bytearray(raw)
    bad[sum(e[0] for e in entries[:8]) + entries[8][0] // 2] ^= 0x55
    bad_t = torch.frombuffer(bad, dtype=torch.uint8).cuda()
    g = frame * k
    rg = [(10, 100), (2 * g - 3, 5), (2 * g, g), (3 * g, 37 * k), (0, src.size), (3 * g - 1, 1), (3 * g, 1), (g + 1, g - 1), (2 * g + 8, 0)]
    touches = [o < 3 * g and o + ln > 2 * g and ln > 0 for o, ln in rg]
    assert touches == [False, True, True, False, True, True, False, False, False]
    with zstd.device.SeekableStream(ctx, bad_t, base=b) as st:
        table = np.zeros((len(rg), 3), dtype=np.uint64)
        at = 0
        for i, (o, ln) in enumerate(rg):
            table[i] = (o, ln, at); at += ln
        dst = torch.zeros(at, dtype=torch.uint8, device="cuda")
        status = torch.zeros(2 + 2 * len(rg), dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream()
        rc = ctx.L.zhip_seekable_decompress_typed_ranges_base_device(ctx.ctx, st.handle, b.data_ptr(), b.numel(), table.ctypes.data, len(rg), dst.data_ptr(), at, status.data_ptr(), None,
                                                                     s.cuda_stream)
        assert rc == 0
        s.synchronize()
        status = status.cpu().tolist()
        got = _host(dst)
        assert status[:2] == [22, 1]
        for r, ((o, ln), touch) in enumerate(zip(rg, touches)):
            assert status[2 + 2 * r:4 + 2 * r] == ([22, 8] if touch else [0, 0]), r
            if not touch:
                assert got[int(table[r, 2]):int(table[r, 2]) + ln].tobytes() == src[o:o + ln].tobytes(), r
        with pytest.raises(zstd.ZstdError):
            st.read(2 * g, 10)


# ------------------------------------------------------------------------------------------------ the refusals
def test_refusals(zstd, ctx):
    """through Python, and through the C calls: UNSUPPORTED (6), nothing queued; destination, size and status words untouched"""
    import torch
    t = torch.zeros(24, dtype=torch.uint8, device="cuda"); b = torch.ones(24, dtype=torch.uint8, device="cuda")
    for call in (lambda: ctx.seekable_compress(t, element_size=2, filter="xor_base"), lambda: ctx.seekable_compress(t, element_size=2, filter="delta", base=b),
                 lambda: ctx.seekable_compress(t, element_size=2, filter="xor", base=b), lambda: ctx.seekable_compress(t, element_size=2, filter="xor"),
                 lambda: ctx.seekable_compress(t, base=b), lambda: ctx.seekable_compress(t, element_size=1, base=b), lambda: ctx.seekable_compress(t, element_size=2, base=b[:22]),
                 lambda: ctx.seekable_compress(t, element_size=2, base=b.cpu()), lambda: ctx.seekable_compress(t, element_size=3, base=b),
                 lambda: ctx.planes_split(t, 4, 2, filter="xor_base"), lambda: ctx.planes_join(t, 4, 2, filter="xor_base"), lambda: ctx.planes_split(t, 4, 2, filter="delta", base=b),
                 lambda: ctx.planes_join(t, 4, 2, base=b[:20]), lambda: ctx.planes_split(t, 4, 1, base=b), lambda: ctx.planes_split(t, 4, 2, out=b, base=b),
                 lambda: ctx.planes_join(t, 4, 2, out=b, base=b)):
        with pytest.raises(zstd.ZstdError):
            call()
    assert (_host(b) == 1).all()
    plain = ctx.seekable_compress(t, frame_size=4, element_size=2)
    with pytest.raises(zstd.ZstdError, match="base"):
        zstd.device.SeekableStream(ctx, plain, base=b)                          # base= on a stream that was not written against one
    with zstd.device.SeekableStream(ctx, plain, raw=True, base=b) as st:        # (raw: a plain stream, the base is not looked at)
        assert st.filter is None
    # the C calls themselves
    dst = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    size = torch.full((1,), -1, dtype=torch.int64, device="cuda"); status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    L = ctx.L
    for k, base_ptr, word in ((2, None, b"NULL"), (1, b.data_ptr(), b"element size"), (2, dst.data_ptr() + 4095, b"overlaps"), (2, dst.data_ptr(), b"overlaps")):
        assert L.zhip_seekable_compress_typed_base_device(ctx.ctx, t.data_ptr(), 24, 4, k, base_ptr, 0, dst.data_ptr(), 4096, size.data_ptr(), status.data_ptr(), s) == 6
        assert word in L.zhip_last_error() and b"base" in L.zhip_last_error()
        for call in (L.zhip_planes_split_base_device, L.zhip_planes_join_base_device):
            assert call(ctx.ctx, t.data_ptr(), 24, k, 4, base_ptr if base_ptr != dst.data_ptr() + 4095 else dst.data_ptr() + 23, dst.data_ptr(), s) == 6
            assert word in L.zhip_last_error()
    for k in (1, 2):                                                            # the *_filter_ calls have no base to take: filter 4 as filter 2
        assert L.zhip_seekable_compress_typed_filter_device(ctx.ctx, t.data_ptr(), 24, 4, k, 4, 0, dst.data_ptr(), 4096, size.data_ptr(), status.data_ptr(), s) == 6
        assert b"filter" in L.zhip_last_error()
    for call in (L.zhip_planes_split_filter_device, L.zhip_planes_join_filter_device):
        assert call(ctx.ctx, t.data_ptr(), 24, 2, 4, 4, dst.data_ptr(), s) == 6 and b"filter" in L.zhip_last_error()
    # the reads: a filter-4 handle without a base, with a NULL base, a base of another size, a base over the output; a handle whose filter is not 4 with one
    src, base = _pair(2, 12)
    sb = _dev(base)
    xs = ctx.seekable_compress(_dev(src), frame_size=4, element_size=2, base=sb)
    ds = ctx.seekable_compress(_dev(src), frame_size=4, element_size=2, filter="delta")
    table = np.array([[2, 20, 0]], dtype=np.uint64)
    rstatus = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    with zstd.device.SeekableStream(ctx, xs, base=sb) as st, zstd.device.SeekableStream(ctx, ds) as st_delta, zstd.device.SeekableStream(ctx, plain) as st_plain:
        assert L.zhip_seekable_filter(st.handle) == 4 and L.zhip_seekable_filter(st_delta.handle) == 1 and L.zhip_seekable_filter(st_plain.handle) == 0
        assert L.zhip_seekable_decompress_typed_ranges_device(ctx.ctx, st.handle, table.ctypes.data, 1, dst.data_ptr(), 4096, rstatus.data_ptr(), None, s) == 6
        assert b"base" in L.zhip_last_error()
        for base_ptr, base_size, word in ((None, 24, b"NULL"), (sb.data_ptr(), 22, b"size"), (sb.data_ptr(), 26, b"size"), (dst.data_ptr() + 4090, 24, b"overlaps")):
            assert L.zhip_seekable_decompress_typed_ranges_base_device(ctx.ctx, st.handle, base_ptr, base_size, table.ctypes.data, 1, dst.data_ptr(), 4096, rstatus.data_ptr(), None, s) == 6
            assert word in L.zhip_last_error() and b"base" in L.zhip_last_error()
        for other in (st_delta, st_plain):
            assert L.zhip_seekable_decompress_typed_ranges_base_device(ctx.ctx, other.handle, sb.data_ptr(), 24, table.ctypes.data, 1, dst.data_ptr(), 4096, rstatus.data_ptr(), None, s) == 6
            assert b"filter" in L.zhip_last_error()
    torch.cuda.synchronize()
    assert (_host(dst) == 0x5A).all() and int(size[0]) == -1 and status.tolist() == [-1, -1] and rstatus.tolist() == [-1] * 4


# ------------------------------------------------------------------------------------------------ one context, every filter
def test_one_context_alternating_filters(zstd, ctx):
    """plain, delta and base calls alternate on ONE context over the same buffers, twice: every stream is what that call writes on its own, every read returns
    the source -- nothing of one call (the staging buffer, the tile sums, a handle's tables) leaks into the next"""
    import torch
    k, frame = 4, 1025
    elements = ELEMENTS[frame]
    src, base = _pair(k, elements, seed=31)
    t, b = _dev(src), _dev(base)
    ref = reflib.checker()
    want = {}
    for name, planes, stream_of in (("plain", pm.planes(src, k, frame), lambda f, p: pm.stream_of(f, p, k, frame, False)),
                                    ("delta", dm.planes(src, k, frame), lambda f, p: dm.stream_of(f, p, k, frame, False)),
                                    ("base", xm.planes(src, base, k, frame), lambda f, p: xm.stream_of(f, p, k, frame, False))):
        want[name] = stream_of([ref.compress(p, level=3) for p in planes], planes)
    kw = {"plain": {}, "delta": {"filter": "delta"}, "base": {"base": b}}
    planar_want = {"plain": pm.split(src, k, frame), "delta": dm.split(src, k, frame), "base": xm.split(src, base, k, frame)}
    rg = _ranges(k, frame, elements)
    out = torch.empty(src.size, dtype=torch.uint8, device="cuda"); back = torch.empty(src.size, dtype=torch.uint8, device="cuda")
    for name in ("base", "plain", "delta", "base", "delta", "plain", "base"):
        stream = ctx.seekable_compress(t, frame_size=frame, element_size=k, **kw[name])
        assert _host(stream).tobytes() == want[name], name
        with zstd.device.SeekableStream(ctx, stream, scratch_limit=5000, base=b if name == "base" else None) as st:
            assert st.filter == {"plain": None, "delta": "delta", "base": "xor_base"}[name]
            for (o, n), v in zip(rg, st.read_ranges(rg)):
                assert _host(v).tobytes() == src[o:o + n].tobytes(), (name, o, n)
        planar = ctx.planes_split(t, frame, k, out=out, **kw[name])
        assert (_host(planar) == planar_want[name]).all(), name
        assert (_host(ctx.planes_join(planar, frame, k, out=back, **kw[name])) == src).all(), name
    assert (_host(t) == src).all() and (_host(b) == base).all()
