"""Typed seekable streams on the GPU (include/zstd_hip.h, "typed streams"): the two transposition kernels against the numpy model of tests/planes_model.py,
typed compress through DeviceBatchContext with every plane frame compared with libzstd 1.5.7's frame of that plane (tests/reflib.checker()), the marker, the
typed reads against slices of the source, one damaged plane frame, and the plain behaviour that must not move. All of it fails on a build without the feature:
the arguments, the calls and the attributes do not exist there."""
import ctypes as C

import numpy as np
import pytest

from tests import planes_model as pm
from tests import reflib
from tests import seekable_cases as sc

pytestmark = pytest.mark.gpu

FRAME = 4096
ELEMENTS = 3 * FRAME + 37
GUARD = 64


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


def _sources():
    rng = np.random.default_rng(20)
    return {"fp32": rng.normal(0, 0.02, ELEMENTS).astype(np.float32).view(np.uint8), "int32": rng.integers(0, 50000, ELEMENTS, dtype=np.int32).view(np.uint8)}


# ------------------------------------------------------------------------------------------------ the kernels on their own
@pytest.mark.parametrize("k", [2, 4, 8])
def test_planes_split_and_join(zstd, ctx, k):
    """every group size at which the bodies take another path, a shorter last group, tensor views at byte offsets 0 and 1, guard bytes on both sides"""
    import torch
    for m in pm.GROUP_SIZES:
        elements = 2 * m + max(1, m // 3)
        src = np.random.default_rng(1000 * k + m).integers(0, 256, elements * k, dtype=np.uint8)
        want = pm.split(src, k, m)
        for off in (0, 1):
            hold = torch.full((src.size + 2 * GUARD + 1,), 0x5A, dtype=torch.uint8, device="cuda")
            s = hold[GUARD + off:GUARD + off + src.size]; s.copy_(torch.from_numpy(src))
            out_hold = torch.full((src.size + 2 * GUARD + 1,), 0xC7, dtype=torch.uint8, device="cuda")
            out = out_hold[GUARD + 1 - off:GUARD + 1 - off + src.size]
            got = ctx.planes_split(s, m, k, out=out)
            assert (_host(got) == want).all(), (k, m, off)
            h = _host(out_hold)
            assert (h[:GUARD + 1 - off] == 0xC7).all() and (h[GUARD + 1 - off + src.size:] == 0xC7).all()
            back_hold = torch.full((src.size + 2 * GUARD + 1,), 0xC7, dtype=torch.uint8, device="cuda")
            back = ctx.planes_join(got, m, k, out=back_hold[GUARD + off:GUARD + off + src.size])
            assert (_host(back) == src).all(), (k, m, off)
            h = _host(back_hold)
            assert (h[:GUARD + off] == 0xC7).all() and (h[GUARD + off + src.size:] == 0xC7).all()


def test_planes_more_tiles_than_waves(zstd, ctx):
    """twice the launch's waves plus one tile of 1 024 elements (the grid is eight waves a CU): the grid-stride loop's second and third trip, k = 2"""
    import torch
    waves = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    elements = (2 * waves + 1) * 1024
    src = np.random.default_rng(3).integers(0, 1 << 16, elements, dtype=np.uint16)
    t = torch.from_numpy(src.view(np.int16)).cuda()
    planar = zstd.device.planes_split(t, 131072, ctx=ctx)             # element_size from the dtype
    assert (_host(planar) == pm.split(src, 2, 131072)).all()
    assert (_host(ctx.planes_join(planar, 131072, 2)).view(np.uint16) == src).all()


def test_planes_refusals(zstd, ctx):
    import torch
    t = torch.zeros(24, dtype=torch.uint8, device="cuda")
    for frame, k in ((4, 3), (0, 2), ((1 << 30) + 1, 2)):
        with pytest.raises(zstd.ZstdError):
            ctx.planes_split(t, frame, k)
    with pytest.raises(zstd.ZstdError):
        ctx.planes_join(t[:23], 4, 2)


# ------------------------------------------------------------------------------------------------ typed compress and the typed reads
ODD_RANGES = [(1, 2), (3, 6), (100, 999), (FRAME * 4 - 5, 11), (FRAME * 4 - 3, 2 * FRAME * 4 + 9), (50, 0), (100, 999), (500, 2000), (0, ELEMENTS * 4), (ELEMENTS * 4 - 3, 3),
              (FRAME * 4, FRAME * 4), (2 * FRAME * 4 + 2, FRAME * 4 + 37 * 4 - 2)]


def _check_typed_stream(zstd, ctx, src, stream_t, stream=None):
    ref = reflib.checker()
    raw = _host(stream_t).tobytes()
    planes = pm.planes(src, 4, FRAME)
    frames = [ref.compress(p, level=3) for p in planes]
    entries, ck, table_at = sc.parse(raw)
    assert not ck and len(entries) == len(planes) + 1 and entries[-1][:2] == (24, 0)
    at = 0
    for i, (c, d, _) in enumerate(entries[:-1]):
        assert raw[at:at + c] == frames[i], "plane frame %d is not libzstd's" % i
        assert d == len(planes[i])
        at += c
    assert raw[at:at + 24] == pm.marker(4, FRAME) and at + 24 == table_at
    assert raw == pm.stream_of(frames, planes, 4, FRAME, False)
    # the stream's size against the plain cut's at the same frame bytes: libzstd's totals, computed here
    plain_total = sum(len(ref.compress(c, level=3)) for c in sc.chunks(src.tobytes(), FRAME))
    plane_total = sum(len(f) for f in frames)
    print("plane frames %d bytes, plain frames %d bytes" % (plane_total, plain_total))
    assert at == plane_total and plane_total < plain_total
    with zstd.device.SeekableStream(ctx, stream_t, stream=stream) as st:
        assert st.element_size == 4 and st.group_elements == FRAME and st.content_size == src.size and st.n_frames == len(planes) + 1
        assert (_host(st.read(stream=stream)) == src).all()
        views = st.read_ranges(ODD_RANGES, stream=stream)
        assert st.last_gather_stats["passes"] == 1
        for (o, n), v in zip(ODD_RANGES, views):
            assert _host(v).tobytes() == src[o:o + n].tobytes(), (o, n)
        assert _host(st.read(7, 1001, stream=stream)).tobytes() == src[7:1008].tobytes()
        # read_records / frame_offsets stay raw: the plane frames
        assert st.frame_offsets().tolist() == np.cumsum([0] + [len(p) for p in planes] + [0]).tolist()
        assert _host(st.read_records([5], stream=stream)[0]).tobytes() == planes[5]
    with zstd.device.SeekableStream(ctx, stream_t, stream=stream, raw=True) as st:
        assert st.element_size == 1 and st.group_elements == 0
        planar = _host(st.read(stream=stream)).tobytes()
        assert planar == pm.split(src, 4, FRAME).tobytes()
        assert zstd.seekable.planes_to_elements(planar, 4, FRAME) == src.tobytes()
        assert zstd.seekable.elements_to_planes(src.tobytes(), 4, FRAME) == planar


@pytest.mark.parametrize("name", ["fp32", "int32"])
def test_typed_compress_and_read(zstd, ctx, name):
    src = _sources()[name]
    _check_typed_stream(zstd, ctx, src, ctx.seekable_compress(_dev(src), frame_size=FRAME, element_size=4))


def test_typed_on_a_callers_stream(zstd, ctx):
    import torch
    src = _sources()["fp32"]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = _dev(src)
    out = ctx.seekable_compress(t, frame_size=FRAME, element_size=4, stream=side)
    _check_typed_stream(zstd, ctx, src, out, stream=side)
    side.synchronize()


def test_scratch_limit_passes(zstd, ctx):
    """a planar buffer limited to 20 000 bytes: the whole content is cut at group boundaries into passes"""
    src = _sources()["int32"]
    out = ctx.seekable_compress(_dev(src), frame_size=FRAME, element_size=4)
    with zstd.device.SeekableStream(ctx, out, scratch_limit=20000) as st:
        views = st.read_ranges([(5, src.size - 7), (7, 9)])
        assert st.last_gather_stats["passes"] == 3
        assert _host(views[0]).tobytes() == src[5:src.size - 2].tobytes() and _host(views[1]).tobytes() == src[7:16].tobytes()


def test_bf16_groups_with_checksums_and_damage(zstd, ctx):
    """bf16 N(0, 0.02), 131 072-element groups, 5 groups + 1 000 elements, table checksums: the round trip; then one flipped byte inside plane frame 4 (group 2,
    plane 0) fails exactly the ranges that need group 2 -- 22, or the decoder's code -- and no other"""
    import torch
    G, n = 131072, 5 * 131072 + 1000
    t = (torch.randn(n, generator=torch.Generator().manual_seed(4)) * 0.02).to(torch.bfloat16).cuda()
    src = _host(t.view(torch.uint8)).reshape(-1)
    out = ctx.seekable_compress(t.view(torch.uint8).reshape(-1), frame_size=G, checksum=True, element_size=2)
    raw = _host(out).tobytes()
    entries, ck, _ = sc.parse(raw)
    assert ck and len(entries) == 13 and [e[1] for e in entries] == [G] * 10 + [1000, 1000, 0]
    planes = pm.planes(src, 2, G)
    assert [e[2] for e in entries[:-1]] == [sc.xxh64(p) & 0xFFFFFFFF for p in planes] and entries[-1][2] == pm.XXH_EMPTY
    with zstd.device.SeekableStream(ctx, out) as st:
        assert st.element_size == 2 and st.group_elements == G and st.has_checksums
        assert (_host(st.read()) == src).all()
    bad = bytearray(raw)
    bad[sum(e[0] for e in entries[:4]) + entries[4][0] // 2] ^= 0x55
    bad_t = torch.frombuffer(bad, dtype=torch.uint8).cuda()
    g = 2 * G                                           # bytes of one group
    rg = [(10, 100), (2 * g - 3, 5), (2 * g, g), (3 * g, g), (0, src.size), (3 * g - 1, 1), (3 * g, 1), (5 * g, 2000), (g + 1, g - 1)]
    touches = [o < 3 * g and o + ln > 2 * g for o, ln in rg]
    assert touches == [False, True, True, False, True, True, False, False, False]
    with zstd.device.SeekableStream(ctx, bad_t) as st:
        table = np.zeros((len(rg), 3), dtype=np.uint64)
        at = 0
        for i, (o, ln) in enumerate(rg):
            table[i] = (o, ln, at); at += ln
        dst = torch.zeros(at, dtype=torch.uint8, device="cuda")
        status = torch.zeros(2 + 2 * len(rg), dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream()
        rc = ctx.L.zhip_seekable_decompress_typed_ranges_device(ctx.ctx, st.handle, table.ctypes.data, len(rg), dst.data_ptr(), at, status.data_ptr(), None, s.cuda_stream)
        assert rc == 0
        s.synchronize()
        status = status.cpu().tolist()
        got = _host(dst)
        assert status[0] != 0 and status[1] == 1
        for r, ((o, ln), touch) in enumerate(zip(rg, touches)):
            code, frame = status[2 + 2 * r], status[3 + 2 * r]
            if touch:
                assert code != 0 and frame == 4, (r, code, frame)
            else:
                assert (code, frame) == (0, 0), r
                assert got[int(table[r, 2]):int(table[r, 2]) + ln].tobytes() == src[o:o + ln].tobytes(), r
        with pytest.raises(zstd.ZstdError):
            st.read(2 * g, 10)


# ------------------------------------------------------------------------------------------------ plain behaviour held
def test_plain_behaviour_held(zstd, ctx):
    import torch
    src = _sources()["fp32"]
    t = _dev(src)
    plain = ctx.seekable_compress(t, frame_size=FRAME)
    assert torch.equal(plain, ctx.seekable_compress(t, frame_size=FRAME, element_size=1))
    assert len(sc.parse(_host(plain).tobytes())[0]) == len(sc.chunks(src.tobytes(), FRAME))      # no marker
    typed = ctx.seekable_compress(t, frame_size=FRAME, element_size=4)
    with zstd.device.SeekableStream(ctx, plain) as st:
        assert st.element_size == 1 and st.group_elements == 0
        assert (_host(st.read()) == src).all()
        table = np.array([[0, 16, 0]], dtype=np.uint64)
        dst = torch.zeros(16, dtype=torch.uint8, device="cuda"); status = torch.zeros(4, dtype=torch.int32, device="cuda")
        rc = ctx.L.zhip_seekable_decompress_typed_ranges_device(ctx.ctx, st.handle, table.ctypes.data, 1, dst.data_ptr(), 16, status.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        assert rc == 6 and b"plain" in ctx.L.zhip_last_error()
    rec = [(0, 100)]
    with zstd.device.SeekableStream(ctx, typed) as st:
        for call in (lambda: st.edit([(0, 0)]), lambda: st.append_records(t, rec), lambda: st.replace_records([0], t, rec), lambda: st.delete_records([0]), lambda: st.reorder([1, 0])):
            with pytest.raises(ValueError):
                call()
    with zstd.device.SeekableStream(ctx, typed, raw=True) as st:          # the planar form may be edited: it is an ordinary stream
        kept = st.reorder(list(range(st.n_frames)))
        assert torch.equal(kept, typed)
    for kw in ({"element_size": 3}, {"element_size": 4, "frame_size": 0}):
        with pytest.raises(zstd.ZstdError):
            ctx.seekable_compress(t, **kw)
    with pytest.raises(zstd.ZstdError):
        ctx.seekable_compress(t[:-1], element_size=4)


def test_host_bytes_module(zstd):
    """zstandard_amd.seekable: compress(element_size=) and the readers that detect the typed stream; a wave-finder context is accepted"""
    src = _sources()["int32"]
    data = src.tobytes()
    stream = zstd.seekable.compress(data, frame_size=FRAME, element_size=4)
    assert zstd.seekable.decompress(stream) == data
    assert zstd.seekable.decompress(stream, 5, 100) == data[5:105]
    assert zstd.seekable.decompress_ranges(stream, [(3, 9), (FRAME * 4 - 1, 2)]) == [data[3:12], data[FRAME * 4 - 1:FRAME * 4 + 1]]
    wave = zstd.seekable.compress(data, frame_size=FRAME, element_size=4, match_finder="wave")
    assert sc.parse(wave)[0][-1][:2] == (24, 0) and zstd.seekable.decompress(wave) == data
