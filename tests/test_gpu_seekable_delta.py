"""The delta filter of typed seekable streams on the GPU (include/zstd_hip.h, "filters"): the split-with-delta kernel and the three launches
of the delta join against the numpy model of tests/delta_model.py, seekable_compress(filter="delta") with every plane frame compared with libzstd 1.5.7's
frame of the model's plane (tests/reflib.checker()), the marker, the reads against slices of the source, the literals-only and wave finders, one damaged
plane frame, and the unfiltered stream that must not move. All of it fails on a build without the filter: the argument and the calls do not exist there."""
import numpy as np
import pytest

from tests import delta_model as dm
from tests import planes_model as pm
from tests import reflib
from tests import seekable_cases as sc

pytestmark = pytest.mark.gpu

GUARD = 64
ELEMENTS = {1025: 3 * 1025 + 37, 4096: 3 * 4096 + 37}


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


def _source(k, elements, seed=20):
    """integer tensors the filter is for: sorted ids (k = 4), running sums (k = 8), a noisy ramp (k = 2) -- as bytes"""
    rng = np.random.default_rng(seed + k)
    x = np.sort(rng.integers(0, 1 << 31, elements)) if k == 4 else np.cumsum(rng.integers(0, 1000, elements)) if k == 8 else np.arange(elements) * 3 + rng.integers(0, 40, elements)
    return x.astype(dm.DTYPES[k]).view(np.uint8).copy()


def _ranges(k, frame, elements):
    g, size = frame * k, elements * k
    rg = [(1, 2), (3, k + 2), (100, 999), (g - 5, 11), (g - 3, 2 * g + 9), (50, 0), (100, 999), (500, 2000), (0, size), (size - 3, 3), (g, g), (0, 1), (size, 0), (2 * g + 2, g + 37 * k - 2)]
    return [(o, min(n, size - o)) for o, n in rg]


# ------------------------------------------------------------------------------------------------ the kernels on their own
@pytest.mark.parametrize("k", [2, 4, 8])
def test_planes_split_and_join(zstd, ctx, k):
    """every group size at which the bodies take another path with last groups of 1, 15 and 17 elements, every value kind, tensor views at byte offsets 0 and 1,
    guard bytes on both sides"""
    import torch
    n_case = 0
    for m in dm.GROUP_SIZES:
        for last in dm.LAST_GROUPS:
            if last > m:
                continue
            elements = 2 * m + last
            kind = dm.KINDS[n_case % len(dm.KINDS)]; off = n_case % 2; n_case += 1
            for kind in (kind, "carry"):
                src = dm.values(kind, k, elements, m, seed=1000 * k + m)
                want = dm.split(src, k, m)
                hold = torch.full((src.size + 2 * GUARD + 1,), 0x5A, dtype=torch.uint8, device="cuda")
                s = hold[GUARD + off:GUARD + off + src.size]; s.copy_(torch.from_numpy(src))
                out_hold = torch.full((src.size + 2 * GUARD + 1,), 0xC7, dtype=torch.uint8, device="cuda")
                out = out_hold[GUARD + 1 - off:GUARD + 1 - off + src.size]
                got = ctx.planes_split(s, m, k, out=out, filter="delta")
                assert (_host(got) == want).all(), (k, m, last, kind)
                h = _host(out_hold)
                assert (h[:GUARD + 1 - off] == 0xC7).all() and (h[GUARD + 1 - off + src.size:] == 0xC7).all()
                back_hold = torch.full((src.size + 2 * GUARD + 1,), 0xC7, dtype=torch.uint8, device="cuda")
                back = ctx.planes_join(got, m, k, out=back_hold[GUARD + off:GUARD + off + src.size], filter="delta")
                assert (_host(back) == src).all(), (k, m, last, kind)
                h = _host(back_hold)
                assert (h[:GUARD + off] == 0xC7).all() and (h[GUARD + off + src.size:] == 0xC7).all()


@pytest.mark.parametrize("k", [2, 4, 8])
def test_planes_three_groups_of_4103(zstd, ctx, k):
    """3 groups of 4 103 elements (five tiles and a tail of 7 each), random and carrying values; the module functions, element size from the dtype"""
    import torch
    m = 4103
    for kind in ("random", "carry"):
        src = dm.values(kind, k, 3 * m, m, seed=k)
        t = torch.from_numpy(src.view({2: np.int16, 4: np.int32, 8: np.int64}[k])).cuda()
        planar = zstd.device.planes_split(t, m, ctx=ctx, filter="delta")
        assert (_host(planar) == dm.split(src, k, m)).all(), (k, kind)
        assert (_host(zstd.device.planes_join(planar, m, k, ctx=ctx, filter="delta")) == src).all(), (k, kind)
        assert (_host(ctx.planes_split(t, m, filter=None)) == pm.split(src, k, m)).all()


def test_planes_more_tiles_than_waves_and_long_groups(zstd, ctx):
    """twice the launch's waves plus one tile in ONE group: the grid-stride loops' later trips and the offsets kernel's carry over many trips of 64 tiles, k = 8"""
    import torch
    waves = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    elements = (2 * waves + 1) * 1024 + 5
    src = np.cumsum(np.random.default_rng(3).integers(0, 1 << 62, elements, dtype=np.uint64), dtype=np.uint64)
    t = torch.from_numpy(src.view(np.int64)).cuda()
    planar = ctx.planes_split(t, elements, filter="delta")
    assert (_host(planar) == dm.split(src.view(np.uint8), 8, elements)).all()
    assert (_host(ctx.planes_join(planar, elements, 8, filter="delta")).view(np.uint64) == src).all()


def test_refusals(zstd, ctx):
    import torch
    t = torch.zeros(24, dtype=torch.uint8, device="cuda")
    for call in (lambda: ctx.planes_split(t, 4, 2, filter="xor"), lambda: ctx.planes_join(t, 4, 2, filter="xor"), lambda: ctx.seekable_compress(t, element_size=2, filter="xor"),
                 lambda: ctx.seekable_compress(t, filter="delta"), lambda: ctx.seekable_compress(t, element_size=1, filter="delta")):
        with pytest.raises(zstd.ZstdError):
            call()
    # the C calls themselves: an unknown filter, and a filter with element size 1 -- UNSUPPORTED (6), nothing queued, nothing written
    dst = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    size = torch.full((1,), -1, dtype=torch.int64, device="cuda"); status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for k, filt in ((2, 2), (4, 0x100), (1, 1), (1, 2)):
        assert ctx.L.zhip_seekable_compress_typed_filter_device(ctx.ctx, t.data_ptr(), 24, 4, k, filt, 0, dst.data_ptr(), 4096, size.data_ptr(), status.data_ptr(), s) == 6
        assert b"filter" in ctx.L.zhip_last_error()
    for call in (ctx.L.zhip_planes_split_filter_device, ctx.L.zhip_planes_join_filter_device):
        assert call(ctx.ctx, t.data_ptr(), 24, 2, 4, 2, dst.data_ptr(), s) == 6
    torch.cuda.synchronize()
    assert (_host(dst) == 0x5A).all() and int(size[0]) == -1 and status.tolist() == [-1, -1]


# ------------------------------------------------------------------------------------------------ compress and the reads
@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("frame", [1025, 4096])
def test_compress_and_read(zstd, ctx, k, frame):
    """every plane frame is libzstd's frame of the model's plane; the marker and the table are the model's; read and read_ranges return the source's bytes, also
    under a small scratch limit; libzstd decodes the whole stream to the filtered planar bytes, which planes_to_elements(filter="delta") turns into the source"""
    elements = ELEMENTS[frame]
    src = _source(k, elements)
    out = ctx.seekable_compress(_dev(src), frame_size=frame, element_size=k, filter="delta")
    raw = _host(out).tobytes()
    ref = reflib.checker()
    planes = dm.planes(src, k, frame)
    frames = [ref.compress(p, level=3) for p in planes]
    entries, ck, table_at = sc.parse(raw)
    assert not ck and len(entries) == len(planes) + 1 and entries[-1][:2] == (24, 0)
    at = 0
    for i, (c, d, _) in enumerate(entries[:-1]):
        assert raw[at:at + c] == frames[i], "plane frame %d is not libzstd's" % i
        assert d == len(planes[i])
        at += c
    assert raw[at:at + 24] == dm.marker(k, frame) and at + 24 == table_at
    assert raw == dm.stream_of(frames, planes, k, frame, False)
    rg = _ranges(k, frame, elements)
    for limit in (None, 5000):
        with zstd.device.SeekableStream(ctx, out, scratch_limit=limit) as st:
            assert st.element_size == k and st.group_elements == frame and st.filter == "delta" and st.content_size == src.size
            assert (_host(st.read()) == src).all()
            views = st.read_ranges(rg)
            assert (st.last_gather_stats["passes"] == 1) == (limit is None)
            for (o, n), v in zip(rg, views):
                assert _host(v).tobytes() == src[o:o + n].tobytes(), (o, n, limit)
            assert _host(st.read(7, 1001)).tobytes() == src[7:1008].tobytes()
    with zstd.device.SeekableStream(ctx, out, raw=True) as st:
        assert st.element_size == 1 and st.filter is None
        planar = _host(st.read()).tobytes()
    whole = b"".join(ref.decompress(raw[a:a + c], d) for (c, d, _), a in zip(entries[:-1], np.cumsum([0] + [e[0] for e in entries[:-2]]).tolist()))
    assert whole == planar == dm.split(src, k, frame).tobytes()
    assert zstd.seekable.planes_to_elements(whole, k, frame, filter="delta") == src.tobytes()
    assert zstd.seekable.elements_to_planes(src.tobytes(), k, frame, filter="delta") == planar


@pytest.mark.parametrize("finder", ["none", "wave"])
def test_other_match_finders(zstd, finder):
    """the same round trip under the literals-only and the wave finder (the host-bytes module builds the contexts): libzstd decodes every frame to the model's
    plane, the readers return the elements"""
    k, frame = 8, 4096
    src = _source(k, ELEMENTS[frame])
    data = src.tobytes()
    stream = zstd.seekable.compress(data, frame_size=frame, element_size=k, filter="delta", match_finder=finder)
    entries, _, _ = sc.parse(stream)
    ref = reflib.checker()
    planes = dm.planes(src, k, frame)
    at = 0
    for (c, d, _), p in zip(entries[:-1], planes):
        assert ref.decompress(stream[at:at + c], d) == p
        at += c
    assert stream[at:at + 24] == dm.marker(k, frame)
    assert zstd.seekable.decompress(stream) == data
    assert zstd.seekable.decompress(stream, 5, 100) == data[5:105]
    assert zstd.seekable.decompress_ranges(stream, [(3, 9), (frame * k - 1, 2)]) == [data[3:12], data[frame * k - 1:frame * k + 1]]


def test_checksums_and_damage(zstd, ctx):
    """with checksum=True: the table's checksums are those of the filtered planar content; one flipped content byte (a raw literal of plane frame 9: group 2,
    plane 1 of a k = 4 stream of random ids) fails with 22 exactly the ranges that need group 2, and no others"""
    import torch
    k, frame = 4, 1025
    elements = ELEMENTS[frame]
    src = np.random.default_rng(8).integers(0, 256, elements * k, dtype=np.uint8)      # (incompressible planes: raw blocks, so a flipped byte is a content byte)
    out = ctx.seekable_compress(_dev(src), frame_size=frame, element_size=k, checksum=True, filter="delta")
    raw = _host(out).tobytes()
    entries, ck, _ = sc.parse(raw)
    planes = dm.planes(src, k, frame)
    assert ck and [e[2] for e in entries[:-1]] == [sc.xxh64(p) & 0xFFFFFFFF for p in planes] and entries[-1][2] == pm.XXH_EMPTY
    with zstd.device.SeekableStream(ctx, out) as st:
        assert st.has_checksums and st.filter == "delta" and (_host(st.read()) == src).all()
    bad = bytearray(raw)
    bad[sum(e[0] for e in entries[:9]) + entries[9][0] // 2] ^= 0x55
    bad_t = torch.frombuffer(bad, dtype=torch.uint8).cuda()
    g = frame * k
    rg = [(10, 100), (2 * g - 3, 5), (2 * g, g), (3 * g, 37 * k), (0, src.size), (3 * g - 1, 1), (3 * g, 1), (g + 1, g - 1), (2 * g + 8, 0)]
    touches = [o < 3 * g and o + ln > 2 * g and ln > 0 for o, ln in rg]
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
        assert status[:2] == [22, 1]
        for r, ((o, ln), touch) in enumerate(zip(rg, touches)):
            assert status[2 + 2 * r:4 + 2 * r] == ([22, 9] if touch else [0, 0]), r
            if not touch:
                assert got[int(table[r, 2]):int(table[r, 2]) + ln].tobytes() == src[o:o + ln].tobytes(), r
        with pytest.raises(zstd.ZstdError):
            st.read(2 * g, 10)


def test_unfiltered_stream_held(zstd, ctx):
    """an unfiltered typed stream written through the new entry point (what seekable_compress calls now) equals the old entry point's bytes"""
    import torch
    k, frame = 4, 4096
    src = _source(k, ELEMENTS[frame])
    t = _dev(src)
    new = ctx.seekable_compress(t, frame_size=frame, element_size=k)
    assert torch.equal(new, ctx.seekable_compress(t, frame_size=frame, element_size=k, filter=None))
    bound = ctx.L.zhip_seekable_typed_bound(src.size, frame, k, 0)
    dst = torch.zeros(bound, dtype=torch.uint8, device="cuda"); size = torch.zeros(1, dtype=torch.int64, device="cuda"); status = torch.zeros(2, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()
    assert ctx.L.zhip_seekable_compress_typed_device(ctx.ctx, t.data_ptr(), src.size, frame, k, 0, dst.data_ptr(), bound, size.data_ptr(), status.data_ptr(), s.cuda_stream) == 0
    s.synchronize()
    assert status.tolist() == [0, 0] and torch.equal(dst[:int(size[0])], new)
    raw = _host(new).tobytes()
    assert raw[sc.parse(raw)[2] - 24:sc.parse(raw)[2]] == pm.marker(k, frame)
    with zstd.device.SeekableStream(ctx, new) as st:
        assert st.filter is None and st.element_size == k and (_host(st.read()) == src).all()
