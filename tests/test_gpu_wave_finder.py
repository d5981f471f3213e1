"""The wave-parallel match finder on the MI355X (DeviceBatchContext(match_finder="wave"): zhip_ctx_set_match_finder(ZHIP_FINDER_WAVE), zhip_encode_match_wave_kernel).
Its frames are valid zstd, not libzstd's bytes: every frame is decoded by libzstd 1.5.7 and by the backend's own decoder, and compared with what the host emulator
wrote for the same source (tests/golden/wave_finder.json, tests/golden/make_wave_finder.py) -- the output is a pure function of source and parameters. Launch counts,
launch shapes, refusals, a context that alternates finders, and the seekable calls."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from tests import wave_sources as ws

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CANARY = 64
WAVE_TIMER, TIMERS = 10, (1, 5, 6, 8, 10)


@pytest.fixture(scope="module")
def zstd():
    import zstandard_amd
    assert zstandard_amd._lib.lib().zhip_device_count() >= 1, "no GPU visible"
    assert zstandard_amd._lib.lib().zhip_kernel_name(WAVE_TIMER) == b"zhip_encode_match_wave_kernel"
    return zstandard_amd


@pytest.fixture(scope="module")
def ref():
    from tests import reflib
    return reflib.checker()


@pytest.fixture(scope="module")
def sources(corpus):
    return ws.all_sources(corpus)


@pytest.fixture(scope="module")
def fixture():
    fx = json.load(open(os.path.join(HERE, "golden", "wave_finder.json")))
    return {row["name"]: (row["size"], row["sha256"]) for row in fx["frames"] + fx["all_frames"]}


def _run(ctx, raws):
    """raws through ctx.compress: sources packed back to back in an allocation of exactly their size (the last one ends at its end), every destination slot of
    zhip_compress_bound bytes between two canaries. Returns (frames, statuses, what zhip_ctx_sync reports or None)."""
    import torch
    from zstandard_amd import _lib
    dev = torch.device("cuda", 0)
    n = len(raws)
    lens = np.array([len(r) for r in raws], dtype=np.int64)
    offs = np.zeros(n, dtype=np.int64); offs[1:] = np.cumsum(lens)[:-1]
    bound_of = {x: int(_lib.lib().zhip_compress_bound(int(x))) for x in set(lens.tolist())}
    bounds = np.array([bound_of[x] for x in lens.tolist()], dtype=np.int64)
    doffs = CANARY + np.concatenate([[0], np.cumsum(bounds + CANARY)[:-1]]).astype(np.int64)

    def segs(o, l):
        a = np.zeros((n, 2), dtype=np.int64); a[:, 0] = o; a[:, 1] = l
        return torch.from_numpy(a).to(dev)

    joined = b"".join(raws)
    src = torch.from_numpy(np.frombuffer(joined, dtype=np.uint8).copy()).to(dev) if joined else torch.zeros(1, dtype=torch.uint8, device=dev)
    dst = torch.full((int(doffs[-1] + bounds[-1] + CANARY),), 0xC5, dtype=torch.uint8, device=dev)
    out_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ctx.compress(src, segs(offs, lens), dst, segs(doffs, bounds), out_sizes, status)
    err = _lib.Error()
    rc = ctx.L.zhip_ctx_sync(ctx.ctx, torch.cuda.current_stream().cuda_stream, status.data_ptr(), n, C.byref(err))
    st = status.cpu().numpy(); got = dst.cpu().numpy(); sz = out_sizes.cpu().numpy()
    keep = np.ones(got.size, dtype=bool)
    for i in range(n):
        keep[doffs[i]: doffs[i] + bounds[i]] = False
    assert (got[keep] == 0xC5).all(), "bytes outside the destination slots were written"
    assert ((0 <= sz) & (sz <= bounds)).all()                                                   # (inside its own slot a kernel may write past the frame it ends up with)
    return [got[doffs[i]: doffs[i] + sz[i]].tobytes() for i in range(n)], st.tolist(), (int(err.index), int(err.zstdErr)) if rc else None


def _libzstd_whole(ref, stream, size):
    """ZSTD_decompress: every frame of the stream, the skippable table frame passed over"""
    L = ref.lib
    L.ZSTD_decompress.restype = C.c_size_t
    L.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    dst = C.create_string_buffer(max(size, 1))
    r = L.ZSTD_decompress(dst, size, stream, len(stream))
    assert not L.ZSTD_isError(r), L.ZSTD_getErrorName(r)
    return dst.raw[:r]


def _ctx(zstd, **kw):
    from zstandard_amd.device import DeviceBatchContext
    return DeviceBatchContext(match_finder="wave", **kw)


def _is_fixture(fixture, names, frames):
    for name, f in zip(names, frames):
        assert (len(f), hashlib.sha256(f).hexdigest()) == fixture[name], "%s: the GPU's frame is not the emulator's" % name


def test_source_set_decodes_and_equals_the_emulator(zstd, ref, sources, fixture):
    names, raws = [n for n, _ in sources], [r for _, r in sources]
    ctx = _ctx(zstd, level=3)
    try:
        ctx.kernel_time(WAVE_TIMER)
        got, st, first = _run(ctx, raws)
        launches = {k: ctx.kernel_time(k)[1] for k in TIMERS}
    finally:
        ctx.close()
    assert not any(st) and first is None, (st, first)
    assert launches == {1: 0, 5: 0, 6: 1, 8: 0, 10: 1}, ("the wave kernel once, the entropy kernel once, no other search", launches)
    for name, raw, f in zip(names, raws, got):
        assert ref.decompress(f, len(raw)) == raw, name
    back = zstd.ZstdDecompressor().multi_decompress_to_buffer(got)
    assert [back[i].tobytes() for i in range(len(raws))] == raws
    _is_fixture(fixture, names, got)


@pytest.mark.parametrize("level,checksum", [(1, True), (-3, False)], ids=["level 1, checksum", "level -3"])
def test_other_levels_decode(zstd, ref, sources, level, checksum):
    raws = [r for _, r in sources]
    ctx = _ctx(zstd, level=level, write_checksum=checksum)
    try:
        got, st, first = _run(ctx, raws)
    finally:
        ctx.close()
    assert not any(st) and first is None
    for (name, raw), f in zip(sources, got):
        assert ref.decompress(f, len(raw)) == raw, name
    back = zstd.ZstdDecompressor().multi_decompress_to_buffer(got)
    assert [back[i].tobytes() for i in range(len(raws))] == raws


def _shape_sources(corpus, shape):
    text = corpus.frame_bytes(9)
    if shape == "n=1": return [text[:50000]]
    if shape == "n=65": return [text[i * 100: i * 100 + 3000 + 37 * i] for i in range(65)]
    if shape == "n=4097": return [text[i: i + 1 + i % 4096] for i in range(4097)]              # 1 ... 4 096 bytes: more sources than resident waves
    assert shape == "n=65537"
    return [text[i % 1000: i % 1000 + (200 if i % 2 else 1)] for i in range(65537)]               # two chunks


@pytest.mark.parametrize("shape", ["n=1", "n=65", "n=4097", "n=65537"])
def test_launch_shapes_in_fresh_contexts(zstd, ref, corpus, shape):
    raws = _shape_sources(corpus, shape)
    chunks = (len(raws) + 65535) // 65536
    ctx = _ctx(zstd, level=3)
    try:
        ctx.kernel_time(WAVE_TIMER)
        got, st, first = _run(ctx, raws)
        launches = {k: ctx.kernel_time(k)[1] for k in TIMERS}
    finally:
        ctx.close()
    assert not any(st) and first is None
    assert launches == {1: 0, 5: 0, 6: chunks, 8: 0, 10: chunks}, launches
    back = zstd.ZstdDecompressor().multi_decompress_to_buffer(got)
    assert [back[i].tobytes() for i in range(len(raws))] == raws
    for i in list(range(0, len(raws), max(1, len(raws) // 200))) + [len(raws) - 1]:               # libzstd on a spread of them (the backend's decoder took all)
        assert ref.decompress(got[i], len(raws[i])) == raws[i], i


def test_mixed_batch_refuses_sources_of_several_blocks_at_their_own_index(zstd, ref, corpus, fixture):
    text = corpus.frame_bytes(9)
    small = ws.small_sources(corpus)[:6]
    raws = [small[0][1], small[1][1], text + text[:1], small[2][1], (text * 3)[:300000], small[3][1], small[4][1], small[5][1]]
    ctx = _ctx(zstd, level=3)
    try:
        got, st, first = _run(ctx, raws)
    finally:
        ctx.close()
    assert st == [0, 0, 40, 0, 40, 0, 0, 0] and first == (2, 40), (st, first)                     # zhip_ctx_sync reports the lowest
    assert got[2] == b"" and got[4] == b""
    _is_fixture(fixture, [n for n, _ in small], [got[i] for i in (0, 1, 3, 5, 6, 7)])


def test_refusals(zstd, corpus):
    text = corpus.frame_bytes(9)
    # (strategy 4 is refused where the parameters are set, as for every finder; a dictionary, level 5 and explicit greedy parameters by the call, naming the finder)
    for kw, msg in ((dict(level=3, dict_data=text[:4000]), "wave match finder"), (dict(level=5), "wave match finder"), (dict(level=3, strategy=3, search_log=4), "wave match finder"),
                    (dict(level=3, strategy=4), "could not set compression parameters")):
        ctx = _ctx(zstd, **kw)
        try:
            with pytest.raises(zstd.ZstdError, match=msg):
                _run(ctx, [text[:40000]])
        finally:
            ctx.close()
    # a window that does not cover the source: known only per source -- status 40 from compress, ZstdError from the calls that wait for the result
    ctx = _ctx(zstd, level=3, window_log=10)
    try:
        got, st, first = _run(ctx, [text[:40000], text[:1000]])
        assert st == [40, 0] and first == (0, 40)
        import torch
        with pytest.raises(zstd.ZstdError, match="Unsupported parameter"):
            ctx.seekable_compress(torch.from_numpy(np.frombuffer(text[:40000], dtype=np.uint8).copy()).cuda())
    finally:
        ctx.close()
    from zstandard_amd.device import DeviceBatchContext
    with pytest.raises(zstd.ZstdError, match="match_finder"):
        DeviceBatchContext(match_finder="lazy")                                                # refused before a native context exists
    ctx = _ctx(zstd)
    try:
        with pytest.raises(zstd.ZstdError, match="match_finder"):
            ctx.set_match_finder("lazy")
        assert ctx.match_finder == "wave"                                                       # the finder stays what it was
    finally:
        ctx.close()


def test_one_context_alternating_finders(zstd, ref, corpus, fixture):
    small = ws.small_sources(corpus)
    order = np.random.default_rng(5).permutation(len(small)).tolist()
    names, raws = [small[i][0] for i in order], [small[i][1] for i in order]
    want = [ref.compress(r, level=3) for r in raws]
    from zstandard_amd.device import DeviceBatchContext
    ctx = DeviceBatchContext(level=3)
    try:
        for finder in ("wave", "libzstd", "wave", "libzstd"):
            ctx.set_match_finder(finder)
            got, st, first = _run(ctx, raws)
            assert not any(st) and first is None, finder
            if finder == "wave": _is_fixture(fixture, names, got)
            else: assert got == want, "the default finder's frames are libzstd's"
    finally:
        ctx.close()


def test_seekable_streams(zstd, ref, corpus):
    import torch
    from zstandard_amd import seekable
    from zstandard_amd.device import DeviceBatchContext, SeekableStream
    content = b"".join(corpus.frame_bytes(30 + i) for i in range(3)) + corpus.frame_bytes(9)[:1000]
    assert len(content) == 3 * 131072 + 1000
    default = seekable.compress(content, level=3, frame_size=131072)
    stream = seekable.compress(content, level=3, frame_size=131072, match_finder="wave")
    assert stream != default and stream == seekable.compress(content, level=3, frame_size=131072, match_finder="wave")
    assert _libzstd_whole(ref, stream, len(content)) == content                                 # the reference's decoder reads the stream whole
    ctx = DeviceBatchContext()
    try:
        with SeekableStream(ctx, torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()) as st:
            assert st.n_frames == 4
            assert st.read(131072 - 77, 131072 + 500).cpu().numpy().tobytes() == content[131072 - 77: 2 * 131072 + 423]
    finally:
        ctx.close()
    text = corpus.frame_bytes(9) + corpus.frame_bytes(10)
    records = [text[i * 3000: i * 3000 + 1 + (i * 131) % 8192] for i in range(64)]
    rstream = seekable.compress_records(records, level=3, match_finder="wave")
    assert rstream != seekable.compress_records(records, level=3)
    assert _libzstd_whole(ref, rstream, sum(len(r) for r in records)) == b"".join(records)
    assert seekable.decompress_records(rstream, [63, 0, 17]) == [records[63], records[0], records[17]]
    with pytest.raises(zstd.ZstdError):
        seekable.compress(content, level=3, frame_size=262144, match_finder="wave")            # frames of several blocks: refused, never the other finder quietly
