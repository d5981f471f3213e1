"""Level 5 on sources of 16 385 ... 131 072 bytes, and explicit STRATEGY_GREEDY parameters in the same scope: the greedy search with libzstd's row match finder in
zhip_encode_match_greedy_kernel (ze_greedy_row). Every frame of every call is compared byte for byte with libzstd 1.5.7 (tests/reflib.checker()) at
the same level / parameters and decompressed back through the backend; nothing is sampled. What is out of scope must be refused as before: per frame with status 40
("Unsupported parameter") or when the parameters are set."""
import ctypes as C
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import greedy_sources as gs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zstd():
    import zstandard_amd
    assert zstandard_amd._lib.lib().zhip_device_count() >= 1, "no GPU visible"
    return zstandard_amd


@pytest.fixture(scope="module")
def ref():
    from tests import reflib
    return reflib.checker()


def _ref_frames(ref, raws, checksum=False, **params):
    from tests import reflib
    flags = reflib.DEFAULT_FLAGS | (reflib.F_CHECKSUM if checksum else 0)
    with ThreadPoolExecutor(16) as pool:                     # (ctypes drops the GIL)
        if params: return list(pool.map(lambda r: ref.compress_advanced(r, level=5, flags=flags, **params), raws))
        return list(pool.map(lambda r: ref.compress(r, level=5, flags=flags), raws))


@pytest.fixture(scope="module")
def aimed(corpus):
    return [r for _, r in gs.aimed_sources(corpus)]


@pytest.fixture(scope="module")
def data(corpus, aimed):
    """the aimed sources, 256 corpus sources of 131 072 bytes and 256 of 20 000"""
    from tests.corpus import Corpus
    small = Corpus(frame_size=20000, mix="silesia")
    return aimed + corpus.frame_list(2000, 256) + small.frame_list(0, 256)


@pytest.fixture(scope="module")
def want(ref, data):
    return {ck: _ref_frames(ref, data, checksum=ck) for ck in (False, True)}


def _device_run(ctx, raws):
    """raws through DeviceBatchContext.compress, slots of zhip_compress_bound back to back; returns (frames, status, first failing index by zhip_ctx_sync or None)"""
    import torch
    from zstandard_amd import _lib
    dev = torch.device("cuda", 0)
    n = len(raws)
    lens = np.array([len(r) for r in raws], dtype=np.int64)
    offs = np.zeros(n, dtype=np.int64); offs[1:] = np.cumsum(lens)[:-1]
    bound_of = {x: int(_lib.lib().zhip_compress_bound(int(x))) for x in set(lens.tolist())}
    bounds = np.array([bound_of[x] for x in lens.tolist()], dtype=np.int64)
    doffs = np.zeros(n, dtype=np.int64); doffs[1:] = np.cumsum(bounds)[:-1]

    def segs(o, l):
        a = np.zeros((n, 2), dtype=np.int64); a[:, 0] = o; a[:, 1] = l
        return torch.from_numpy(a).to(dev)

    src = torch.from_numpy(np.frombuffer(b"".join(raws), dtype=np.uint8).copy()).to(dev)
    dst = torch.zeros(int(bounds.sum()), dtype=torch.uint8, device=dev)
    out_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ctx.compress(src, segs(offs, lens), dst, segs(doffs, bounds), out_sizes, status)
    err = _lib.Error()
    rc = ctx.L.zhip_ctx_sync(ctx.ctx, torch.cuda.current_stream().cuda_stream, status.data_ptr(), n, C.byref(err))
    st = status.cpu().numpy()
    got = dst.cpu().numpy(); sz = out_sizes.cpu().numpy()
    return [got[doffs[i]: doffs[i] + sz[i]].tobytes() for i in range(n)], st, (int(err.index), int(err.zstdErr)) if rc else None


def _in_fresh_thread(env, fn):
    """fn() in a new thread (its own device context) with `env` set while it runs; returns fn's result, re-raises its exception"""
    box = {}

    def run():
        try:
            box["out"] = fn()
        except Exception as e:              # noqa: BLE001 -- re-raised below
            box["error"] = e

    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        t = threading.Thread(target=run); t.start(); t.join()
    finally:
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    if "error" in box:
        raise box["error"]
    return box["out"]


def _differing(got, want):
    return [i for i in range(len(want)) if got[i] != want[i]]


@pytest.mark.parametrize("checksum", [False, True], ids=["plain", "checksum"])
def test_frames_are_libzstds_through_the_batch_api(zstd, data, want, checksum):
    res = zstd.ZstdCompressor(level=5, write_checksum=checksum).multi_compress_to_buffer(data)
    got = [res[i].tobytes() for i in range(len(data))]
    bad = _differing(got, want[checksum])
    assert not bad, (len(bad), bad[:8], [len(data[i]) for i in bad[:8]])
    back = zstd.ZstdDecompressor().multi_decompress_to_buffer(got)
    assert [back[i].tobytes() for i in range(len(data))] == data


@pytest.mark.parametrize("checksum", [False, True], ids=["plain", "checksum"])
def test_frames_are_libzstds_through_a_device_context(zstd, data, want, checksum):
    from zstandard_amd.device import DeviceBatchContext
    ctx = DeviceBatchContext(level=5, write_checksum=checksum)
    try:
        ctx.kernel_time(5)
        got, st, first = _device_run(ctx, data)
        launches = {k: ctx.kernel_time(k)[1] for k in (1, 5, 6, 8)}
    finally:
        ctx.close()
    assert not st.any() and first is None, (np.nonzero(st)[0][:8], first)
    assert launches[5] == 1 and launches[6] == 1 and launches[8] == 0 and launches[1] == 0, ("one lane-serial match launch, one entropy launch, no flat search", launches)
    bad = _differing(got, want[checksum])
    assert not bad, (len(bad), bad[:8], [len(data[i]) for i in bad[:8]])
    back = zstd.ZstdDecompressor().multi_decompress_to_buffer(got)
    assert [back[i].tobytes() for i in range(len(data))] == data


@pytest.mark.parametrize("checksum", [False, True], ids=["plain", "checksum"])
def test_frames_are_libzstds_one_source_at_a_time(zstd, data, aimed, want, checksum):
    """.compress(): a batch of one through the same two kernels. One call is one source's whole serial search with nothing beside it, so the aimed sources and eight
    corpus sources of either size go through it one by one, not all 512 (the batch tests above run all of them through the same kernels)"""
    idx = list(range(len(aimed))) + list(range(len(aimed), len(aimed) + 8)) + list(range(len(aimed) + 256, len(aimed) + 264))
    c = zstd.ZstdCompressor(level=5, write_checksum=checksum)
    d = zstd.ZstdDecompressor()
    for i in idx:
        got = c.compress(data[i])
        assert got == want[checksum][i], (i, len(data[i]))
        assert d.decompress(got) == data[i]


@pytest.mark.parametrize("kw", gs.PARAM_SETS[1:], ids=["search_log=%d" % k["search_log"] if "search_log" in k else "min_match=%d" % k["min_match"] for k in gs.PARAM_SETS[1:]])
def test_explicit_greedy_parameters(zstd, ref, aimed, corpus, kw):
    """strategy=STRATEGY_GREEDY with search_log 1 ... 4 / min_match 3, 5, 6, 7 over level 5's row: the aimed sources and 24 of other sizes against the checker with the same parameters"""
    raws = aimed + [corpus.frame_bytes(2300 + i)[: 16385 + 977 * i] for i in range(24)]
    got = _explicit(zstd, raws, kw)
    bad = _differing(got, _ref_frames(ref, raws, **kw))
    assert not bad, (kw, len(bad), bad[:8], [len(raws[i]) for i in bad[:8]])


def _explicit(zstd, raws, kw):
    """explicit fields over level 5's row, through a device context (it takes a level and explicit fields together, as the checker does)"""
    from zstandard_amd.device import DeviceBatchContext
    ctx = DeviceBatchContext(level=5, **kw)
    try:
        got, st, first = _device_run(ctx, raws)
    finally:
        ctx.close()
    assert not st.any() and first is None, (kw, np.nonzero(st)[0][:8], first)
    return got


def test_explicit_greedy_parameters_object(zstd, ref, aimed):
    """the same through ZstdCompressor(compression_params=ZstdCompressionParameters(strategy=STRATEGY_GREEDY, ...)): unset fields are the default level's row there"""
    kw = dict(strategy=zstd.STRATEGY_GREEDY, search_log=3, min_match=5, window_log=17, hash_log=16)
    res = zstd.ZstdCompressor(compression_params=zstd.ZstdCompressionParameters(**kw)).multi_compress_to_buffer(aimed)
    with ThreadPoolExecutor(16) as pool:
        wanted = list(pool.map(lambda r: ref.compress_advanced(r, level=3, flags=1, **kw), aimed))
    bad = _differing([res[i].tobytes() for i in range(len(aimed))], wanted)
    assert not bad, (len(bad), bad[:8])


def test_several_waves_of_mixed_sizes(zstd, ref, corpus):
    """2 049 sources of 1 ... 131 072 bytes in one batch: sources of 16 384 bytes and less (level 5 is lazy there) come back refused with status 40 at their own index
    while their neighbours compress; zhip_ctx_sync reports the lowest such index"""
    from zstandard_amd.device import DeviceBatchContext
    rng = np.random.default_rng(41)
    pool = [corpus.frame_bytes(2400 + i) for i in range(32)]
    sizes = [int(rng.choice([1, 3, 6, 7, 20, 63, 64, 1000, 16384, 16385, 17000, 20000, 33333, 65536, 131071, 131072],
                            p=[.01, .01, .01, .01, .01, .01, .01, .02, .02, .1, .2, .3, .1, .1, .04, .05])) for _ in range(2049)]
    sizes[0], sizes[5], sizes[2048] = 20000, 6, 131072
    raws = [pool[i % 32][o: o + n] for i, (n, o) in enumerate(zip(sizes, rng.integers(0, 1000, 2049).tolist()))]
    assert any(n < 7 for n in sizes) and any(7 <= n < 64 for n in sizes) and any(64 <= n <= 16384 for n in sizes)
    ctx = DeviceBatchContext(level=5)
    try:
        got, st, first = _device_run(ctx, raws)
    finally:
        ctx.close()
    refused = [i for i, n in enumerate(sizes) if n <= 16384]
    assert [i for i in range(2049) if st[i] != 0] == refused and all(st[i] == 40 for i in refused), ([i for i in range(2049) if st[i] != 0][:8], refused[:8])
    assert first == (refused[0], 40), (first, refused[0])
    served = [i for i, n in enumerate(sizes) if n > 16384]
    wanted = _ref_frames(ref, [raws[i] for i in served])
    bad = [i for k, i in enumerate(served) if got[i] != wanted[k]]
    assert not bad, (len(bad), bad[:8], [sizes[i] for i in bad[:8]])
    back = zstd.ZstdDecompressor().multi_decompress_to_buffer([got[i] for i in served])
    assert [back[k].tobytes() for k in range(len(served))] == [raws[i] for i in served]


def test_out_of_scope_is_still_refused(zstd, corpus):
    """each of these raised ZstdError before level 5 existed and still does"""
    text = corpus.frame_bytes(9)
    samples = [corpus.frame_bytes(2500 + i)[:4096] for i in range(64)]
    d = zstd.ZstdCompressionDict(b"".join(samples)[:8192])
    with pytest.raises(zstd.ZstdError):                      # any dictionary
        zstd.ZstdCompressor(level=5, dict_data=d).multi_compress_to_buffer([text[:20000], text])
    with pytest.raises(zstd.ZstdError):                      # a source of several blocks
        zstd.ZstdCompressor(level=5).multi_compress_to_buffer([text + text])
    with pytest.raises(zstd.ZstdError):                      # rows of 32 entries
        zstd.ZstdCompressor(compression_params=zstd.ZstdCompressionParameters(strategy=zstd.STRATEGY_GREEDY, search_log=5)).multi_compress_to_buffer([text])
    with pytest.raises(zstd.ZstdError):                      # tables above hashLog 17
        zstd.ZstdCompressor(compression_params=zstd.ZstdCompressionParameters(strategy=zstd.STRATEGY_GREEDY, window_log=17, hash_log=18)).multi_compress_to_buffer([text])
    with pytest.raises(zstd.ZstdError):                      # a window that does not cover the source
        zstd.ZstdCompressor(compression_params=zstd.ZstdCompressionParameters(strategy=zstd.STRATEGY_GREEDY, window_log=15)).multi_compress_to_buffer([text[:40000]])
    with pytest.raises(zstd.ZstdError):                      # lazy
        zstd.ZstdCompressor(level=6).multi_compress_to_buffer([text])
    with pytest.raises(zstd.ZstdError):                      # greedy below the row match finder's window: the hash-chain finder
        zstd.ZstdCompressor(level=5).multi_compress_to_buffer([text[:16384]])


def test_tables_across_calls(zstd, ref, corpus):
    """one thread's context: level 5, level 3, level 5 again on the same sources shuffled. The lane-serial kernel's table slots hold rows of positions and tags, then two
    hash tables' worth of other cells is in the flat tables, then rows again -- nothing stale may survive (each source's slot is zeroed before its search)"""
    rng = np.random.default_rng(42)
    raws = [corpus.frame_bytes(2600 + i)[: int(rng.integers(16385, 131073))] for i in range(96)]
    shuffled = [raws[i] for i in rng.permutation(len(raws))]
    steps = [(raws, 5), (raws, 3), (shuffled, 5), (shuffled, 3), (raws, 5)]

    def run():
        out = []
        for rs, level in steps:
            res = zstd.ZstdCompressor(level=level).multi_compress_to_buffer(rs)
            out.append([res[i].tobytes() for i in range(len(rs))])
        return out

    out = _in_fresh_thread({}, run)
    cache = {}
    for k, (rs, level) in enumerate(steps):
        key = (id(rs), level)
        if key not in cache:
            with ThreadPoolExecutor(16) as pool: cache[key] = list(pool.map(lambda r: ref.compress(r, level=level), rs))
        bad = _differing(out[k], cache[key])
        assert not bad, ("call %d, level %d" % (k, level), len(bad), bad[:8])


@pytest.mark.parametrize("n", [9, 32769, 65537])
def test_launch_shapes(zstd, ref, corpus, n):
    """The lane-serial kernel's shapes, each in a fresh context. 9 sources: two waves of eight lanes, the second with one busy lane. 32 769 sources of 16 385 ... 17 408 bytes:
    batches above 32 768 sources run sixteen sources per wave in chunks of 65 536, and there are more sources than table slots, so every lane searches several sources in the
    slot it zeroes each time. 65 537 sources: two chunks (65 536 and 1) -- one-byte sources, refused at their own index, around ~600 served ones in both chunks, the last
    index among them"""
    from zstandard_amd.device import DeviceBatchContext
    rng = np.random.default_rng(43)
    pool = b"".join(corpus.frame_bytes(2700 + i) for i in range(16))
    served = list(range(n)) if n < 65537 else sorted(set(range(0, n, 113)) | {7, 32767, 32768, 65535, 65536})
    raws = [b"x"] * n
    for i, o, m in zip(served, rng.integers(0, len(pool) - 17408, len(served)).tolist(), rng.integers(16385, 17409, len(served)).tolist()): raws[i] = pool[o: o + m]

    def run():
        ctx = DeviceBatchContext(level=5, write_checksum=True)
        try:
            ctx.kernel_time(5)
            got, st, first = _device_run(ctx, raws)
            return got, st, first, {k: ctx.kernel_time(k)[1] for k in (1, 5, 6, 8)}
        finally:
            ctx.close()

    got, st, first, launches = _in_fresh_thread({}, run)
    refused = sorted(set(range(n)) - set(served))
    assert np.nonzero(st)[0].tolist() == refused and all(st[i] == 40 for i in refused) and first == ((refused[0], 40) if refused else None), (np.nonzero(st)[0][:8], first)
    chunks = (n + 65535) // 65536
    assert launches[5] == chunks and launches[6] == chunks and launches[8] == 0 and launches[1] == 0, launches
    want = _ref_frames(ref, [raws[i] for i in served], checksum=True)
    bad = [i for k, i in enumerate(served) if got[i] != want[k]]
    assert not bad, (n, len(bad), bad[:8], [len(raws[i]) for i in bad[:8]])
