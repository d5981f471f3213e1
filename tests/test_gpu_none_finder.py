"""match_finder="none" on the MI355X (DeviceBatchContext(match_finder="none"): zhip_ctx_set_match_finder(ZHIP_FINDER_NONE), zhip_encode_none_kernel -- one kernel per chunk
in place of the match kernels and the entropy kernel, the source itself read as the block's literals). Its frames are libzstd's: every frame is compared byte for byte
with libzstd 1.5.7's ZSTD_compressSequences frame of the list that is only the block delimiter (RefZstd.compress_sequences(data, [], len(data))) and with what
ctx.compress_sequences writes for count 0 on the same device, and decoded by the backend. Launch counts, launch shapes, refusals, a context that alternates the three
finders, and the seekable calls."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import none_sources as ns
from tests import planes_model as pm
from tests import reflib
from tests import seekable_cases as sc

pytestmark = pytest.mark.gpu
CANARY = 64
NONE_TIMER, OTHER_TIMERS = 11, (5, 6, 8, 10)
CHUNK = 65536                                       # ze_none_plan (tests/test_emu_none_finder.py::test_plan holds it)


@pytest.fixture(scope="module")
def zstd():
    import zstandard_amd
    import zstandard_amd.device  # noqa: F401
    import zstandard_amd.seekable  # noqa: F401
    assert zstandard_amd._lib.lib().zhip_device_count() >= 1, "no GPU visible"
    assert zstandard_amd._lib.lib().zhip_kernel_name(NONE_TIMER) == b"zhip_encode_none_kernel"
    assert zstandard_amd._lib.lib().zhip_abi_version() == 3
    return zstandard_amd


@pytest.fixture(scope="module")
def ref():
    return reflib.checker()


@pytest.fixture(scope="module")
def big_set(corpus):
    """[(name, bytes)]: the aimed set, 256 corpus sources of 20 000 bytes and 64 of 131 072"""
    return ([(n, r) for n, r, _ in ns.aimed_sources(corpus)] + [("corpus %d, 20000" % i, r[:20000]) for i, r in enumerate(corpus.frame_list(0, 256))]
            + [("corpus %d, 131072" % i, r) for i, r in enumerate(corpus.frame_list(256, 64))])


def _flags(checksum):
    return reflib.F_CONTENTSIZE | reflib.F_DICTID | (reflib.F_CHECKSUM if checksum else 0)


def _literals_only(ref, raw, level=3, checksum=False):
    return ref.compress_sequences(raw, [], len(raw), level=level, flags=_flags(checksum))


def _run(ctx, raws, sequences=False):
    """raws through ctx.compress (sequences: through ctx.compress_sequences with an empty list for every source): sources packed back to back in an allocation of
    exactly their size (the last one ends at its end), every destination slot of zhip_compress_bound bytes between two canaries. Returns (frames, statuses, what
    zhip_ctx_sync reports or None)."""
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
    if sequences:
        ctx.compress_sequences(src, segs(offs, lens), torch.zeros(1, dtype=torch.int64, device=dev), segs(0, 0), dst, segs(doffs, bounds), out_sizes, status)
    else:
        ctx.compress(src, segs(offs, lens), dst, segs(doffs, bounds), out_sizes, status)
    err = _lib.Error()
    rc = ctx.L.zhip_ctx_sync(ctx.ctx, torch.cuda.current_stream().cuda_stream, status.data_ptr(), n, C.byref(err))
    st = status.cpu().numpy(); got = dst.cpu().numpy(); sz = out_sizes.cpu().numpy()
    canaries = np.concatenate([np.arange(CANARY), ((doffs + bounds)[:, None] + np.arange(CANARY)[None, :]).reshape(-1)])
    assert (got[canaries] == 0xC5).all(), "bytes outside the destination slots were written"
    assert ((0 <= sz) & (sz <= bounds)).all()                                                   # (inside its own slot a kernel may write past the frame it ends up with)
    return [got[doffs[i]: doffs[i] + sz[i]].tobytes() for i in range(n)], st.tolist(), (int(err.index), int(err.zstdErr)) if rc else None


def _ctx(finder="none", **kw):
    from zstandard_amd.device import DeviceBatchContext
    return DeviceBatchContext(match_finder=finder, **kw)


def _in_fresh_thread(fn):
    """fn() in a thread of its own (a context created, used and closed there); re-raises what it raised"""
    box = {}

    def body():
        try:
            box["value"] = fn()
        except BaseException as e:                                   # noqa: BLE001
            box["error"] = e

    t = threading.Thread(target=body)
    t.start(); t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


def _timed_run(raws, sequences_too=True, **kw):
    """raws through a fresh "none" context: (frames, statuses, first error, launches by timer, frames of compress_sequences with count 0 on the same device)"""
    ctx = _ctx(**kw)
    try:
        ctx.kernel_time(NONE_TIMER)
        got, st, first = _run(ctx, raws)
        launches = {k: ctx.kernel_time(k)[1] for k in (NONE_TIMER,) + OTHER_TIMERS}
        by_seq = _run(ctx, raws, sequences=True) if sequences_too else None
    finally:
        ctx.close()
    return got, st, first, launches, by_seq


@pytest.mark.parametrize("checksum", [False, True], ids=["plain", "checksum"])
def test_frames_are_libzstds_literals_only_frames(zstd, ref, corpus, big_set, checksum):
    names, raws = [n for n, _ in big_set], [r for _, r in big_set]
    aimed = ns.aimed_sources(corpus)
    assert names[:len(aimed)] == [n for n, _, _ in aimed]
    for name, raw, prop in aimed:                                                               # the property first, from libzstd's own frame
        ns.check_property(name, _literals_only(ref, raw, checksum=checksum), prop)
    got, st, first, launches, by_seq = _timed_run(raws, write_checksum=checksum)
    assert not any(st) and first is None, (st, first)
    assert launches == {11: 1, 5: 0, 6: 0, 8: 0, 10: 0}, ("the literals-only kernel once, no match kernel, no entropy kernel", launches)
    for name, raw, f in zip(names, raws, got):
        assert f == _literals_only(ref, raw, checksum=checksum), name
    assert by_seq[1] == st and by_seq[0] == got, "zhip_compress_sequences_device with count 0 writes other frames on this device"
    back = zstd.ZstdDecompressor().multi_decompress_to_buffer(got)
    assert [back[i].tobytes() for i in range(len(raws))] == raws


@pytest.mark.parametrize("shape", ["n=1", "resident waves + 3", "one chunk + 1"])
def test_launch_shapes_in_fresh_contexts(zstd, ref, corpus, shape):
    text = corpus.frame_bytes(9)

    def body():
        if shape == "n=1":
            raws = [text[:50000]]
        elif shape == "resident waves + 3":
            ctx = _ctx()
            try:
                grid = ctx.entropy_grid()
            finally:
                ctx.close()
            raws = [text[i: i + 300] for i in range(grid + 3)]                                  # every wave takes several
        else:
            raws = [text[i % 5000: i % 5000 + 64 + i % 237] for i in range(CHUNK + 1)]              # 64 ... 300 bytes, two launches
        return raws, _timed_run(raws)

    raws, (got, st, first, launches, by_seq) = _in_fresh_thread(body)
    chunks = (len(raws) + CHUNK - 1) // CHUNK
    assert not any(st) and first is None
    assert launches == {11: chunks, 5: 0, 6: 0, 8: 0, 10: 0}, launches
    assert by_seq[1] == st and by_seq[0] == got                                                  # every frame against the device's own count-0 frames ...
    # ... and against libzstd the first and the last 512 only: a libzstd context per source takes longer than the rest of the test over 65 537 sources, and the
    # count-0 frames they all equal are held to libzstd source by source in tests/test_gpu_entropy_sequences.py and above
    for i in sorted(set(list(range(min(512, len(raws)))) + list(range(max(0, len(raws) - 512), len(raws))))):
        assert got[i] == _literals_only(ref, raws[i]), i


def test_mixed_batch_refuses_at_the_sources_own_index(zstd, ref, corpus):
    text = corpus.frame_bytes(9) + corpus.frame_bytes(10)
    sizes = [1, 131072, 131073, 7, 300000, 64, 131071, 262144, 5000, 6, 131072, 131073, 40960]
    raws = [text[:n] if n <= len(text) else (text * 2)[:n] for n in sizes]
    refused = [i for i, n in enumerate(sizes) if n > 131072]
    assert refused == [2, 4, 7, 11]
    got, st, first, _, _ = _timed_run(raws, sequences_too=False)
    assert st == [40 if i in refused else 0 for i in range(len(sizes))] and first == (2, 40), (st, first)          # zhip_ctx_sync reports the lowest
    for i, raw in enumerate(raws):
        assert got[i] == (b"" if i in refused else _literals_only(ref, raw)), i
    # level 4: the row of sources of 16 384 bytes and below is greedy -- refused one by one, the larger ones served
    got, st, first, _, _ = _timed_run([text[:40000], text[:16384], text[:16385]], sequences_too=False, level=4)
    assert st == [0, 40, 0] and first == (1, 40) and got[2] == _literals_only(ref, text[:16385], level=4)


def test_refusals(zstd, corpus):
    text = corpus.frame_bytes(9)
    for kw in (dict(level=3, dict_data=text[:4000]), dict(level=5)):
        ctx = _ctx(**kw)
        try:
            with pytest.raises(zstd.ZstdError, match="none"):
                _run(ctx, [text[:40000]])
        finally:
            ctx.close()
    from zstandard_amd.device import DeviceBatchContext
    assert DeviceBatchContext.MATCH_FINDERS["none"] == 2
    with pytest.raises(zstd.ZstdError, match="match_finder"):
        DeviceBatchContext(match_finder="lazy")                                                # refused before a native context exists
    ctx = _ctx()
    try:
        with pytest.raises(zstd.ZstdError, match="match_finder"):
            ctx.set_match_finder("lazy")
        assert ctx.match_finder == "none"                                                       # the finder stays what it was
        assert ctx.L.zhip_ctx_set_match_finder(ctx.ctx, 3) != 0
        got, st, _ = _run(ctx, [text[:3000]])
        assert st == [0] and got[0] == _literals_only(reflib.checker(), text[:3000])
    finally:
        ctx.close()


def test_one_context_alternating_finders(zstd, ref, corpus):
    raws = [r[: 1 + (i * 5471) % 131072] for i, r in enumerate(corpus.frame_list(300, 96))]
    fresh = {}
    for finder in ("libzstd", "none", "wave"):
        ctx = _ctx(finder)
        try:
            fresh[finder], st, first = _run(ctx, raws)
            assert not any(st) and first is None, finder
        finally:
            ctx.close()
    assert fresh["libzstd"] == [ref.compress(r, level=3) for r in raws]
    assert fresh["none"] == [_literals_only(ref, r) for r in raws]
    assert fresh["none"] != fresh["libzstd"] and fresh["wave"] != fresh["libzstd"]
    ctx = _ctx("libzstd")
    try:
        for finder in ("libzstd", "none", "wave", "none", "libzstd"):
            ctx.set_match_finder(finder)
            got, st, first = _run(ctx, raws)
            assert not any(st) and first is None, finder
            assert got == fresh[finder], "after a switch to %r the context writes other frames than a fresh one" % finder
    finally:
        ctx.close()


def _dev(data):
    import torch
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def _libzstd_frame_by_frame(ref, stream, contents):
    """every frame of the stream read by libzstd on its own, in the table's order"""
    entries, _, _ = sc.parse(stream)
    at = 0
    assert len(entries) == len(contents)
    for (c, d, _), want in zip(entries, contents):
        assert d == len(want) and ref.decompress(stream[at:at + c], d) == want
        at += c


def test_seekable_streams(zstd, ref, corpus):
    from zstandard_amd import seekable
    from zstandard_amd.device import DeviceBatchContext, SeekableStream
    content = b"".join(corpus.frame_bytes(30 + i) for i in range(3)) + corpus.frame_bytes(9)[:1000]
    pieces = [content[i: i + 131072] for i in range(0, len(content), 131072)]
    stream = seekable.compress(content, level=3, frame_size=131072, match_finder="none")
    assert stream != seekable.compress(content, level=3, frame_size=131072)
    _libzstd_frame_by_frame(ref, stream, pieces)
    entries, _, _ = sc.parse(stream)
    at = 0
    for (c, _, _), piece in zip(entries, pieces):
        assert stream[at:at + c] == _literals_only(ref, piece); at += c
    ctx = DeviceBatchContext()
    try:
        with SeekableStream(ctx, _dev(stream)) as st:
            assert st.n_frames == 4
            for o, n in ((0, 10), (131072 - 77, 131072 + 500), (3 * 131072 - 1, 1001)):
                assert st.read(o, n).cpu().numpy().tobytes() == content[o: o + n], (o, n)
    finally:
        ctx.close()
    with pytest.raises(zstd.ZstdError):
        seekable.compress(content, level=3, frame_size=262144, match_finder="none")            # frames of several blocks: refused, never another finder quietly
    text = corpus.frame_bytes(9) + corpus.frame_bytes(10)
    records = [text[i * 3000: i * 3000 + 1 + (i * 131) % 8192] for i in range(64)]
    rstream = seekable.compress_records(records, level=3, match_finder="none")
    _libzstd_frame_by_frame(ref, rstream, records)
    assert seekable.decompress_records(rstream, [63, 0, 17]) == [records[63], records[0], records[17]]
    more = seekable.append_records(rstream, records[:64][::-1], level=3, match_finder="none")
    _libzstd_frame_by_frame(ref, more, records + records[::-1])
    assert seekable.decompress_records(more, [64, 127, 5]) == [records[63], records[0], records[5]]
    assert more == seekable.edit(rstream, [(0, i) for i in range(64)] + [(1, j) for j in range(64)], records[::-1], level=3, match_finder="none")


def test_typed_bf16_stream(zstd, ref):
    """1 MiB of bf16 N(0, 0.02), element_size 2, groups of 131 072 elements: the elements come back, every plane frame is libzstd's literals-only frame of that plane,
    and the stream is smaller than the default finder's"""
    from zstandard_amd.device import SeekableStream
    data = ns.bf16_bytes(524288)
    src = np.frombuffer(data, dtype=np.uint8)
    planes = pm.planes(src, 2, 131072)
    assert len(planes) == 8 and all(len(p) == 131072 for p in planes)
    ctx = _ctx()
    try:
        out = ctx.seekable_compress(_dev(data), frame_size=131072, element_size=2)
        raw = out.cpu().numpy().tobytes()
        with SeekableStream(ctx, out) as st:
            assert st.element_size == 2 and st.n_frames == 9
            assert st.read().cpu().numpy().tobytes() == data
            assert st.read(2 * 131072 - 6, 4000).cpu().numpy().tobytes() == data[2 * 131072 - 6: 2 * 131072 - 6 + 4000]
            off = st.frame_offsets().tolist()
        assert off == np.cumsum([0] + [len(p) for p in planes] + [0]).tolist()                  # frame i holds plane i's bytes
        entries, _, _ = sc.parse(raw)
        at = none_total = 0
        for i, plane in enumerate(planes):
            want = _literals_only(ref, plane)
            assert entries[i][0] == len(want) and raw[at:at + len(want)] == want, "plane frame %d is not libzstd's literals-only frame" % i
            at += len(want); none_total += len(want)
        ctx.set_match_finder("libzstd")
        default = ctx.seekable_compress(_dev(data), frame_size=131072, element_size=2)
        print("typed bf16 MiB: %d bytes of plane frames without a search, the default finder's stream %d bytes" % (none_total, default.numel()))
        assert len(raw) < default.numel()
    finally:
        ctx.close()
