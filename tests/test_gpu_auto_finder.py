"""match_finder="auto" on the MI355X (DeviceBatchContext(match_finder="auto"): zhip_ctx_set_match_finder(ZHIP_FINDER_AUTO) -- zhip_encode_classify_kernel, the partition /
gather / scatter kernels of zhip_encode_auto.hpp, then the default finder's and the literals-only finder's kernels as they are). The choice bytes and statistics of
ctx.classify must equal the numpy model's (tests/auto_model.py); every frame must be libzstd 1.5.7's for the chosen mode -- ZSTD_compressSequences with the list that is
only the block delimiter, or ZSTD_compress2 --, with and without checksums, and decode back. Launch counts, launch shapes, a typed stream, a context that alternates all
four finders, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from tests import auto_model as am
from tests import delta_model as dm
from tests import planes_model as pm
from tests import reflib
from tests import seekable_cases as sc

pytestmark = pytest.mark.gpu
CANARY = 64
CLASSIFY_TIMER, SEARCH_TIMERS, NONE_TIMER = 12, (5, 6, 8), 11
CHUNK = 65536                                       # ze_auto_plan (tests/test_emu_auto_finder.py::test_plan holds it)


@pytest.fixture(scope="module")
def zstd():
    import zstandard_amd
    import zstandard_amd.device  # noqa: F401
    import zstandard_amd.seekable  # noqa: F401
    lib = zstandard_amd._lib.lib()
    assert lib.zhip_device_count() >= 1, "no GPU visible"
    assert lib.zhip_kernel_name(CLASSIFY_TIMER) == b"zhip_encode_classify_kernel" and lib.zhip_kernel_name(13) == b""
    assert lib.zhip_abi_version() == 3 and zstandard_amd.device.DeviceBatchContext.MATCH_FINDERS["auto"] == 4
    return zstandard_amd


@pytest.fixture(scope="module")
def ref():
    return reflib.checker()


@pytest.fixture(scope="module")
def sets():
    """frames of the six sets of DESIGN.md 4.2's table: {name: [bytes]}"""
    return dict(am.data_sets(1))


@pytest.fixture(scope="module")
def mixed(sets):
    """96 sources from the sets at 4 096 ... 131 072 bytes, with the model's (choice, statistics) of each: [(name, bytes, choice, stats)]"""
    lens = [4096, 5000, am.ALL, am.ALL + 1, 20000, 65536, 100001, am.BLOCK_MAX]
    out = []
    for name, frames in sets.items():
        for j in range(16):
            f = frames[(j * 5) % len(frames)]
            n = lens[(j + len(out)) % len(lens)]
            raw = f[(j * 977) % (len(f) - n + 1):][:n]
            out.append(("%s %d/%d" % (name, j, n), raw) + am.classify(raw))
    assert len(out) == 96 and 20 < sum(ch for _, _, ch, _ in out) < 76
    return out


def _flags(checksum):
    return reflib.F_CONTENTSIZE | reflib.F_DICTID | (reflib.F_CHECKSUM if checksum else 0)


def _libzstd(ref, raw, choice, level=3, checksum=False):
    if choice == am.LITERALS:
        return ref.compress_sequences(raw, [], len(raw), level=level, flags=_flags(checksum))
    return ref.compress(raw, level=level, flags=_flags(checksum))


def _batch(raws, caps=None):
    """sources packed back to back in an allocation of exactly their size (the last one ends at its end); destination slots of zhip_compress_bound bytes (or caps[i])
    between canaries"""
    import torch
    from zstandard_amd import _lib
    dev = torch.device("cuda", 0)
    n = len(raws)
    lens = np.array([len(r) for r in raws], dtype=np.int64)
    offs = np.zeros(n, dtype=np.int64); offs[1:] = np.cumsum(lens)[:-1]
    bound_of = {x: int(_lib.lib().zhip_compress_bound(int(x))) for x in set(lens.tolist())}
    bounds = np.array([bound_of[x] if caps is None or caps[i] is None else caps[i] for i, x in enumerate(lens.tolist())], dtype=np.int64)
    doffs = CANARY + np.concatenate([[0], np.cumsum(bounds + CANARY)[:-1]]).astype(np.int64)

    def segs(o, l):
        a = np.zeros((n, 2), dtype=np.int64); a[:, 0] = o; a[:, 1] = l
        return torch.from_numpy(a).to(dev)

    joined = b"".join(raws)
    src = torch.from_numpy(np.frombuffer(joined, dtype=np.uint8).copy()).to(dev) if joined else torch.zeros(1, dtype=torch.uint8, device=dev)
    return src, segs(offs, lens), doffs, bounds, segs(doffs, bounds)


def _run(ctx, raws, caps=None):
    """(frames, statuses, what zhip_ctx_sync reports or None)"""
    import torch
    from zstandard_amd import _lib
    n = len(raws)
    src, ssegs, doffs, bounds, dsegs = _batch(raws, caps)
    dst = torch.full((int(doffs[-1] + bounds[-1] + CANARY),), 0xC5, dtype=torch.uint8, device=src.device)
    out_sizes = torch.zeros(n, dtype=torch.int64, device=src.device)
    status = torch.full((n,), -1, dtype=torch.int32, device=src.device)
    ctx.compress(src, ssegs, dst, dsegs, out_sizes, status)
    err = _lib.Error()
    rc = ctx.L.zhip_ctx_sync(ctx.ctx, torch.cuda.current_stream().cuda_stream, status.data_ptr(), n, C.byref(err))
    st = status.cpu().numpy(); got = dst.cpu().numpy(); sz = out_sizes.cpu().numpy()
    canaries = np.concatenate([np.arange(CANARY), ((doffs + bounds)[:, None] + np.arange(CANARY)[None, :]).reshape(-1)])
    assert (got[canaries] == 0xC5).all(), "bytes outside the destination slots were written"
    assert ((0 <= sz) & (sz <= bounds)).all()
    return [got[doffs[i]: doffs[i] + sz[i]].tobytes() for i in range(n)], st.tolist(), (int(err.index), int(err.zstdErr)) if rc else None


def _classify(ctx, raws, stats=True):
    src, ssegs, _, _, _ = _batch(raws)
    choice, st = ctx.classify(src, ssegs, stats=True)
    return choice.cpu().numpy().tolist(), st.cpu().numpy().view(np.uint32).tolist()


def _ctx(finder="auto", **kw):
    from zstandard_amd.device import DeviceBatchContext
    return DeviceBatchContext(match_finder=finder, **kw)


def _launches(ctx):
    return {k: ctx.kernel_time(k)[1] for k in (CLASSIFY_TIMER, NONE_TIMER) + SEARCH_TIMERS}


def test_classify_equals_the_model(zstd, mixed):
    ctx = _ctx("libzstd")                                                       # (the entry point reads neither the finder nor the level)
    try:
        choice, stats = _classify(ctx, [r for _, r, _, _ in mixed])
    finally:
        ctx.close()
    for (name, raw, ch, sv), got_ch, got_sv in zip(mixed, choice, stats):
        assert (got_ch, got_sv) == (ch, sv), (name, got_ch, got_sv, ch, sv)


@pytest.mark.parametrize("checksum", [False, True], ids=["plain", "checksum"])
def test_mixed_batch_frames_are_libzstds_for_the_chosen_mode(zstd, ref, mixed, checksum):
    raws = [r for _, r, _, _ in mixed]
    ctx = _ctx(write_checksum=checksum)
    try:
        ctx.kernel_time(CLASSIFY_TIMER)
        got, st, first = _run(ctx, raws)
        launches = _launches(ctx)
    finally:
        ctx.close()
    assert not any(st) and first is None, (st, first)
    assert launches[CLASSIFY_TIMER] == 1 and launches[NONE_TIMER] == 1 and launches[6] == 1, launches
    for (name, raw, ch, _), f in zip(mixed, got):
        assert f == _libzstd(ref, raw, ch, checksum=checksum), (name, ch)
    back = zstd.ZstdDecompressor().multi_decompress_to_buffer(got)
    assert [back[i].tobytes() for i in range(len(raws))] == raws


def test_batches_of_one_kind_launch_nothing_of_the_other(zstd, ref, sets):
    floats = [f[k * 1000:][:30000 + k] for k, f in enumerate(sets["bf16 planes"] + sets["fp32 planes"])]
    texts = [f[k * 1000:][:30000 + k] for k, f in enumerate(f for f in sets["text"] if am.classify(f[:40000])[0] == am.SEARCH)][:12]
    texts = [t for t in texts if am.classify(t)[0] == am.SEARCH]
    assert all(am.classify(f)[0] == am.LITERALS for f in floats) and len(texts) >= 6
    for raws, choice in ((floats, am.LITERALS), (texts, am.SEARCH)):
        ctx = _ctx()
        try:
            ctx.kernel_time(CLASSIFY_TIMER)
            got, st, first = _run(ctx, raws)
            launches = _launches(ctx)
        finally:
            ctx.close()
        assert not any(st) and got == [_libzstd(ref, r, choice) for r in raws]
        if choice == am.LITERALS:
            assert launches == {12: 1, 11: 1, 5: 0, 6: 0, 8: 0}, launches
        else:
            assert launches[12] == 1 and launches[11] == 0 and launches[6] == 1, launches


@pytest.mark.parametrize("shape", ["n=1", "n=65", "n=4097"])
def test_launch_shapes(zstd, ref, sets, shape):
    """n = 4 097 sources of 1 ... 2 KiB: a wave claims more than one source and the partition runs over five tiles; drawn from 61 distinct sources, so that the model and
    libzstd run once for each"""
    expo, text = sets["bf16 planes"][1], sets["text"][0]
    pool = [(expo if k % 3 else text)[k * 1700:][:1024 + (k * 97) % 1025] for k in range(61)]
    n = int(shape[2:])
    idx = [0] if n == 1 else [(i * 7) % 61 for i in range(n)]
    want = {k: am.classify(pool[k]) for k in set(idx)}
    frames = {k: _libzstd(ref, pool[k], want[k][0]) for k in set(idx)}
    raws = [pool[k] for k in idx]
    ctx = _ctx()
    try:
        ctx.kernel_time(CLASSIFY_TIMER)
        got, st, first = _run(ctx, raws)
        launches = _launches(ctx)
        choice, stats = _classify(ctx, raws)
    finally:
        ctx.close()
    assert not any(st) and first is None
    assert launches[CLASSIFY_TIMER] == (n + CHUNK - 1) // CHUNK
    assert choice == [want[k][0] for k in idx] and stats == [want[k][1] for k in idx]
    assert got == [frames[k] for k in idx]
    if n > 1:
        assert 0 < sum(choice) < n


def test_refused_sources_keep_their_own_index(zstd, ref, mixed):
    """destinations too small (status 70) scattered among served sources of both kinds: status, size and frame at the source's own index, zhip_ctx_sync the lowest"""
    raws = [r for _, r, _, _ in mixed][:40]
    choice = [ch for _, _, ch, _ in mixed][:40]
    small = (3, 4, 21, 39)
    assert {choice[i] for i in small} == {0, 1}
    caps = [8 if i in small else None for i in range(40)]
    ctx = _ctx()
    try:
        got, st, first = _run(ctx, raws, caps)
    finally:
        ctx.close()
    assert st == [70 if i in small else 0 for i in range(40)] and first == (3, 70), (st, first)
    for i, raw in enumerate(raws):
        assert got[i] == (b"" if i in small else _libzstd(ref, raw, choice[i])), i


@pytest.mark.parametrize("filt", [None, "delta"])
def test_typed_stream_of_int64_sums(zstd, ref, filt):
    """2 groups of 4 096 elements and a short last one: every plane frame is libzstd's for the model's choice of that plane, the readers return the elements, libzstd
    decodes the whole stream"""
    frame, k = 4096, 8
    src = am.sums_values(1, 2 * frame + 1000).view(np.uint8)
    data = src.tobytes()
    planes = (dm if filt else pm).planes(src, k, frame)
    choice = [am.classify(p)[0] for p in planes]
    assert len(planes) == 24 and 0 < sum(choice) < 24
    stream = zstd.seekable.compress(data, frame_size=frame, element_size=k, filter=filt, match_finder="auto")
    entries, _, _ = sc.parse(stream)
    at = 0
    for i, ((c, d, _), p) in enumerate(zip(entries[:-1], planes)):
        assert stream[at:at + c] == _libzstd(ref, p, choice[i]), "plane frame %d is not libzstd's for choice %d" % (i, choice[i])
        assert ref.decompress(stream[at:at + c], d) == p
        at += c
    assert stream[at:at + 24] == (dm.marker(k, frame) if filt else pm.marker(k, frame))
    assert zstd.seekable.decompress(stream) == data
    assert zstd.seekable.decompress(stream, 8 * frame - 3, 100) == data[8 * frame - 3:8 * frame + 97]
    ctx = _ctx()
    try:
        import torch
        dev = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
        with zstd.device.SeekableStream(ctx, dev) as st:
            assert st.element_size == k and st.read().cpu().numpy().tobytes() == data
    finally:
        ctx.close()


def test_records_stream(zstd, ref, mixed):
    records = [r[:9000] for _, r, _, _ in mixed[::4]]
    stream = zstd.seekable.compress_records(records, level=3, match_finder="auto")
    entries, _, _ = sc.parse(stream)
    at = 0
    for (c, d, _), r in zip(entries, records):
        assert stream[at:at + c] == _libzstd(ref, r, am.classify(r)[0]); at += c
    assert zstd.seekable.decompress_records(stream, [23, 0]) == [records[23], records[0]]


def test_one_context_alternating_finders(zstd, ref, mixed):
    raws = [r for _, r, _, _ in mixed[1::3]]
    fresh = {}
    for finder in ("libzstd", "auto", "none", "wave"):
        ctx = _ctx(finder)
        try:
            fresh[finder], st, first = _run(ctx, raws)
            assert not any(st) and first is None, finder
        finally:
            ctx.close()
    assert fresh["auto"] != fresh["libzstd"] and fresh["auto"] != fresh["none"]
    ctx = _ctx("libzstd")
    try:
        for finder in ("libzstd", "auto", "none", "wave", "auto"):
            ctx.set_match_finder(finder)
            got, st, first = _run(ctx, raws)
            assert not any(st) and first is None, finder
            assert got == fresh[finder], "after a switch to %r the context writes other frames than a fresh one" % finder
    finally:
        ctx.close()


def test_refusals(zstd, sets):
    text = sets["text"][0]
    for kw in (dict(level=3, dict_data=text[:4000]), dict(level=5)):
        ctx = _ctx(**kw)
        try:
            with pytest.raises(zstd.ZstdError, match="auto"):
                _run(ctx, [text[:40000]])
        finally:
            ctx.close()
    ctx = _ctx()
    try:
        assert ctx.L.zhip_ctx_set_match_finder(ctx.ctx, 3) != 0 and ctx.match_finder == "auto"      # value 3 stays refused
        src, ssegs, _, _, _ = _batch([text[:3000]])
        ctx.kernel_time(CLASSIFY_TIMER)
        assert ctx.L.zhip_classify_batch_device(ctx.ctx, src.data_ptr(), ssegs.data_ptr(), 1, None, None, None) != 0      # a null choice pointer: an error ...
        assert ctx.kernel_time(CLASSIFY_TIMER)[1] == 0                                                                      # ... with nothing queued
    finally:
        ctx.close()
