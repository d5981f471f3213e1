"""The compress path at the launch shapes only a real GPU runs, and the device API's segment tables at their edges, every frame compared.

* the switch points of zhip_compress_batch_device: the LDS-source kernel up to numCU x 4 sources (no size hint), the placement pick from
  ZHIP_PICK_MIN = 16 384, the four-probe flat search up to 32 768, three probes up to 65 536, above that 131 072 sources per launch at two;
* BASELINE configs[4]: 131 072 x 128 KiB in one flat launch, all frames against libzstd, then decoded where they lie (two pipeline chunks);
* segment tables multi_*_to_buffer never builds -- odd offsets, gaps, shuffled order, shared sources, slots of exactly zhip_compress_bound and
  one byte short, decode capacities at and around the content size -- with canaries around every slot, both directions;
* zhip_compact_device and the host path's size scan against a NumPy restatement / libzstd, at the sizes and counts where their loops turn over.

Every comparison is frame by frame against libzstd 1.5.7 (tests/reflib.checker()) or byte by byte against NumPy; nothing is sampled."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 0xA5
ZE_DST_TOO_SMALL = 70


@pytest.fixture(scope="module")
def zstd():
    import zstandard_amd
    assert zstandard_amd._lib.lib().zhip_device_count() >= 1, "no GPU visible"
    return zstandard_amd


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _segs(offs, lens):
    a = np.zeros((len(offs), 2), dtype=np.int64)
    a[:, 0] = offs
    a[:, 1] = lens
    return _t(a)


def _bound(n):
    from zstandard_amd import _lib
    return int(_lib.lib().zhip_compress_bound(int(n)))


def _context(env=None, hint=0):
    """a fresh device context; `env` (the existing knobs only) is set just around its creation, where the library reads it, and restored"""
    from zstandard_amd.device import DeviceBatchContext
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = DeviceBatchContext()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if hint:
        ctx.set_size_hint(hint)
    return ctx


def _ref_frames(ref, raws, level=3):
    with ThreadPoolExecutor(16) as pool:                     # (ctypes drops the GIL; the checker keeps a context per thread)
        return list(pool.map(lambda r: ref.compress(r, level=level), raws))


def _odd_layout(rng, lens, order):
    """offsets of items of `lens` placed in the order `order`, each at an odd offset after a gap of 1 ... 40 bytes; returns (offsets, arena size)"""
    offs = np.zeros(len(lens), dtype=np.int64)
    pos = 0
    for i in order:
        pos += int(rng.integers(1, 41))
        pos |= 1
        offs[i] = pos
        pos += int(lens[i])
    return offs, pos + int(rng.integers(1, 41))


def _outside_slots_untouched(arena, offs, caps):
    """True when every byte of `arena` outside every [off, off + cap) still holds the canary"""
    mask = np.ones(len(arena), dtype=bool)
    for o, c in zip(offs, caps):
        mask[o:o + c] = False
    bad = np.nonzero(arena[mask] != CANARY)[0]
    return bad.size == 0, (np.nonzero(mask)[0][bad[:8]].tolist() if bad.size else [])


# ---------------------------------------------------------------------------------------------------------------- 1. launch-shape sweep

SWEEP_MAX = 65537


@pytest.fixture(scope="module")
def sweep_sources(corpus, ref):
    """SWEEP_MAX sources of 64 B ... 4 KiB cut from the corpus, every 4 099th one (and the last) a whole block, every 1 031st empty;
    packed back to back (odd offsets follow). The first n of them are the batch of n."""
    rng = np.random.default_rng(4242)
    pool = np.frombuffer(b"".join(corpus.frame_bytes(2000 + i) for i in range(48)), dtype=np.uint8)
    lens = rng.integers(64, 4097, SWEEP_MAX).astype(np.int64)
    lens[::4099] = 131072
    lens[-1] = 131072
    lens[5::1031] = 0
    starts = rng.integers(0, len(pool) - 131072, SWEEP_MAX)
    offs = np.zeros(SWEEP_MAX, dtype=np.int64)
    offs[1:] = np.cumsum(lens)[:-1]
    arena = np.concatenate([pool[s:s + n] for s, n in zip(starts, lens)])
    raws = [arena[o:o + n].tobytes() for o, n in zip(offs, lens)]
    return arena, offs, lens, _ref_frames(ref, raws)


SWEEP_SIZES = ["L", "L+1", 16383, 16384, 32768, 32769, 65536, 65537]


def _sweep_size(name):
    import torch
    L = torch.cuda.get_device_properties(0).multi_processor_count * 4      # the LDS-source kernel's limit without a size hint (ZHIP_E1LDS_PER_CU)
    return {"L": L, "L+1": L + 1}.get(name, name)


@pytest.mark.parametrize("size", SWEEP_SIZES, ids=[str(x) for x in SWEEP_SIZES])
def test_compress_launch_shape_sweep(zstd, sweep_sources, size):
    """Level 3 through DeviceBatchContext.compress at both sides of every switch point, each size in a fresh context (its own first launch and
    placement pick), slots of exactly zhip_compress_bound back to back. What each size must show (zhip_compress_batch_device): ONE launch of the
    match stage -- timer 8 brackets the LDS-source kernel and the flat kernels alike, the pick's probe launches are timed apart and not counted --,
    one of the lane-serial match and the entropy kernels, none of the generic kernel's own path (timer 1); a placement pick from 16 384 sources on
    and not below; 65 537 sources as one launch (the 131 072-per-launch regime). Every frame libzstd's."""
    import torch
    n = _sweep_size(size)
    arena, offs, lens, want = sweep_sources
    dev = _dev()
    bounds = np.array([_bound(x) for x in lens[:n]], dtype=np.int64)
    doffs = np.zeros(n, dtype=np.int64)
    doffs[1:] = np.cumsum(bounds)[:-1]
    total = int(bounds.sum())
    src = _t(arena[: int(offs[n - 1] + lens[n - 1])])
    dst = torch.full((total,), CANARY, dtype=torch.uint8, device=dev)
    out_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    free_before = torch.cuda.mem_get_info()
    ctx = _context()
    try:
        ctx.kernel_time(8)                                           # switches the timers on (and zeroes them)
        ctx.compress(src, _segs(offs[:n], lens[:n]), dst, _segs(doffs, bounds), out_sizes, status)
        torch.cuda.synchronize()
        t = {k: ctx.kernel_time(k)[1] for k in (1, 5, 6, 8)}
        pick_ms, _ = ctx.table_pick()
    finally:
        ctx.close()
    st = status.cpu().numpy()
    sz = out_sizes.cpu().numpy()
    got = dst.cpu().numpy()
    del src, dst
    torch.cuda.empty_cache()
    assert t[8] == 1, ("match-stage launches", n, t, "free / total device memory before the call: %s" % (free_before,))
    assert t[5] == 1 and t[6] == 1 and t[1] == 0, (n, t)
    assert (pick_ms[0] > 0) == (n >= 16384), (n, pick_ms)
    assert not st.any(), (n, np.nonzero(st)[0][:8], st[np.nonzero(st)[0][:8]])
    bad = [i for i in range(n) if got[doffs[i]: doffs[i] + sz[i]].tobytes() != want[i]]
    assert not bad, (n, len(bad), bad[:8], [int(lens[i]) for i in bad[:8]])


# ---------------------------------------------------------------------------------------------------------------- 2. configs[4], every frame

def test_131072_sources_of_128k_one_launch_every_frame(ref, monkeypatch):
    """BASELINE configs[4]'s shape (bench.bench_roundtrip): 131 072 x 128 KiB through one context -- one flat launch of 131 072 sources, tables
    of ~96 GiB, source indices past 65 536 included --, all 131 072 frames against libzstd's (host threads, slices of 16 384 rows), then the
    frames decoded where they lie in their slots (two decode-pipeline chunks of 65 536) and every byte compared in HBM."""
    import torch
    import bench
    from tests.corpus import Corpus
    monkeypatch.setattr(bench, "HOST_THREADS", min(bench.HOST_THREADS, 16))
    F, item = 131072, 131072
    dev = _dev()
    raw = Corpus(device=dev, mix="silesia").frames(0, F, chunk=256)
    bound = _bound(item)
    src_segs = _segs(np.arange(F, dtype=np.int64) * item, np.full(F, item, dtype=np.int64))
    slot_segs = _segs(np.arange(F, dtype=np.int64) * bound, np.full(F, bound, dtype=np.int64))
    slots = torch.zeros(F * bound, dtype=torch.uint8, device=dev)
    csz = torch.zeros(F, dtype=torch.int64, device=dev)
    st = torch.full((F,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()
    ctx = _context()
    try:
        ctx.kernel_time(8)
        ctx.compress(raw.reshape(-1), src_segs, slots, slot_segs, csz, st)
        torch.cuda.synchronize()
        launches = ctx.kernel_time(8)[1]
    finally:
        ctx.close()
    torch.cuda.empty_cache()
    assert launches == 1, ("flat launches", launches, "free / total device memory before the call: %s" % (free_before,))
    assert int(st.abs().max().item()) == 0, "a frame failed to compress"
    sizes = csz.cpu().numpy()
    slots_v = slots.view(F, bound)
    for lo in range(0, F, 16384):
        hi = lo + 16384
        want, wsz = bench.compress_on_host(raw[lo:hi].cpu().numpy(), item)
        assert np.array_equal(wsz, sizes[lo:hi]), ("frame sizes differ from libzstd's", lo, np.nonzero(wsz != sizes[lo:hi])[0][:8])
        got = slots_v[lo:hi].cpu().numpy()
        bad = [lo + j for j in range(hi - lo) if got[j, : wsz[j]].tobytes() != want[j]]
        assert not bad, ("frames differ from libzstd 1.5.7", len(bad), bad[:8])
        del want, got
    # decode the frames in place: their slots are the sources, the originals' layout the destination
    frame_segs = torch.stack([slot_segs[:, 0], csz], dim=1).contiguous()
    back = torch.full((F * item,), CANARY, dtype=torch.uint8, device=dev)
    bsz = torch.zeros(F, dtype=torch.int64, device=dev)
    st2 = torch.full((F,), -1, dtype=torch.int32, device=dev)
    dctx = _context()
    try:
        dctx.decompress(slots, frame_segs, back, src_segs, bsz, st2)
        torch.cuda.synchronize()
    finally:
        dctx.close()
    assert int(st2.abs().max().item()) == 0 and bool((bsz == item).all().item()), "a frame failed to decode"
    assert torch.equal(back.view(F, item), raw), "round trip differs"
    del raw, slots, back, slots_v, frame_segs, src_segs, slot_segs
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- 3. segment tables, canaries

def _several_blocks(corpus, n, k):
    return b"".join(corpus.frame_bytes(3000 + k + j) for j in range(n // 131072 + 1))[:n]


@pytest.fixture(scope="module")
def compress_table(corpus, ref):
    """distinct sources (one-block ones of 0 ... 131 072 bytes, incompressible and run-length ones, sources of several blocks) and the items
    over them: each source once at exactly zhip_compress_bound, one source three times, and slots of bound - 1 for an empty, a one-block and a
    several-block source"""
    rng = np.random.default_rng(31)
    srcs = [b"", b"", corpus.frame_bytes(3100)[:10], corpus.frame_bytes(3101)[:63], corpus.frame_bytes(3102)[:64], corpus.frame_bytes(3103)[:100],
            corpus.frame_bytes(3104)[:1000], corpus.frame_bytes(3105)[:4096], corpus.frame_bytes(3106)[:30000], corpus.frame_bytes(3107)[:65537],
            corpus.frame_bytes(3108)[:131071], corpus.frame_bytes(3109), rng.bytes(20000), bytes(rng.integers(0, 2, 50000, dtype=np.uint8)),
            _several_blocks(corpus, 200000, 0), _several_blocks(corpus, 300001, 10)]
    items, short = [], []
    for s in range(len(srcs)):
        items.append(s)
    items += [8, 8]                                                                 # source 8 serves three items
    for s in (0, 7, 15):                                                            # empty, one block, several blocks: one byte short
        short.append(len(items))
        items.append(s)
    order = rng.permutation(len(items))                                              # the items in shuffled order of their sources' use
    items = [items[i] for i in order]
    short = [int(np.nonzero(order == j)[0][0]) for j in short]
    return srcs, items, short, _ref_frames(ref, srcs)


@pytest.mark.parametrize("arrangement", ["lds", "flat", "several_blocks"])
def test_compress_segment_tables_with_canaries(zstd, compress_table, arrangement):
    """Sources in shuffled order at odd offsets with gaps, one source used by three items, empty sources, destination slots of exactly
    zhip_compress_bound at odd offsets with gaps and in yet another order, three of bound - 1 (an empty, a one-block and a several-block source).
    Through the LDS-source kernel (a small batch), the flat search (ZHIP_E1LDS_MAX=0) and the several-block flat search (ZHIP_MBC_MIN=0 + a size
    hint). Every status-0 frame is libzstd's; every short slot is refused with status 70 (include/zstd_hip.h: the rule of every kernel); no byte
    outside any slot changes."""
    import torch
    srcs, items, short, want = compress_table
    rng = np.random.default_rng(["lds", "flat", "several_blocks"].index(arrangement) + 7)
    n = len(items)
    slens = np.array([len(s) for s in srcs], dtype=np.int64)
    soffs, sarena = _odd_layout(rng, slens, rng.permutation(len(srcs)))
    src_np = np.full(sarena, 0x3C, dtype=np.uint8)
    for s, o in zip(srcs, soffs):
        src_np[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    caps = np.array([_bound(len(srcs[s])) for s in items], dtype=np.int64)
    caps[short] -= 1
    doffs, darena = _odd_layout(rng, caps, rng.permutation(n))
    dev = _dev()
    dst = torch.full((darena,), CANARY, dtype=torch.uint8, device=dev)
    out_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    env = {"lds": {}, "flat": {"ZHIP_E1LDS_MAX": "0"}, "several_blocks": {"ZHIP_MBC_MIN": "0"}}[arrangement]
    ctx = _context(env, hint=max(slens) if arrangement == "several_blocks" else 0)
    try:
        ctx.compress(_t(src_np), _segs(soffs[items], slens[items]), dst, _segs(doffs, caps), out_sizes, status)
        torch.cuda.synchronize()
    finally:
        ctx.close()
    st, sz, got = status.cpu().numpy(), out_sizes.cpu().numpy(), dst.cpu().numpy()
    for i, s in enumerate(items):
        if i in short:
            assert st[i] == ZE_DST_TOO_SMALL, (arrangement, "slot of bound - 1", i, len(srcs[s]), int(st[i]))
        else:
            assert st[i] == 0, (arrangement, i, len(srcs[s]), int(st[i]))
            assert got[doffs[i]: doffs[i] + sz[i]].tobytes() == want[s], (arrangement, i, len(srcs[s]))
    ok, where = _outside_slots_untouched(got, doffs, caps)
    assert ok, (arrangement, "bytes outside the slots changed at", where)


@pytest.fixture(scope="module")
def decompress_table(corpus, ref):
    """libzstd frames (empty, one-block of 1 ... 131 072 bytes, a raw block, run-length content, several blocks) and items over them:
    capacities of the content size + 0, 1, 2, 15, 16, 17, 31 and 63 bytes, one byte short, and the empty frame into a slot of capacity 0"""
    rng = np.random.default_rng(57)
    raws = [b"", corpus.frame_bytes(3200)[:1], corpus.frame_bytes(3201)[:100], corpus.frame_bytes(3202)[:4096], corpus.frame_bytes(3203)[:65536],
            corpus.frame_bytes(3204), rng.bytes(20000), bytes(rng.integers(0, 2, 50000, dtype=np.uint8)) * 2,
            _several_blocks(corpus, 200000, 20), _several_blocks(corpus, 300001, 30)]
    frames = [ref.compress(r) for r in raws]
    items, caps = [], []
    for f, r in enumerate(raws):
        for extra in (0, 1, 2, 15, 16, 17, 31, 63) + ((-1,) if r else ()):
            items.append(f)
            caps.append(len(r) + extra)
    order = rng.permutation(len(items))
    items = [items[i] for i in order]
    caps = np.array([caps[i] for i in order], dtype=np.int64)
    expect = []
    for f, c in zip(items, caps):
        try:
            expect.append(ref.decompress(frames[f], int(c)))
        except RuntimeError:
            expect.append(None)                                     # libzstd cannot produce the whole frame in that capacity
    return raws, frames, items, caps, expect


@pytest.mark.parametrize("arrangement", ["default", "k0_pipeline", "several_blocks"])
def test_decompress_segment_tables_with_canaries(zstd, decompress_table, arrangement):
    """Frames in shuffled order at odd offsets with gaps, each shared by several items; destination slots in another shuffled order at odd
    offsets with gaps. Through the default context (the pipeline, the generic kernel for frames of several blocks), the pipeline with K0 on
    every batch (ZHIP_K0_MIN=0) and the several-block mode (size hint above 128 KiB). Status 0 exactly where libzstd produces the whole frame in
    that capacity, and then its bytes; no byte outside any slot changes."""
    import torch
    raws, frames, items, caps, expect = decompress_table
    rng = np.random.default_rng(["default", "k0_pipeline", "several_blocks"].index(arrangement) + 70)
    n = len(items)
    flens = np.array([len(f) for f in frames], dtype=np.int64)
    foffs, farena = _odd_layout(rng, flens, rng.permutation(len(frames)))
    src_np = np.full(farena, 0x3C, dtype=np.uint8)
    for f, o in zip(frames, foffs):
        src_np[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    doffs, darena = _odd_layout(rng, caps, rng.permutation(n))
    dev = _dev()
    dst = torch.full((darena,), CANARY, dtype=torch.uint8, device=dev)
    out_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    env = {"default": {}, "k0_pipeline": {"ZHIP_K0_MIN": "0"}, "several_blocks": {}}[arrangement]
    ctx = _context(env, hint=max(len(r) for r in raws) if arrangement == "several_blocks" else 0)
    try:
        ctx.decompress(_t(src_np), _segs(foffs[items], flens[items]), dst, _segs(doffs, caps), out_sizes, status)
        torch.cuda.synchronize()
    finally:
        ctx.close()
    st, sz, got = status.cpu().numpy(), out_sizes.cpu().numpy(), dst.cpu().numpy()
    for i, f in enumerate(items):
        if expect[i] is None:
            assert st[i] != 0, (arrangement, "accepted where libzstd cannot finish", i, len(raws[f]), int(caps[i]))
        else:
            assert st[i] == 0, (arrangement, i, len(raws[f]), int(caps[i]), int(st[i]))
            assert sz[i] == len(expect[i]) and got[doffs[i]: doffs[i] + sz[i]].tobytes() == expect[i], (arrangement, i, len(raws[f]), int(caps[i]))
    ok, where = _outside_slots_untouched(got, doffs, caps)
    assert ok, (arrangement, "bytes outside the slots changed at", where)


# ---------------------------------------------------------------------------------------------------------------- 4. compaction and the scan

def _compact_numpy(slots, slot_offs, sizes, status, offs, dense):
    out = dense.copy()
    for i in range(len(sizes)):
        if status[i] == 0:
            out[offs[i]: offs[i] + sizes[i]] = slots[slot_offs[i]: slot_offs[i] + sizes[i]]
    return out


@pytest.mark.parametrize("n", [1, 5000, 70000])
def test_compact_device_against_numpy(zstd, n):
    """zhip_compact_device called directly: slots at odd offsets in shuffled order, sizes of 0, 1, 15, 16, 17, 1 023, 1 024, 1 025, ~128 KiB and
    ~1 MiB, non-zero status on scattered items, dense offsets that leave gaps and keep room at the targets of skipped items. n = 5 000 and 70 000
    turn the grid-stride loop over past numCU x 16 workgroups. The dense arena must equal the NumPy restatement byte for byte: the copies in place,
    the canaries in the gaps and at the skipped items' targets intact."""
    import torch
    rng = np.random.default_rng(n)
    small = np.array([0, 1, 15, 16, 17, 1023, 1024, 1025], dtype=np.int64)
    sizes = small[rng.integers(0, len(small), n)]
    big = rng.choice(n, size=min(n, 8), replace=False)
    sizes[big[::2]] = 131072 + 5
    sizes[big[1::2]] = (1 << 20) + 3
    status = np.where(rng.random(n) < 0.07, rng.choice([70, 11, -1], n), 0).astype(np.int32)
    if n == 1:
        sizes[0], status[0] = (1 << 20) + 3, 0
    else:
        status[big[0]] = 70                                          # a skipped item of ~128 KiB: its target must stay untouched
    caps = sizes + rng.integers(0, 48, n)
    slot_offs, sarena = _odd_layout(rng, caps, rng.permutation(n))
    slots = rng.integers(0, 256, sarena, dtype=np.uint8)
    gaps = rng.integers(0, 10, n)
    offs = np.cumsum(sizes + gaps) - sizes                             # skipped items keep their room: a canary there must survive
    dense = np.full(int(offs[-1] + sizes[-1] + 64), CANARY, dtype=np.uint8)
    want = _compact_numpy(slots, slot_offs, sizes, status, offs, dense)
    d_dense = _t(dense)
    d_slots, d_segs, d_sizes, d_status, d_offs = _t(slots), _segs(slot_offs, caps), _t(sizes), _t(status), _t(offs.astype(np.int64))
    rc = zstd._lib.lib().zhip_compact_device(d_slots.data_ptr(), d_segs.data_ptr(), d_sizes.data_ptr(), d_status.data_ptr(), d_offs.data_ptr(), n,
                                             d_dense.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    got = d_dense.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (n, bad.size, bad[:8].tolist())


def test_sharded_compact_over_device_compress_output(zstd, corpus, ref):
    """sharded._compact with the library's real compactor over what DeviceBatchContext.compress wrote (slots of zhip_compress_bound at odd
    offsets, two of them one byte short: status 70, no bytes): the dense payload holds every status-0 frame, libzstd's, at its dense segment."""
    import torch
    from zstandard_amd import sharded
    rng = np.random.default_rng(99)
    raws = [corpus.frame_bytes(3300 + i % 40)[: int(rng.integers(0, 131073))] for i in range(300)]
    want = _ref_frames(ref, raws)
    n = len(raws)
    lens = np.array([len(r) for r in raws], dtype=np.int64)
    soffs, sarena = _odd_layout(rng, lens, np.arange(n))
    src_np = np.zeros(sarena, dtype=np.uint8)
    for r, o in zip(raws, soffs):
        src_np[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
    caps = np.array([_bound(x) for x in lens], dtype=np.int64)
    caps[[17, 200]] -= 1
    doffs, darena = _odd_layout(rng, caps, rng.permutation(n))
    dev = _dev()
    slots = torch.full((darena,), CANARY, dtype=torch.uint8, device=dev)
    slot_segs = _segs(doffs, caps)
    csz = torch.zeros(n, dtype=torch.int64, device=dev)
    st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ctx = _context()
    try:
        ctx.compress(_t(src_np), _segs(soffs, lens), slots, slot_segs, csz, st)
        torch.cuda.synchronize()
    finally:
        ctx.close()
    dense, dsegs = sharded._compact(slots, slot_segs, csz, st, dev)
    torch.cuda.synchronize()
    stn, dn, ds = st.cpu().numpy(), dense.cpu().numpy(), dsegs.cpu().numpy()
    assert stn[17] == ZE_DST_TOO_SMALL and stn[200] == ZE_DST_TOO_SMALL
    for i in range(n):
        if i in (17, 200):
            assert ds[i, 1] == 0
            continue
        assert stn[i] == 0, (i, int(stn[i]))
        assert dn[ds[i, 0]: ds[i, 0] + ds[i, 1]].tobytes() == want[i], i
    assert int(ds[:, 1].sum()) == sum(len(want[i]) for i in range(n) if i not in (17, 200))


@pytest.mark.parametrize("count", [1, 1023, 1024, 1025, 32768, 32769])
def test_host_api_scan_chunk_sizes(zstd, corpus, ref, count):
    """multi_compress_to_buffer's chunks go through zhip_scan_sizes_kernel (one workgroup of 1 024 threads, ceil(n / 1 024) items each) and the
    compaction: counts at both sides of 1 024 and of the 32 768-item chunk (32 769: a second chunk of one item). Every frame libzstd's."""
    rng = np.random.default_rng(count)
    pool = b"".join(corpus.frame_bytes(3400 + i) for i in range(4))
    starts = rng.integers(0, len(pool) - 300, count)
    lens = rng.integers(0, 300, count)
    raws = [pool[s:s + k] for s, k in zip(starts, lens)]
    res = zstd.ZstdCompressor(level=3).multi_compress_to_buffer(raws)
    assert len(res) == count
    want = _ref_frames(ref, raws)
    bad = [i for i in range(count) if res[i].tobytes() != want[i]]
    assert not bad, (count, len(bad), bad[:8])
