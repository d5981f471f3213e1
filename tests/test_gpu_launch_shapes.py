"""Both directions at the launch shapes only a real GPU runs, and the device API's segment tables at their edges, every frame compared.

* the switch points of zhip_compress_batch_device: the LDS-source kernel up to numCU x 4 sources (no size hint), the placement pick from
  ZHIP_PICK_MIN = 16 384, the four-probe flat search up to 32 768, three probes up to 65 536, above that 131 072 sources per launch at two;
* BASELINE configs[4]: 131 072 x 128 KiB in one flat launch, all frames against libzstd, then decoded where they lie (two pipeline chunks);
* segment tables multi_*_to_buffer never builds -- odd offsets, gaps, shuffled order, shared sources, slots of exactly zhip_compress_bound and
  one byte short, decode capacities at and around the content size -- with canaries around every slot, both directions;
* zhip_compact_device and the host path's size scan against a NumPy restatement / libzstd, at the sizes and counts where their loops turn over;
* the switch points of zhip_decompress_batch_device, which only the device API reaches (the host-buffer API hands the pipeline at most 32 768
  items a call, one chunk): chunks in series on one slot stream with K1b on the side stream, three slot streams for small frames and their
  reuse, the bin kernel's grid at 4 096 items, K0 from 6 144 frames per chunk, the several-block mode over two chunks, the fallback list filled
  from chunks past the first, a compact arena running out in a later chunk, one context through a sequence of calls.

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


COMPRESS_ARRANGEMENTS = ["lds", "flat", "several_blocks"]


def _compress_table_layout(table, rng):
    """where the compress table lies for one call: sources in shuffled order at odd offsets with gaps in an arena of 0x3C, destination slots of
    zhip_compress_bound (the short ones one byte less) at odd offsets with gaps in yet another order. Returns (source arena, the items' source
    offsets, the items' source lengths, slot offsets, slot capacities, destination arena size)."""
    srcs, items, short, _ = table
    slens = np.array([len(s) for s in srcs], dtype=np.int64)
    soffs, sarena = _odd_layout(rng, slens, rng.permutation(len(srcs)))
    src_np = np.full(sarena, 0x3C, dtype=np.uint8)
    for s, o in zip(srcs, soffs):
        src_np[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    caps = np.array([_bound(len(srcs[s])) for s in items], dtype=np.int64)
    caps[short] -= 1
    doffs, darena = _odd_layout(rng, caps, rng.permutation(len(items)))
    return src_np, soffs[items], slens[items], doffs, caps, darena


def _compress_table_context(table, arrangement):
    """a fresh context that serves the table through the LDS-source kernel (a small batch), the flat search (ZHIP_E1LDS_MAX=0) or the
    several-block flat search (ZHIP_MBC_MIN=0 + a size hint)"""
    env = {"lds": {}, "flat": {"ZHIP_E1LDS_MAX": "0"}, "several_blocks": {"ZHIP_MBC_MIN": "0"}}[arrangement]
    return _context(env, hint=max(len(s) for s in table[0]) if arrangement == "several_blocks" else 0)


def _check_compress_table(label, table, st, sz, got, doffs, caps):
    """every status-0 frame is libzstd's; every short slot is refused with status 70; no byte outside any slot changed"""
    srcs, items, short, want = table
    for i, s in enumerate(items):
        if i in short:
            assert st[i] == ZE_DST_TOO_SMALL, (label, "slot of bound - 1", i, len(srcs[s]), int(st[i]))
        else:
            assert st[i] == 0, (label, i, len(srcs[s]), int(st[i]))
            assert got[doffs[i]: doffs[i] + sz[i]].tobytes() == want[s], (label, i, len(srcs[s]))
    ok, where = _outside_slots_untouched(got, doffs, caps)
    assert ok, (label, "bytes outside the slots changed at", where)


@pytest.mark.parametrize("arrangement", COMPRESS_ARRANGEMENTS)
def test_compress_segment_tables_with_canaries(zstd, compress_table, arrangement):
    """Sources in shuffled order at odd offsets with gaps, one source used by three items, empty sources, destination slots of exactly
    zhip_compress_bound at odd offsets with gaps and in yet another order, three of bound - 1 (an empty, a one-block and a several-block source).
    Through the LDS-source kernel (a small batch), the flat search (ZHIP_E1LDS_MAX=0) and the several-block flat search (ZHIP_MBC_MIN=0 + a size
    hint). Every status-0 frame is libzstd's; every short slot is refused with status 70 (include/zstd_hip.h: the rule of every kernel); no byte
    outside any slot changes."""
    import torch
    rng = np.random.default_rng(COMPRESS_ARRANGEMENTS.index(arrangement) + 7)
    n = len(compress_table[1])
    src_np, soffs, slens, doffs, caps, darena = _compress_table_layout(compress_table, rng)
    dev = _dev()
    dst = torch.full((darena,), CANARY, dtype=torch.uint8, device=dev)
    out_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ctx = _compress_table_context(compress_table, arrangement)
    try:
        ctx.compress(_t(src_np), _segs(soffs, slens), dst, _segs(doffs, caps), out_sizes, status)
        torch.cuda.synchronize()
    finally:
        ctx.close()
    _check_compress_table(arrangement, compress_table, status.cpu().numpy(), out_sizes.cpu().numpy(), dst.cpu().numpy(), doffs, caps)


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


# ---------------------------------------------------------------------------------------------------------------- 5. decode launch shapes

DEC_TIMERS = (0, 2, 3, 4, 7, 9)      # zhip_kernel_name: the generic kernel, K1, K2, K3, K1b, one chunk's pipeline from K1's start to K3's end
SIZE_SENTINEL = 0x5A5A5A5A5A5A5A5A   # out_sizes before a call: a frame no kernel answered keeps it (and status -1)
POOL = 12289                         # items in the decode pool: a prime, so a frame decoded from or into another chunk's index never meets its twin


def _answers(ref, frames, caps):
    """libzstd's bytes for every (frame, capacity), None where it refuses"""
    def one(k):
        try:
            return ref.decompress(frames[k], int(caps[k]))
        except RuntimeError:
            return None
    with ThreadPoolExecutor(16) as pool:
        return list(pool.map(one, range(len(frames))))


class _Pool:
    pass


@pytest.fixture(scope="module")
def decode_pool(corpus, ref):
    """POOL items, shuffled: libzstd frames of 0 ... 4 KiB at levels 1, 3 and 19 (corpus text; noise, which makes raw blocks; runs, which make
    RLE blocks), every 7th with a content checksum, and craft.py's hand-made, skippable and unusual frames -- each with its capacity (the
    content size) and libzstd's answer. Beside them: frames of two blocks, one of three, and two of 1 MiB (eight blocks, more than a frame's
    share of the several-block mode's slots), some of them checksummed."""
    from tests import craft, reflib
    rng = np.random.default_rng(POOL)
    text = b"".join(corpus.frame_list(4000, 24))
    cases = craft.edge_frames() + craft.skippable_frames() + craft.encoding_variants()
    nl = POOL - len(cases)
    raws = []
    for k in range(nl):
        n = int(rng.integers(0, 4097))
        if k % 16 == 5:
            raws.append(rng.bytes(n))
        elif k % 16 == 11:
            raws.append(bytes([k & 255]) * n)
        else:
            s = int(rng.integers(0, len(text) - n))
            raws.append(text[s:s + n])

    def enc(r, level, checksum):
        return ref.compress(r, level=level, flags=reflib.DEFAULT_FLAGS | (reflib.F_CHECKSUM if checksum else 0))
    with ThreadPoolExecutor(16) as pool:
        frames = list(pool.map(lambda k: enc(raws[k], (1, 3, 19)[k % 3], k % 7 == 0), range(nl)))
    frames += [c[1] for c in cases]
    caps = [len(r) for r in raws] + [c[2] for c in cases]
    checked = [k % 7 == 0 and len(raws[k]) > 0 for k in range(nl)] + [False] * len(cases)
    order = rng.permutation(POOL)
    p = _Pool()
    p.frames = [frames[k] for k in order]
    p.caps = np.array([caps[k] for k in order], dtype=np.int64)
    p.want = _answers(ref, p.frames, p.caps)
    p.checked = [j for j, k in enumerate(order) if checked[k]]      # one-block frames with a content checksum: what a wrong checksum is made from
    # two blocks at level 3 (128 KiB + 1 ... 256 KiB), three (300 007 bytes), eight (1 MiB): (frame, content size, content)
    multi = [text[19 * 4096 * j: 19 * 4096 * j + n] for j, n in enumerate((131073, 150001, 200003, 262144, 300007))]
    p.multi = [(enc(r, 3, j % 2), len(r), r) for j, r in enumerate(multi)]
    p.mib = [(enc(r, 3, j), len(r), r) for j, r in enumerate((text[:1 << 20], text[2 << 20: 3 << 20]))]
    return p


def _damage(frame, rng, how):
    """a damaged copy: a bit flipped in the last four bytes (a frame's content checksum), the end cut off, or one to three bits flipped past the magic"""
    b = bytearray(frame)
    if how == 0:
        b[len(b) - 1 - int(rng.integers(0, 4))] ^= 1 << int(rng.integers(0, 8))
    elif how == 1:
        del b[max(1, len(b) - 1 - int(rng.integers(0, 48))):]
    else:
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(4, len(b)))] ^= 1 << int(rng.integers(0, 8))
    return bytes(b)


def _decode_batch(pool, ref, n, chunk, seed, several_block_mode=False):
    """n items: pool item i % POOL at index i, then -- per chunk of `chunk` frames -- the frames the pipeline must hand on or refuse. Without the
    several-block mode: frames of several blocks (K1 lists them for the generic kernel) at three places in every chunk; in it, a two-block frame
    at every 50th index and a 1 MiB frame at two places in every chunk. ~1 % damaged copies anywhere; a one-block frame with a wrong content
    checksum at index 5 of every chunk and at n - 2; at n - 1 a checksummed frame of several blocks (1 MiB in the several-block mode) with a
    wrong one. Returns (frames, capacities, libzstd's answers, which items are damaged copies)."""
    rng = np.random.default_rng(seed)
    reps = -(-n // POOL)
    frames = (pool.frames * reps)[:n]
    caps = np.tile(pool.caps, reps)[:n].copy()
    want = (pool.want * reps)[:n]
    damaged = np.zeros(n, dtype=bool)
    over = {}                                                        # index: (frame, capacity, content or None = ask libzstd, damaged)
    if several_block_mode:
        for i in range(25, n, 50):
            f, c, r = pool.multi[(i // 50) % 4]
            over[i] = (f, c, r, False)
    for first in range(0, n, chunk):
        cnt = min(chunk, n - first)
        places = (100, cnt // 2) if several_block_mode else (17, cnt // 2, cnt - 3)
        for j, at in enumerate(places):
            if 0 <= at < cnt:
                f, c, r = pool.mib[j] if several_block_mode else pool.multi[(first // chunk + j) % 5]
                over[first + at] = (f, c, r, False)
    for i in rng.choice(n, max(1, n // 100), replace=False):
        i, how = int(i), int(rng.integers(0, 3))
        if how == 0:
            k = pool.checked[int(rng.integers(0, len(pool.checked)))]
            f, c = pool.frames[k], pool.caps[k]
        else:
            f, c = over[i][:2] if i in over else (frames[i], caps[i])
        over[i] = (_damage(f, rng, how), int(c), None, True)
    for i in [first + 5 for first in range(0, n, chunk) if first + 5 < n] + [n - 2]:
        k = pool.checked[int(rng.integers(0, len(pool.checked)))]
        over[i] = (_damage(pool.frames[k], rng, 0), int(pool.caps[k]), None, True)
    f, c, _ = pool.mib[1] if several_block_mode else pool.multi[1]
    over[n - 1] = (_damage(f, rng, 0), c, None, True)
    ask = [i for i, v in over.items() if v[2] is None]
    told = dict(zip(ask, _answers(ref, [over[i][0] for i in ask], [over[i][1] for i in ask])))
    for i, (f, c, r, d) in over.items():
        frames[i], caps[i], damaged[i] = f, c, d
        want[i] = told[i] if r is None else r
    return frames, caps, want, damaged


def _decode_layout(batch, rng):
    """where `batch` lies for one call: frames at odd offsets with gaps in an arena of 0x3C, destination slots of the items' capacities at odd
    offsets with gaps in shuffled order. Returns (source arena, frame offsets, frame lengths, slot offsets, destination arena size)."""
    frames, caps, _, _ = batch
    n = len(frames)
    flens = np.fromiter((len(f) for f in frames), dtype=np.int64, count=n)
    soffs, sarena = _odd_layout(rng, flens, np.arange(n))
    src_np = np.full(sarena, 0x3C, dtype=np.uint8)
    for f, o in zip(frames, soffs):
        src_np[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    doffs, darena = _odd_layout(rng, caps, rng.permutation(n))
    return src_np, soffs, flens, doffs, darena


def _decode(ctx, batch, rng):
    """one ctx.decompress over `batch`: frames at odd offsets with gaps, destination slots of the items' capacities at odd offsets with gaps in
    shuffled order and canaries around them, status -1 and SIZE_SENTINEL before the call. Returns (launches per timer, status, sizes,
    destination arena, slot offsets)."""
    import torch
    frames, caps, _, _ = batch
    n = len(frames)
    src_np, soffs, flens, doffs, darena = _decode_layout(batch, rng)
    dev = _dev()
    src = _t(src_np)
    dst = torch.full((darena,), CANARY, dtype=torch.uint8, device=dev)
    out_sizes = torch.full((n,), SIZE_SENTINEL, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    for k in DEC_TIMERS:
        ctx.kernel_time(k)                                           # switches the timers on (and zeroes them)
    ctx.decompress(src, _segs(soffs, flens), dst, _segs(doffs, caps), out_sizes, status)
    torch.cuda.synchronize()
    launches = {k: ctx.kernel_time(k)[1] for k in DEC_TIMERS}
    return launches, status.cpu().numpy(), out_sizes.cpu().numpy(), dst.cpu().numpy(), doffs


def _check_decode(label, batch, chunk, st, sz, got, doffs):
    """every frame answered (status and size written); accepted only where libzstd decodes it, and then with libzstd's bytes; an undamaged frame
    refused only where libzstd refuses it (a damaged one may be refused where libzstd decodes something: test_truncated_and_corrupt_frames_do_not_crash);
    no byte outside the slots changed"""
    frames, caps, want, damaged = batch

    def at(idx):
        return [(int(i), int(i) // chunk, int(st[i])) for i in idx[:8]]          # (frame, chunk, status)
    silent = np.nonzero((st == -1) | (sz == SIZE_SENTINEL))[0]
    assert silent.size == 0, (label, "frames no kernel answered (frame, chunk, status)", silent.size, at(silent))
    decodes = np.fromiter((w is not None for w in want), dtype=bool, count=len(want))
    acc = st == 0
    wrong = np.nonzero(acc & ~decodes)[0]
    assert wrong.size == 0, (label, "accepted where libzstd refuses (frame, chunk, status)", wrong.size, at(wrong))
    refused = np.nonzero(~damaged & ~acc & decodes)[0]
    assert refused.size == 0, (label, "refused where libzstd decodes (frame, chunk, status)", refused.size, at(refused))
    bad = [i for i in np.nonzero(acc)[0] if sz[i] != len(want[i]) or got[doffs[i]: doffs[i] + sz[i]].tobytes() != want[i]]
    assert not bad, (label, "bytes differ from libzstd's (frame, chunk, status)", len(bad), at(np.array(bad)))
    ok, where = _outside_slots_untouched(got, doffs, caps)
    assert ok, (label, "bytes outside the slots changed at", where)


def _chunk_frames(hint):
    """frames per pipeline chunk (zhip_decompress_batch_device): 65 536; in the several-block mode (a hint above 128 KiB) 65 536 block slots at
    2 x the hint's blocks + 2 per frame -- 10 922 at 256 KiB"""
    return 65536 if hint <= 131072 else 65536 // (2 * -(-hint // 131072) + 2)


def _per_chunk(chunks):
    return {0: 1, 2: chunks, 3: chunks, 4: chunks, 7: chunks, 9: chunks}


# (hint, frames, pipeline chunks); slot streams -- hint 0: one, K1b on the side stream; hint 4 096: min(chunks, 3), K1b before K2; 256 KiB: one
DECODE_SHAPES = [(0, 4095, 1), (0, 4096, 1), (0, 6143, 1), (0, 6144, 1), (0, 65536, 1), (0, 65537, 2), (0, 131073, 3),
                 (4096, 6144, 1), (4096, 65537, 2), (4096, 196608, 3), (4096, 262145, 5), (262144, 10922, 1), (262144, 10923, 2)]


@pytest.mark.parametrize("hint,n,chunks", DECODE_SHAPES, ids=["hint%d-n%d" % s[:2] for s in DECODE_SHAPES])
def test_decode_launch_shape_sweep(zstd, decode_pool, ref, hint, n, chunks):
    """DeviceBatchContext.decompress at both sides of every switch point of zhip_decompress_batch_device, each shape in a fresh context. No hint:
    K1b beside K2 on the side stream and a batch's chunks one after another on ONE slot stream (its counters zeroed there from the second chunk
    on); 4 095 / 4 096 frames straddle the bin kernel's grid (2 workgroups below 4 096 items, 128 from), 6 143 / 6 144 K0 (from 6 144 frames per
    chunk), 65 536 / 65 537 / 131 073 are one, two and three chunks. Hint 4 096: K1b before K2 on the chunk's stream, chunks round-robin over
    three slot streams -- 262 145 frames are five chunks, the fourth and fifth on slots 0 and 1 again. Hint 256 KiB: the several-block mode,
    10 922 frames a chunk. Frames of several blocks sit inside every chunk and at the very end, so the fallback list takes global indices from
    every chunk; damaged copies -- wrong checksums among them, on reused slots and at the very end -- are spread over all chunks. Every frame
    against libzstd, canaries around every slot, and the launches the chunk count implies: one of K1, K2, K3, K1b and the pipeline span per
    chunk, one of the generic kernel per call."""
    chunk = _chunk_frames(hint)
    assert -(-n // chunk) == chunks
    batch = _decode_batch(decode_pool, ref, n, chunk, seed=hint + n, several_block_mode=hint > 131072)
    ctx = _context(hint=hint)
    try:
        launches, st, sz, got, doffs = _decode(ctx, batch, np.random.default_rng(n))
    finally:
        ctx.close()
    _check_decode((hint, n), batch, chunk, st, sz, got, doffs)
    assert launches == _per_chunk(chunks), (hint, n, "launches per timer", launches)


@pytest.mark.parametrize("n", [6144, 65537])
def test_decode_k0_on_and_off_give_the_same_answers(zstd, decode_pool, ref, n):
    """K0 has no timer. The sweep's kind of batch, n frames in one layout, through a default context (K0 in front of K1 from 6 144 frames per
    chunk: here every chunk but 65 537's second) and through one made with ZHIP_K0_MIN=1000000000 (K0 off): status, sizes and bytes identical
    frame by frame, and libzstd's."""
    batch = _decode_batch(decode_pool, ref, n, 65536, seed=n)
    res = []
    for env in ({}, {"ZHIP_K0_MIN": "1000000000"}):
        ctx = _context(env)
        try:
            launches, st, sz, got, doffs = _decode(ctx, batch, np.random.default_rng(n))
        finally:
            ctx.close()
        _check_decode((n, env), batch, 65536, st, sz, got, doffs)
        assert launches == _per_chunk(-(-n // 65536)), (n, env, launches)
        res.append((st, sz, got, doffs))
    (st0, sz0, got0, d0), (st1, sz1, got1, d1) = res
    assert np.array_equal(d0, d1)
    assert np.array_equal(st0, st1), [(int(i), int(st0[i]), int(st1[i])) for i in np.nonzero(st0 != st1)[0][:8]]
    assert np.array_equal(sz0, sz1), np.nonzero(sz0 != sz1)[0][:8]
    bad = [i for i in np.nonzero(st0 == 0)[0] if got0[d0[i]: d0[i] + sz0[i]].tobytes() != got1[d1[i]: d1[i] + sz1[i]].tobytes()]
    assert not bad, bad[:8]


@pytest.mark.parametrize("hint", [4096, 0])
def test_one_context_through_a_sequence_of_decode_calls(zstd, decode_pool, ref, hint):
    """One context, four calls: 262 145, 6 143, 131 073 and 262 145 frames (five, one, three and five chunks), other inputs and another layout
    each time, every frame checked after every call. What a call leaves behind -- arenas reserved for a larger batch, the slot streams and
    their counters and arenas, the fallback list and its length -- must not reach the next one. Hint 4 096: three slot streams; no hint: one
    slot stream with the side stream."""
    ctx = _context(hint=hint)
    try:
        for call, n in enumerate((262145, 6143, 131073, 262145)):
            batch = _decode_batch(decode_pool, ref, n, 65536, seed=100 * call + hint + 1)
            launches, st, sz, got, doffs = _decode(ctx, batch, np.random.default_rng(call + hint))
            _check_decode((hint, "call", call, n), batch, 65536, st, sz, got, doffs)
            assert launches == _per_chunk(-(-n // 65536)), (hint, "call", call, n, launches)
            del batch, got
    finally:
        ctx.close()


def test_arena_overrun_in_later_chunks(zstd, corpus, ref, monkeypatch):
    """Hint 256: three slot streams, and a compact arena of 4 x 256 + 1 KiB = 2 KiB of literal and sequence room per frame -- 128 MiB per chunk
    of 65 536. 196 608 tiny frames, but 2 048 frames of 128 KiB at the start of chunk 2 (slot 1) and as the whole of chunk 4 (slot 0 again). By
    the comment over that budget in zhip_decompress_batch_device, such frames need ~121 KiB each (45 KiB of literals, 76 KiB of sequences):
    ~242 MiB, about twice what either chunk has, so both run out of room (the code's figure, not measured here). The frames that find none are
    listed by K1 / K2 with their global indices -- past 65 536 and past 196 608 -- and served by the generic kernel after every slot drains:
    every large frame compared in HBM with its original, every tiny frame with libzstd's input, canaries around the tiny frames' slots."""
    import torch
    import bench
    from tests.corpus import Corpus
    monkeypatch.setattr(bench, "HOST_THREADS", min(bench.HOST_THREADS, 16))
    hint, item, nbig, distinct, ntiny = 256, 131072, 2048, 601, 4099
    n = 3 * 65536 + nbig
    big = np.zeros(n, dtype=bool)
    big[65536:65536 + nbig] = True
    big[3 * 65536:] = True
    big_idx, tiny_idx = np.nonzero(big)[0], np.nonzero(~big)[0]
    dev = _dev()
    raw = Corpus(device=dev, mix="silesia").frames(7000, distinct, chunk=256)
    torch.cuda.synchronize()
    big_frames, _ = bench.compress_on_host(raw.cpu().numpy(), item)
    rng = np.random.default_rng(hint)
    text = b"".join(corpus.frame_list(4100, 4))
    tiny_raws = []
    for _ in range(ntiny):
        m = int(rng.integers(0, hint + 1))
        s = int(rng.integers(0, len(text) - m))
        tiny_raws.append(text[s:s + m])
    tiny_frames = _ref_frames(ref, tiny_raws)
    frames = [None] * n
    for j, i in enumerate(tiny_idx):
        frames[i] = tiny_frames[j % ntiny]
    for j, i in enumerate(big_idx):
        frames[i] = big_frames[j % distinct]
    flens = np.fromiter((len(f) for f in frames), dtype=np.int64, count=n)
    soffs, sarena = _odd_layout(rng, flens, np.arange(n))
    src_np = np.full(sarena, 0x3C, dtype=np.uint8)
    for f, o in zip(frames, soffs):
        src_np[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    tcaps = np.array([len(tiny_raws[j % ntiny]) for j in range(len(tiny_idx))], dtype=np.int64)
    toffs, tarena = _odd_layout(rng, tcaps, rng.permutation(len(tiny_idx)))
    base = (tarena + 255) // 256 * 256                                # the large frames' slots follow, 128 KiB each
    doffs, caps = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    doffs[tiny_idx], caps[tiny_idx] = toffs, tcaps
    doffs[big_idx], caps[big_idx] = base + np.arange(2 * nbig, dtype=np.int64) * item, item
    dst = torch.full((base + 2 * nbig * item,), CANARY, dtype=torch.uint8, device=dev)
    out_sizes = torch.full((n,), SIZE_SENTINEL, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ctx = _context(hint=hint)
    try:
        for k in DEC_TIMERS:
            ctx.kernel_time(k)
        ctx.decompress(_t(src_np), _segs(soffs, flens), dst, _segs(doffs, caps), out_sizes, status)
        torch.cuda.synchronize()
        launches = {k: ctx.kernel_time(k)[1] for k in DEC_TIMERS}
    finally:
        ctx.close()
    st, sz = status.cpu().numpy(), out_sizes.cpu().numpy()
    failed = np.nonzero(st != 0)[0]
    assert failed.size == 0, ("frames not decoded (frame, chunk, status)", failed.size, [(int(i), int(i) // 65536, int(st[i])) for i in failed[:8]])
    assert np.array_equal(sz, caps), np.nonzero(sz != caps)[0][:8]
    same = (dst[base:].view(2 * nbig, item) == raw[torch.arange(2 * nbig, device=dev) % distinct]).all(dim=1).cpu().numpy()
    assert same.all(), ("large frames that differ from their originals", big_idx[~same][:8])
    got = dst[:base].cpu().numpy()
    bad = [int(tiny_idx[j]) for j in range(len(tiny_idx)) if got[toffs[j]: toffs[j] + tcaps[j]].tobytes() != tiny_raws[j % ntiny]]
    assert not bad, ("tiny frames that differ", len(bad), bad[:8])
    ok, where = _outside_slots_untouched(got, toffs, tcaps)
    assert ok, ("bytes outside the tiny frames' slots changed at", where)
    assert launches == _per_chunk(4), ("launches per timer", launches)
