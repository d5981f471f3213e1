"""The double-fast search (level 3) on the GPU with the aimed sources of tests/dfast_sources.py, in batches that make the library choose each of its forms: a few hundred sources
(the LDS-source kernel, and under ZHIP_E1LDS_MAX=0 the flat kernel at four probes a trip), the set replicated to 4 097, 32 769 and 65 537 items (four, three and two probes),
sources of several blocks under a size hint (the flat block form), dictionary contexts (the flat dictionary search) and one context through consecutive calls (launch numbers in
the cells), and dictionary contexts with sources above the attach cutoff and of two blocks (libzstd's table-copy mode: ze_dfast_ext in the generic kernel). Every frame of every call is compared with libzstd 1.5.7 (tests/reflib.checker()); nothing is sampled. Destination slots lie in an arena of canary bytes with gaps
between them. Timer 8 brackets the match stage's launch (LDS-source and flat kernels alike); the lane-serial kernel (timer 5) is launched once per call whatever the batch holds
-- it takes the sources below 64 bytes --, so its count says nothing about which kernel searched and is only held at one.

What a launch count does NOT show: timer 8 brackets the LDS-source kernel, the flat kernels and the several-block flat kernel alike, and the library has no counter that tells
them apart on the device. That the small batch takes the LDS-source kernel and ZHIP_E1LDS_MAX=0 the flat one, that a size hint with ZHIP_MBC_MIN=0 engages the several-block
search, and that a dictionary source above 16 KiB is searched in copy mode rest on the dispatch rules of zhip_compress_batch_device (zhip_lib.hip) and ze_compress_block, not on
an observation here: were a rule to change, these cases would still compare every frame with libzstd but through another kernel. The replicated batches are different: each is ONE
launch of a size only one flat kernel takes (four probes up to 32 768 sources, three up to 65 536, two above). On the host the same forms are reached directly and by name
(tests/test_emu_dfast.py, and the emulator's hooks in test_emu_kernels.py).

The properties the sources exist for are asserted against libzstd by tests/test_emu_dfast.py on the host; here the same bytes go through the device code."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import dfast_sources as ds

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GAP = 9


@pytest.fixture(scope="module")
def zstd():
    import zstandard_amd
    assert zstandard_amd._lib.lib().zhip_device_count() >= 1, "no GPU visible"
    return zstandard_amd


@pytest.fixture(scope="module")
def ref():
    from tests import reflib
    return reflib.checker()


def _ref_frames(ref, raws, **kw):
    with ThreadPoolExecutor(16) as pool:                     # (ctypes drops the GIL; the checker keeps a context per thread)
        return list(pool.map(lambda r: ref.compress(r, level=3, **kw), raws))


@pytest.fixture(scope="module")
def aimed(ref):
    """every one-block aimed source with libzstd's level-3 frame: computed once, shared, never changed"""
    raws = [c.raw for c in ds.one_block_sources()]
    assert len(raws) > 600 and min(len(r) for r in raws) == 8 and max(len(r) for r in raws) == ds.BLOCK
    return raws, _ref_frames(ref, raws)


@pytest.fixture(scope="module")
def small(aimed):
    """the aimed sources of 64 ... 4 200 bytes: what the replicated batches are made of"""
    raws, want = aimed
    idx = [i for i, r in enumerate(raws) if 64 <= len(r) <= 4200]
    assert len(idx) > 250
    return [raws[i] for i in idx], [want[i] for i in idx]


def _context(env=None, hint=0, **kw):
    """a fresh device context; `env` (the library's existing knobs) is set just around its creation, where the library reads it, and restored"""
    from zstandard_amd.device import DeviceBatchContext
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = DeviceBatchContext(level=3, **kw)
    finally:
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    if hint: ctx.set_size_hint(hint)
    return ctx


def _compress(ctx, raws, order=None):
    """raws (in `order`) through ctx.compress: sources back to back, destination slots of zhip_compress_bound with GAP canary bytes before, between and behind them.
    Returns (frames in the order of `raws`, launches per timer). Asserts every status and the canaries."""
    import torch
    from zstandard_amd import _lib
    dev = torch.device("cuda", 0)
    n = len(raws)
    order = np.arange(n) if order is None else np.asarray(order)
    lens = np.array([len(raws[i]) for i in order], dtype=np.int64)
    offs = np.zeros(n, dtype=np.int64); offs[1:] = np.cumsum(lens)[:-1]
    bound_of = {int(x): int(_lib.lib().zhip_compress_bound(int(x))) for x in set(lens.tolist())}
    caps = np.array([bound_of[int(x)] for x in lens], dtype=np.int64)
    doffs = GAP + np.concatenate([[0], np.cumsum(caps + GAP)[:-1]])
    total = int(doffs[-1] + caps[-1] + GAP)

    def segs(o, l):
        a = np.zeros((n, 2), dtype=np.int64); a[:, 0] = o; a[:, 1] = l
        return torch.from_numpy(a).to(dev)

    src = torch.from_numpy(np.frombuffer(b"".join(raws[i] for i in order), dtype=np.uint8).copy()).to(dev)
    dst = torch.full((total,), CANARY, dtype=torch.uint8, device=dev)
    out_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ctx.kernel_time(8)                                           # switches the timers on (and zeroes them)
    ctx.compress(src, segs(offs, lens), dst, segs(doffs, caps), out_sizes, status)
    torch.cuda.synchronize()
    launches = {k: ctx.kernel_time(k)[1] for k in (1, 5, 6, 8)}
    st = status.cpu().numpy(); sz = out_sizes.cpu().numpy(); got = dst.cpu().numpy()
    del src, dst
    assert not st.any(), (np.nonzero(st)[0][:8], st[np.nonzero(st)[0][:8]])
    assert (sz <= caps).all()
    gaps = np.concatenate([np.arange(GAP), ((doffs + caps)[:, None] + np.arange(GAP)[None, :]).ravel()])
    assert (got[gaps] == CANARY).all(), ("a byte outside every slot was written", gaps[np.nonzero(got[gaps] != CANARY)[0][:8]].tolist())
    frames = [None] * n
    for k, i in enumerate(order.tolist()): frames[i] = got[doffs[k]: doffs[k] + sz[k]].tobytes()
    return frames, launches


def _bad(frames, want, raws):
    bad = [i for i in range(len(want)) if frames[i] != want[i]]
    return (len(bad), bad[:8], [len(raws[i]) for i in bad[:8]]) if bad else None


@pytest.mark.parametrize("lds_max", [None, "0"], ids=["lds", "flat"])
def test_aimed_sources_as_one_small_batch(zstd, aimed, lds_max):
    """every aimed source, 8 ... 131 072 bytes, once: a small batch takes the LDS-source kernel (one source per CU, four probes), with ZHIP_E1LDS_MAX=0 the flat kernel; sources
    below 64 bytes are the lane-serial kernel's in both"""
    raws, want = aimed
    ctx = _context({"ZHIP_E1LDS_MAX": lds_max} if lds_max is not None else None)
    try:
        frames, t = _compress(ctx, raws)
    finally:
        ctx.close()
    assert t[8] == 1 and t[5] == 1 and t[6] == 1 and t[1] == 0, t
    assert not _bad(frames, want, raws), _bad(frames, want, raws)


@pytest.mark.parametrize("n", [4097, 32769, 65537])
def test_aimed_sources_replicated(zstd, small, n):
    """the small aimed sources over and over, in a shuffled order, up to 4 097, 32 769 and 65 537 items: one flat launch each, at four, three and two probes a trip"""
    import torch
    raws, want = small
    rng = np.random.default_rng(n)
    pick = np.concatenate([rng.permutation(len(raws)) for _ in range(n // len(raws) + 1)])[:n]
    batch = [raws[i] for i in pick]
    ctx = _context()
    try:
        frames, t = _compress(ctx, batch)
    finally:
        ctx.close()
    torch.cuda.empty_cache()
    assert t[8] == 1 and t[5] == 1 and t[6] == 1 and t[1] == 0, (n, t)
    bad = [k for k in range(n) if frames[k] != want[pick[k]]]
    assert not bad, (n, len(bad), bad[:8], [len(batch[k]) for k in bad[:8]])


def test_sources_of_several_blocks_under_a_size_hint(zstd, ref, aimed):
    """the two- and three-block sources among one-block ones under a size hint above one block (ZHIP_MBC_MIN=0: the batch need not be large): the flat search's block form,
    tables and repeat offsets carried from block to block"""
    raws = [c.raw for c in ds.block_sources()]
    some, some_want = aimed[0][::23], aimed[1][::23]
    batch = raws + some
    want = _ref_frames(ref, raws) + some_want
    ctx = _context({"ZHIP_MBC_MIN": "0", "ZHIP_E1LDS_MAX": "0"}, hint=max(len(r) for r in raws))
    try:
        frames, t = _compress(ctx, batch)
    finally:
        ctx.close()
    assert t[8] == 1, t
    assert not _bad(frames, want, batch), _bad(frames, want, batch)


def test_dictionary_families(zstd, ref):
    """the step and end-of-source families with their match targets in a raw-content dictionary, a context per dictionary: attach mode, the flat dictionary search"""
    batches = ds.dictionary_batches(group=24)
    assert 3 <= len(batches) <= 6
    for d, raws in batches:
        want = _ref_frames(ref, raws, dict_data=d)
        ctx = _context({"ZHIP_E1LDS_MAX": "0"}, dict_data=d)
        try:
            frames, t = _compress(ctx, raws)
        finally:
            ctx.close()
        assert t[8] == 1, t
        assert not _bad(frames, want, raws), (len(d), _bad(frames, want, raws))


def test_dictionary_sources_in_copy_mode(zstd, ref):
    """sources of 17 KiB and more, and of two blocks, on dictionary contexts: above the attach cutoff libzstd copies the dictionary's tables and searches with the dictionary as
    an external segment (ze_dfast_ext, run by the generic kernel -- timer 1 counts its launch)"""
    batches = ds.ext_batches(group=24)
    assert len(batches) == 4 and all(len(r) > 16384 for _, raws in batches for r in raws) and sum(1 for _, raws in batches for r in raws if len(r) > ds.BLOCK) == 2
    for d, raws in batches:
        want = _ref_frames(ref, raws, dict_data=d)
        ctx = _context(dict_data=d)
        try:
            frames, t = _compress(ctx, raws)
        finally:
            ctx.close()
        assert not _bad(frames, want, raws), (len(d), t, _bad(frames, want, raws))


def test_one_context_through_three_calls(zstd, small):
    """one context, three calls with the sources in another order each time: the tables are not zeroed in between, every slot holds another source's cells under another
    launch number"""
    raws, want = small
    rng = np.random.default_rng(77)
    ctx = _context({"ZHIP_E1LDS_MAX": "0"})
    try:
        for call in range(3):
            frames, t = _compress(ctx, raws, order=rng.permutation(len(raws)))
            assert t[8] == 1, (call, t)
            assert not _bad(frames, want, raws), (call, _bad(frames, want, raws))
    finally:
        ctx.close()
