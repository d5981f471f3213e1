"""The fast strategy (levels 1, 2, negative levels, STRATEGY_FAST) through the flat match kernels: one lane per source in zhip_encode_match_flat_fast*_kernel,
one source per CU with its bytes in LDS in zhip_encode_match_lds_fast_kernel (ze_fast_flat_np). Every frame of every call is compared with
libzstd 1.5.7 (tests/reflib.checker()); nothing is sampled. The knobs are read when a thread's context is created, so calls under a knob run in a fresh thread."""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEVELS = (1, 2, -1, -7)


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
        return list(pool.map(lambda r: ref.compress(r, **kw), raws))


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


@pytest.fixture(scope="module")
def mixed(corpus):
    """~300 sources of 63 ... 131 072 bytes: the size and kind mix of test_mixed_small_batch_through_the_large_batch_search, and sizes around the LDS kernel's 16-byte staging units"""
    rng = np.random.default_rng(5)
    raws = []
    for i in range(288):
        n = int(rng.choice([63, 64, 100, 4096, 30000, 131071, 131072], p=[0.02, 0.02, 0.06, 0.2, 0.2, 0.1, 0.4]))
        kind = i % 6
        r = (corpus.frame_bytes(i)[:n] if kind < 3 else rng.bytes(n) if kind == 3 else bytes(rng.integers(0, 3, n, dtype=np.uint8)) if kind == 4
             else (rng.bytes(int(rng.integers(1, 900))) * (n + 1))[:n])
        raws.append(r)
    raws += [corpus.frame_bytes(9)[:n] for n in (64, 65, 79, 80, 81, 4095, 4096, 4097, 16384, 65536, 131071, 131072)]
    return raws


@pytest.fixture(scope="module")
def mixed_ref(ref, mixed):
    from tests import reflib
    return {(lvl, ck): _ref_frames(ref, mixed, level=lvl, flags=reflib.DEFAULT_FLAGS | (reflib.F_CHECKSUM if ck else 0)) for lvl in LEVELS for ck in (False, True)}


def _device_compress(ctx, raws):
    """raws through DeviceBatchContext.compress, slots of zhip_compress_bound back to back; returns the frames"""
    import torch
    from zstandard_amd import _lib
    dev = torch.device("cuda", 0)
    n = len(raws)
    lens = np.array([len(r) for r in raws], dtype=np.int64)
    offs = np.zeros(n, dtype=np.int64); offs[1:] = np.cumsum(lens)[:-1]
    bound_of = {}
    for x in set(lens.tolist()): bound_of[x] = int(_lib.lib().zhip_compress_bound(int(x)))
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
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert not st.any(), (np.nonzero(st)[0][:8], st[np.nonzero(st)[0][:8]])
    got = dst.cpu().numpy(); sz = out_sizes.cpu().numpy()
    return [got[doffs[i]: doffs[i] + sz[i]].tobytes() for i in range(n)]


@pytest.mark.parametrize("pairs", [1, 2])
def test_flat_kernel_takes_fast_strategy_batches(zstd, mixed, mixed_ref, pairs):
    """ZHIP_E1LDS_MAX=0 keeps the LDS-source kernel out of the way: the flat kernel proper, at one and at two pairs per trip (ZHIP_FAST_PAIRS), levels 1, 2, -1, -7, with and
    without the checksum trailer. Timer 8 brackets the flat launch: a level-1 batch through a device context counts one (none before the fast strategy had a flat search)."""
    from zstandard_amd.device import DeviceBatchContext

    def run():
        out = {}
        for lvl in LEVELS:
            for ck in (False, True):
                res = zstd.ZstdCompressor(level=lvl, write_checksum=ck).multi_compress_to_buffer(mixed)
                out[(lvl, ck)] = [res[i].tobytes() for i in range(len(mixed))]
        back = zstd.ZstdDecompressor().multi_decompress_to_buffer(out[(1, True)])
        out["back"] = [back[i].tobytes() for i in range(len(mixed))]
        ctx = DeviceBatchContext(level=1)
        try:
            ctx.kernel_time(8)                                           # switches the timers on (and zeroes them)
            out["device"] = _device_compress(ctx, mixed)
            out["launches"] = {k: ctx.kernel_time(k)[1] for k in (1, 5, 6, 8)}
        finally:
            ctx.close()
        return out

    out = _in_fresh_thread({"ZHIP_E1LDS_MAX": "0", "ZHIP_FAST_PAIRS": str(pairs)}, run)
    assert out["launches"][8] >= 1, ("the flat match kernel did not serve the level-1 batch", out["launches"])
    assert out["launches"][8] == 1 and out["launches"][5] == 1 and out["launches"][6] == 1 and out["launches"][1] == 0, out["launches"]
    for key, want in mixed_ref.items():
        bad = [i for i in range(len(mixed)) if out[key][i] != want[i]]
        assert not bad, (key, len(bad), bad[:8], [len(mixed[i]) for i in bad[:8]])
    bad = [i for i in range(len(mixed)) if out["device"][i] != mixed_ref[(1, False)][i]]
    assert not bad, ("device context", len(bad), bad[:8])
    assert out["back"] == mixed


def test_small_batches_with_the_source_in_lds(zstd, ref, mixed, mixed_ref):
    """No override: ~300 sources are a small batch and take the LDS-source kernel, one source per CU. The four LDS shapes (areas of 4 KiB, 16 KiB, 64 KiB, one block, picked from
    the batch's largest source) each get a batch of their own with sizes around the 16-byte staging units."""
    from tests import reflib

    def run():
        out = {}
        for lvl in LEVELS:
            res = zstd.ZstdCompressor(level=lvl, write_checksum=True).multi_compress_to_buffer(mixed)
            out[lvl] = [res[i].tobytes() for i in range(len(mixed))]
        for cap in (4096, 16384, 65536):
            sub = [r for r in mixed if len(r) <= cap]
            res = zstd.ZstdCompressor(level=1).multi_compress_to_buffer(sub)
            out[("cap", cap)] = [res[i].tobytes() for i in range(len(sub))]
        return out

    out = _in_fresh_thread({}, run)
    for lvl in LEVELS:
        bad = [i for i in range(len(mixed)) if out[lvl][i] != mixed_ref[(lvl, True)][i]]
        assert not bad, (lvl, len(bad), bad[:8], [len(mixed[i]) for i in bad[:8]])
    for cap in (4096, 16384, 65536):
        idx = [i for i, r in enumerate(mixed) if len(r) <= cap]
        assert len(idx) >= 8 and max(len(mixed[i]) for i in idx) == cap
        bad = [i for k, i in enumerate(idx) if out[("cap", cap)][k] != mixed_ref[(1, False)][i]]
        assert not bad, (cap, len(bad), bad[:8])


def test_explicit_fast_parameters(zstd, ref, corpus):
    """ZstdCompressionParameters(strategy=STRATEGY_FAST, min_match, target_length, hash_log): 64 sources each, against the checker with the same parameters"""
    rng = np.random.default_rng(11)
    raws = [corpus.frame_bytes(400 + i)[: int(rng.integers(64, 24000))] for i in range(60)] + [corpus.frame_bytes(470), b"ab" * 40, bytes(rng.integers(0, 2, 5000, dtype=np.uint8)), rng.bytes(3000)]
    P = zstd.ZstdCompressionParameters
    for m in (4, 5, 6, 7):
        for t in (0, 2, 9):
            for h in (10, 14):
                kw = dict(strategy=zstd.STRATEGY_FAST, min_match=m, target_length=t, hash_log=h)
                res = zstd.ZstdCompressor(compression_params=P(**kw)).multi_compress_to_buffer(raws)
                with ThreadPoolExecutor(16) as pool:
                    want = list(pool.map(lambda r: ref.compress_advanced(r, level=3, flags=1, **kw), raws))
                bad = [i for i in range(len(raws)) if res[i].tobytes() != want[i]]
                assert not bad, (kw, len(bad), bad[:8], [len(raws[i]) for i in bad[:8]])


@pytest.mark.parametrize("lds_max", ["0", None], ids=["flat", "lds"])
def test_tables_across_calls_and_levels(zstd, ref, corpus, lds_max):
    """One thread's context: level 1, level 3, level 1 on the same sources shuffled (other sources' cells in every slot), level -3, level 3, then 70 small level-1 calls -- more
    than the 63 launch numbers a zeroed allocation has -- and level 3 once more. The two strategies lay their tables out differently in the same allocation."""
    rng = np.random.default_rng(21)
    big = [corpus.frame_bytes(600 + i)[: int(rng.integers(64, 131073))] for i in range(200)]
    shuffled = [big[i] for i in rng.permutation(len(big))]
    pool = corpus.frame_bytes(650) + corpus.frame_bytes(651)
    small = []
    for _ in range(70):
        small.append([pool[o: o + n] for o, n in zip(rng.integers(0, len(pool) - 3072, 64).tolist(), rng.integers(1024, 3073, 64).tolist())])
    steps = [(big, 1), (big, 3), (shuffled, 1), (big, -3), (shuffled, 3)] + [(s, 1) for s in small] + [(big, 3)]

    def run():
        out = []
        for raws, level in steps:
            res = zstd.ZstdCompressor(level=level).multi_compress_to_buffer(raws)
            out.append([res[i].tobytes() for i in range(len(raws))])
        return out

    out = _in_fresh_thread({"ZHIP_E1LDS_MAX": lds_max} if lds_max is not None else {}, run)
    cache = {}
    for k, (raws, level) in enumerate(steps):
        key = (id(raws), level)
        if key not in cache: cache[key] = _ref_frames(ref, raws, level=level)
        bad = [i for i in range(len(raws)) if out[k][i] != cache[key][i]]
        assert not bad, ("call %d, level %d" % (k, level), len(bad), bad[:8])


def test_one_large_launch_with_the_placement_pick(zstd, ref, corpus):
    """34 000 small sources (64 bytes ... 6 KiB, a few of a whole block: the shape of test_fast_strategy_batches_above_32768_sources) at level 1 through a device context: ONE flat
    launch, its tables' placement picked by probe launches of the fast search. All frames compared."""
    from zstandard_amd.device import DeviceBatchContext
    rng = np.random.default_rng(83)
    pool = [corpus.frame_bytes(1200 + i) for i in range(40)]
    raws = []
    for i in range(34000):
        b = pool[i % 40]; o = int(rng.integers(0, 120000)); n = int(rng.integers(64, 6145)) if i % 500 else 131072
        raws.append(b[o:o + n] if n < 131072 else b)
    ctx = DeviceBatchContext(level=1)
    try:
        ctx.kernel_time(8)
        got = _device_compress(ctx, raws)
        launches = ctx.kernel_time(8)[1]
        pick_ms, _ = ctx.table_pick()
    finally:
        ctx.close()
    assert launches == 1 and pick_ms[0] > 0, (launches, pick_ms)
    want = _ref_frames(ref, raws, level=1)
    bad = [i for i in range(len(raws)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:8], [len(raws[i]) for i in bad[:8]])
