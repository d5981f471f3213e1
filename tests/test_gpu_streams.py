"""The device API as what include/zstd_hip.h says it is: an asynchronous call on the caller's stream ("Ordering and threads" there).

tests/test_gpu_launch_shapes.py makes every call on the null stream, with inputs finished long before and a device-wide sync right behind.
Here the same batches, layouts and checks -- its helpers, imported -- run the way a pipeline runs them:

a. on a torch.cuda.Stream() that is not the current one, read after that stream's own synchronize();
b. between a producer and consumers queued on the same stream with no host sync: the sources and the segment tables are filled by copies that
   sit BEHIND a measured device-side delay, the outputs are copied away and overwritten by work queued right behind the call -- so a call that
   starts before what precedes it on the stream decodes 0x3C and empty segment tables, and a call whose tail is not waited for leaves canaries
   in the copies; compress -> decompress chained the same way, the frame lengths taken from out_sizes on the device;
c. one context through consecutive calls with no sync between them (arenas regrown under a pending call, slots reused, the arrangement changed);
d. two contexts on two streams, queued interleaved from one host thread and from two threads released by a barrier;
e. zhip_ctx_set_ddict / zhip_ctx_set_cparams between calls that are still pending.

zhip_decompress_batch_device runs its chunks on up to three internal slot streams and K1b on a side stream per slot, tied to the caller's stream
by event waits only: the decode shapes cross one slot stream with the side stream (no hint; 65 537 frames are two chunks in series on it), three
slot streams (hint 4 096, 196 608 frames), the several-block mode (hint 256 KiB, two chunks) and -- "huf" -- 2 048 frames of 128 KiB that are all
Huffman literals and next to no sequences, where K1b on the side stream outlasts K2 by the most and K3 depends on the wait for it.

Every frame and byte is compared with libzstd 1.5.7 (tests/reflib.checker()); status is -1, out_sizes the sentinel and the destination canaries
before every call. No test uses a device-wide synchronize between queueing a call and reading its results, and none reads the kernel timers
(zhip_ctx_kernel_time waits for the device)."""
import ctypes as C
import math
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import pytest

from tests.test_gpu_launch_shapes import (CANARY, COMPRESS_ARRANGEMENTS, SIZE_SENTINEL, _check_compress_table, _check_decode, _chunk_frames,  # noqa: F401
                                          _compress_table_context, _compress_table_layout, _context, _decode_batch, _decode_layout, _dev,
                                          _odd_layout, _outside_slots_untouched, _ref_frames, _segs, _t, compress_table, decode_pool, zstd)

pytestmark = pytest.mark.gpu

CANARY2 = 0x5B                       # what the consumers write over the outputs behind a call
MIN_DELAY_MS = 50.0

# (hint, frames): see the module docstring; "huf" is no size hint over _huffman_batch
DECODE_SHAPES = [(0, 6144), (0, 65537), (4096, 196608), (262144, 10923), ("huf", 2048)]
DECODE_IDS = ["hint%s-n%d" % s for s in DECODE_SHAPES]


def _huffman_batch(ref, n):
    """n frames of 128 KiB whose blocks are Huffman-coded literals and next to no sequences: independent draws from a skewed 48-symbol
    distribution (~4.4 bits a byte, no repeats worth a match). 64 distinct ones, repeated."""
    rng = np.random.default_rng(77)
    p = 0.9 ** np.arange(48)
    raws = [(rng.choice(48, 131072, p=p / p.sum()) + 40).astype(np.uint8).tobytes() for _ in range(64)]
    with ThreadPoolExecutor(16) as pool:
        frames = list(pool.map(ref.compress, raws))
    assert max(len(f) for f in frames) < 100000 and min(len(f) for f in frames) > 60000      # entropy-coded, not raw blocks, not matches
    return [frames[i % 64] for i in range(n)], np.full(n, 131072, dtype=np.int64), [raws[i % 64] for i in range(n)], np.zeros(n, dtype=bool)


@pytest.fixture(scope="module")
def batches(decode_pool, ref):
    """batch(hint, n, seed=0): tests/test_gpu_launch_shapes._decode_batch for that shape (frames, capacities, libzstd's answers, which are
    damaged copies), made once per module"""
    made = {}

    def get(hint, n, seed=0):
        key = (hint, n, seed)
        if key not in made:
            if hint == "huf":
                made[key] = _huffman_batch(ref, n)
            else:
                made[key] = _decode_batch(decode_pool, ref, n, _chunk_frames(hint), seed=hint + n + seed, several_block_mode=hint > 131072)
        return made[key]
    return get


def _hint(hint):
    return 0 if hint == "huf" else hint


def _chunk(hint):
    return _chunk_frames(_hint(hint))


# ---------------------------------------------------------------------------------------------------------------- tensors of one call

def _outputs(t, n, darena):
    import torch
    dev = _dev()
    t.dst = torch.full((darena,), CANARY, dtype=torch.uint8, device=dev)
    t.out_sizes = torch.full((n,), SIZE_SENTINEL, dtype=torch.int64, device=dev)
    t.status = torch.full((n,), -1, dtype=torch.int32, device=dev)


def _tensors(src_np, soffs, slens, doffs, caps, darena, staged):
    """the device tensors of one call, made on the current stream. staged: the source arena holds 0x3C and both segment tables zeros (an
    empty item at offset 0: whatever reads them too early stays inside every buffer); t.fill() queues the copies that put the real contents
    there from staging tensors."""
    import torch
    dev = _dev()
    n = len(soffs)
    t = SimpleNamespace(n=n, doffs=doffs, caps=caps)
    src, ssegs, dsegs = _t(src_np), _segs(soffs, slens), _segs(doffs, caps)
    if staged:
        t.src = torch.full((len(src_np),), 0x3C, dtype=torch.uint8, device=dev)
        t.src_segs, t.dst_segs = torch.zeros_like(ssegs), torch.zeros_like(dsegs)

        def fill():
            t.src.copy_(src, non_blocking=True)
            t.src_segs.copy_(ssegs, non_blocking=True)
            t.dst_segs.copy_(dsegs, non_blocking=True)
        t.fill = fill
    else:
        t.src, t.src_segs, t.dst_segs = src, ssegs, dsegs
    _outputs(t, n, darena)
    return t


def _decode_tensors(batch, rng, staged=False):
    src_np, soffs, flens, doffs, darena = _decode_layout(batch, rng)
    return _tensors(src_np, soffs, flens, doffs, batch[1], darena, staged)


def _compress_tensors(table, rng, staged=False):
    src_np, soffs, slens, doffs, caps, darena = _compress_table_layout(table, rng)
    return _tensors(src_np, soffs, slens, doffs, caps, darena, staged)


def _call(ctx, direction, t, stream):
    getattr(ctx, direction)(t.src, t.src_segs, t.dst, t.dst_segs, t.out_sizes, t.status, stream=stream)


def _consume(t):
    """what a pipeline queues behind a call: the outputs copied into fresh tensors, then overwritten. On the current stream."""
    c = SimpleNamespace(n=t.n, doffs=t.doffs, caps=t.caps, dst=t.dst.clone(), out_sizes=t.out_sizes.clone(), status=t.status.clone())
    t.dst.fill_(CANARY2)
    t.out_sizes.fill_(0)
    t.status.fill_(-2)
    return c


def _results(t):
    return t.status.cpu().numpy(), t.out_sizes.cpu().numpy(), t.dst.cpu().numpy(), t.doffs


def _check_decode_call(label, batch, chunk, t):
    st, sz, got, doffs = _results(t)
    _check_decode(label, batch, chunk, st, sz, got, doffs)


def _check_compress_call(label, table, t):
    st, sz, got, doffs = _results(t)
    _check_compress_table(label, table, st, sz, got, doffs, t.caps)


def _table(raws, want):
    """sources that are each one item with a slot of zhip_compress_bound, as a table of tests/test_gpu_launch_shapes' kind"""
    return raws, list(range(len(raws))), [], want


# ---------------------------------------------------------------------------------------------------------------- the delay

class _Delay:
    """A device-side delay on `stream`, built from a unit whose duration is MEASURED on the device with events (once per process):
    torch.cuda._sleep where it exists and does delay, else a 1 GiB device-to-device copy. queue(ms) puts ceil(ms / unit) units on the stream
    between two timing events, which the tests read for the delay's real length."""
    _unit = None        # (callable, ms)

    def __init__(self, stream):
        import torch
        self.stream = stream
        if _Delay._unit is None:
            if hasattr(torch.cuda, "_sleep"):
                unit = lambda: torch.cuda._sleep(1 << 22)                     # noqa: E731
                _Delay._unit = (unit, self._measure(unit))
            if _Delay._unit is None or _Delay._unit[1] < 0.2:
                with torch.cuda.stream(stream):
                    a = torch.empty(1 << 30, dtype=torch.uint8, device=_dev())
                    b = torch.empty_like(a)
                unit = lambda: b.copy_(a, non_blocking=True)                  # noqa: E731
                _Delay._unit = (unit, self._measure(unit))
            assert _Delay._unit[1] >= 0.2, ("no usable delay unit", _Delay._unit[1])
        self.unit, self.unit_ms = _Delay._unit

    def _measure(self, unit):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            unit()
            e0.record()
            for _ in range(4):
                unit()
            e1.record()
        self.stream.synchronize()
        return e0.elapsed_time(e1) / 4

    def queue(self, ms):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            e0.record()
            for _ in range(max(1, math.ceil(ms / self.unit_ms))):
                self.unit()
            e1.record()
        return e0, e1


def _window(s, delay, host_ms, queue_calls):
    """The measured part of (b): a delay of at least 12 x the warm-up call's host time on `s`, then queue_calls() -- producers, the library
    call(s), nothing that waits -- then `not s.query()` taken at once. Returns (the delay's events, whether the stream was still busy)."""
    events = delay.queue(max(MIN_DELAY_MS, 12.0 * host_ms))
    queue_calls()
    return events, not s.query()


def _close_window(label, s, events, still_busy, host_ms):
    """s.synchronize(), then what makes (b) mean something: the stream was still busy when the library call returned -- or the call was never
    made inside the window and the run proves nothing: it FAILS --, and the delay, timed by its events, was 10 x the call's host time."""
    s.synchronize()
    delay_ms = events[0].elapsed_time(events[1])
    print("%s: delay %.1f ms on the stream, host time of the warm-up call %.3f ms, ratio %.0f" % (label, delay_ms, host_ms, delay_ms / host_ms))
    assert still_busy, (label, "the stream had drained when the library call returned: the window was never open, this run proves nothing",
                        "delay ms", delay_ms, "host ms", host_ms)
    assert delay_ms >= 10.0 * host_ms, (label, "the delay is not 10 x the call's host time", delay_ms, host_ms)


# ---------------------------------------------------------------------------------------------------------------- a. not the current stream

@pytest.mark.parametrize("hint,n", DECODE_SHAPES, ids=DECODE_IDS)
def test_decode_on_a_stream_that_is_not_current(zstd, batches, hint, n):
    """Inputs made on a torch.cuda.Stream(), the call given that stream while the current one stays the null stream, the results read after
    that stream's synchronize() and nothing else: what the slot streams and the side stream wrote must be complete by then."""
    import torch
    batch = batches(hint, n)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = _decode_tensors(batch, np.random.default_rng(n))
    ctx = _context(hint=_hint(hint))
    try:
        assert torch.cuda.current_stream() == torch.cuda.default_stream() and s != torch.cuda.default_stream()
        _call(ctx, "decompress", t, s)
        s.synchronize()
        _check_decode_call(("not current", hint, n), batch, _chunk(hint), t)
    finally:
        ctx.close()


@pytest.mark.parametrize("arrangement", COMPRESS_ARRANGEMENTS)
def test_compress_on_a_stream_that_is_not_current(zstd, compress_table, arrangement):
    """The compress direction the same way: the LDS-source kernel, the flat search and the several-block flat search (22 items: far below the
    placement pick, which synchronises on the host by design)."""
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = _compress_tensors(compress_table, np.random.default_rng(COMPRESS_ARRANGEMENTS.index(arrangement) + 40))
    ctx = _compress_table_context(compress_table, arrangement)
    try:
        assert torch.cuda.current_stream() == torch.cuda.default_stream()
        _call(ctx, "compress", t, s)
        s.synchronize()
        _check_compress_call(("not current", arrangement), compress_table, t)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- b. producer and consumer

def _warm_up(ctx, direction, make, s):
    """one call of the measured call's shape, then a sync: `reserve` neither allocates nor frees in the measured call. Returns the call's host
    time in ms."""
    import torch
    with torch.cuda.stream(s):
        warm = make(False)
    t0 = time.perf_counter()
    _call(ctx, direction, warm, s)
    host_ms = (time.perf_counter() - t0) * 1e3
    s.synchronize()
    return host_ms


@pytest.mark.parametrize("hint,n", DECODE_SHAPES, ids=DECODE_IDS)
def test_decode_between_producer_and_consumers(zstd, batches, hint, n):
    """On one stream, no host sync in between: a measured delay; copies that fill the sources and both segment tables (0x3C and empty tables
    until then); zhip_decompress_batch_device; copies of dst / out_sizes / status into fresh tensors; CANARY2 over the originals. The COPIES are
    what is checked. The slot streams must not start before the stream reaches the call (they would decode 0x3C through empty tables: every
    status wrong) and the stream must not go on before every slot has drained (the copies would hold canaries, -1 and the sentinel)."""
    import torch
    batch = batches(hint, n)
    s = torch.cuda.Stream()
    ctx = _context(hint=_hint(hint))
    try:
        def make(staged):
            return _decode_tensors(batch, np.random.default_rng(n + 1), staged)
        host_ms = _warm_up(ctx, "decompress", make, s)
        with torch.cuda.stream(s):
            t = make(True)
        delay = _Delay(s)
        got = []

        def queue_calls():
            with torch.cuda.stream(s):
                t.fill()
            _call(ctx, "decompress", t, s)
        events, busy = _window(s, delay, host_ms, queue_calls)
        with torch.cuda.stream(s):
            got.append(_consume(t))
        _close_window(("decode", hint, n), s, events, busy, host_ms)
        _check_decode_call(("producer / consumer", hint, n), batch, _chunk(hint), got[0])
        assert bool((t.dst == CANARY2).all().item()) and bool((t.status == -2).all().item()), "the library wrote after the consumers ran"
    finally:
        ctx.close()


def test_compress_between_producer_and_consumers(zstd, compress_table):
    """The same for zhip_compress_batch_device, through the flat search."""
    import torch
    s = torch.cuda.Stream()
    ctx = _compress_table_context(compress_table, "flat")
    try:
        def make(staged):
            return _compress_tensors(compress_table, np.random.default_rng(51), staged)
        host_ms = _warm_up(ctx, "compress", make, s)
        with torch.cuda.stream(s):
            t = make(True)
        delay = _Delay(s)

        def queue_calls():
            with torch.cuda.stream(s):
                t.fill()
            _call(ctx, "compress", t, s)
        events, busy = _window(s, delay, host_ms, queue_calls)
        with torch.cuda.stream(s):
            got = _consume(t)
        _close_window("compress flat", s, events, busy, host_ms)
        _check_compress_call("producer / consumer", compress_table, got)
        assert bool((t.dst == CANARY2).all().item()), "the library wrote after the consumers ran"
    finally:
        ctx.close()


@pytest.mark.parametrize("decode_hint", [0, 300001])
def test_compress_then_decompress_chained_on_one_stream(zstd, compress_table, decode_hint):
    """The pipeline's hand-over: behind the delay the sources arrive, zhip_compress_batch_device writes frames into slots of
    zhip_compress_bound, torch operations on the stream build the decode's source table from the slot offsets and out_sizes ON THE DEVICE, and
    zhip_decompress_batch_device (another context: no hint -- the frames of several blocks are the generic kernel's, which runs on the
    caller's stream itself --, and the several-block mode) decodes them where they lie -- no host sync anywhere. The frames are libzstd's, the
    round trip the sources."""
    import torch
    srcs, items, short, want = compress_table
    items = [s for i, s in enumerate(items) if i not in short]                  # (a slot one byte short holds no frame to hand on)
    table = (srcs, items, [], want)
    n = len(items)
    lens = np.array([len(srcs[k]) for k in items], dtype=np.int64)
    s = torch.cuda.Stream()
    cctx, dctx = _compress_table_context(table, "lds"), _context(hint=decode_hint)
    try:
        def make(staged):
            c = _compress_tensors(table, np.random.default_rng(61), staged)
            d = SimpleNamespace(n=n, caps=lens)
            d.doffs, darena = _odd_layout(np.random.default_rng(62), lens, np.random.default_rng(63).permutation(n))
            d.dst_segs = _segs(d.doffs, lens)
            _outputs(d, n, darena)
            return c, d

        def chain(c, d):
            _call(cctx, "compress", c, s)
            with torch.cuda.stream(s):
                d.src, d.src_segs = c.dst, torch.stack([c.dst_segs[:, 0], c.out_sizes], dim=1).contiguous()
            _call(dctx, "decompress", d, s)
        with torch.cuda.stream(s):
            c, d = make(False)
        t0 = time.perf_counter()
        chain(c, d)
        host_ms = (time.perf_counter() - t0) * 1e3
        s.synchronize()
        with torch.cuda.stream(s):
            c, d = make(True)
        delay = _Delay(s)

        def queue_calls():
            with torch.cuda.stream(s):
                c.fill()
            chain(c, d)
        events, busy = _window(s, delay, host_ms, queue_calls)
        with torch.cuda.stream(s):
            back = _consume(d)
            frames = _consume(c)
        _close_window(("chain", decode_hint), s, events, busy, host_ms)
        _check_compress_call(("chain", decode_hint), table, frames)
        st, sz, got, doffs = _results(back)
        assert not st.any(), (decode_hint, np.nonzero(st)[0][:8], st[np.nonzero(st)[0][:8]])
        assert np.array_equal(sz, lens), np.nonzero(sz != lens)[0][:8]
        bad = [i for i in range(n) if got[doffs[i]: doffs[i] + lens[i]].tobytes() != srcs[items[i]]]
        assert not bad, ("round trip differs", decode_hint, bad[:8])
        ok, where = _outside_slots_untouched(got, doffs, lens)
        assert ok, ("bytes outside the decode slots changed at", where)
    finally:
        cctx.close()
        dctx.close()


# ---------------------------------------------------------------------------------------------------------------- c. consecutive calls

def test_one_context_consecutive_decode_calls_without_sync(zstd, batches):
    """A fresh context, four calls back to back on one stream behind a delay, nothing waited for in between: 6 144 frames; 65 537 (every arena
    regrown -- DevBuf::reserve frees and reallocates -- while the first call is still pending, two chunks); 4 095 (the slot and its counters
    again, smaller); then zhip_ctx_set_size_hint(256 KiB) and 10 923 frames in the several-block mode (another arrangement of the same
    arenas). Each call has its own inputs and outputs; all four checked after the one synchronize()."""
    import torch
    s = torch.cuda.Stream()
    seq = [(0, 6144, 0), (0, 65537, 0), (0, 4095, 7), (262144, 10923, 0)]
    work = [batches(h, n, seed) for h, n, seed in seq]
    with torch.cuda.stream(s):
        ts = [_decode_tensors(b, np.random.default_rng(300 + k)) for k, b in enumerate(work)]
    delay = _Delay(s)
    ctx = _context()
    try:
        delay.queue(MIN_DELAY_MS)
        for (hint, n, _), t in zip(seq, ts):
            ctx.set_size_hint(hint)
            _call(ctx, "decompress", t, s)
        s.synchronize()
        for k, ((hint, n, _), b, t) in enumerate(zip(seq, work, ts)):
            _check_decode_call(("consecutive", "call", k, hint, n), b, _chunk_frames(hint), t)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def flat_table(corpus, ref):
    """numCU x 4 + 64 sources of 64 B ... 4 KiB: one more than the LDS-source kernel takes, so the flat search's"""
    import torch
    n = torch.cuda.get_device_properties(0).multi_processor_count * 4 + 64
    rng = np.random.default_rng(n)
    text = b"".join(corpus.frame_list(4200, 8))
    raws = []
    for _ in range(n):
        m = int(rng.integers(64, 4097))
        at = int(rng.integers(0, len(text) - m))
        raws.append(text[at:at + m])
    return _table(raws, _ref_frames(ref, raws))


def test_one_context_consecutive_compress_calls_without_sync(zstd, compress_table, flat_table):
    """A fresh context (ZHIP_MBC_MIN=0, as the several-block arrangement needs), three calls back to back on one stream behind a delay: the
    table through the LDS-source kernel, numCU x 4 + 64 small sources through the flat search (arenas and tables regrown under the pending
    call), then a size hint and the table through the several-block flat search. All three checked after the one synchronize()."""
    import torch
    s = torch.cuda.Stream()
    seq = [(compress_table, 0), (flat_table, 0), (compress_table, max(len(x) for x in compress_table[0]))]
    with torch.cuda.stream(s):
        ts = [_compress_tensors(tab, np.random.default_rng(400 + k)) for k, (tab, _) in enumerate(seq)]
    delay = _Delay(s)
    ctx = _context({"ZHIP_MBC_MIN": "0"})
    try:
        delay.queue(MIN_DELAY_MS)
        for (tab, hint), t in zip(seq, ts):
            ctx.set_size_hint(hint)
            _call(ctx, "compress", t, s)
        s.synchronize()
        for k, ((tab, hint), t) in enumerate(zip(seq, ts)):
            _check_compress_call(("consecutive", "call", k, hint), tab, t)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- d. two contexts, two streams

@pytest.mark.parametrize("threads", [False, True], ids=["one_thread_interleaved", "two_threads"])
def test_two_contexts_on_two_streams(zstd, batches, compress_table, flat_table, threads):
    """Context A (no hint, LDS-source compress) on stream A, context B (hint 4 096: three slot streams; the flat search) on stream B, each
    behind a delay on its own stream so that everything is queued before anything runs: a decode and a compress per context, other batches in
    each. Queued interleaved from one host thread, then each context's calls from a thread of its own, the two released by a barrier. Every
    frame of all four calls."""
    import torch
    shapes = [(0, 6144), (4096, 65537)] if threads else [(0, 65537), (4096, 196608)]
    tables = [compress_table, flat_table]
    work = [batches(h, n) for h, n in shapes]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    ctxs = [_context(), _context({"ZHIP_E1LDS_MAX": "0"}, hint=4096)]
    try:
        dec, com = [], []
        for k, s in enumerate(streams):
            with torch.cuda.stream(s):
                dec.append(_decode_tensors(work[k], np.random.default_rng(500 + k)))
                com.append(_compress_tensors(tables[k], np.random.default_rng(510 + k)))
        delays = [_Delay(s) for s in streams]
        for s in streams:
            s.synchronize()
        if threads:
            gate, errors = threading.Barrier(2), []

            def run(k):
                try:
                    gate.wait(60)
                    delays[k].queue(MIN_DELAY_MS)
                    _call(ctxs[k], "decompress", dec[k], streams[k])
                    _call(ctxs[k], "compress", com[k], streams[k])
                    streams[k].synchronize()
                except BaseException as e:                        # noqa: BLE001  (reported by the main thread)
                    errors.append((k, repr(e)))
            th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
            for x in th:
                x.start()
            for x in th:
                x.join(300)
            assert not errors and not any(x.is_alive() for x in th), errors
        else:
            for k in range(2):
                delays[k].queue(MIN_DELAY_MS)
            for direction, ts in (("decompress", dec), ("compress", com)):
                for k in range(2):
                    _call(ctxs[k], direction, ts[k], streams[k])
            for s in streams:
                s.synchronize()
        for k in range(2):
            _check_decode_call(("two contexts", threads, shapes[k]), work[k], _chunk_frames(shapes[k][0]), dec[k])
            _check_compress_call(("two contexts", threads, k), tables[k], com[k])
    finally:
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------------------------------------------------------- e. setters

N_DOCS = 16384


@pytest.fixture(scope="module")
def dictionaries(corpus, ref):
    """dictionary A (tests/golden/dict_json4k.bin, 112 640 bytes) and B (dict_json4k_16k.bin, 16 384 bytes: it fits A's buffers, so setting it
    reallocates nothing), and per dictionary a batch shaped as test_dictionary_frames_through_the_pipeline's: 16 384 JSON documents of 4 KiB
    (B's are others than A's), a one-byte source, one of 40 000 bytes, one that starts with dictionary content, two that straddle it"""
    import os
    import torch
    from tests.corpus import Corpus
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    blobs = {"A": open(os.path.join(golden, "dict_json4k.bin"), "rb").read(), "B": open(os.path.join(golden, "dict_json4k_16k.bin"), "rb").read()}
    docs = Corpus(frame_size=4096, device=_dev()).json_docs(0, 2 * N_DOCS).cpu().numpy()
    torch.cuda.synchronize()
    rng = np.random.default_rng(7)
    raws = {}
    for k, (name, dd) in enumerate(blobs.items()):
        mine = [docs[i].tobytes() for i in range(k * N_DOCS, (k + 1) * N_DOCS)]
        content, b30 = dd[-4000:], rng.bytes(30)
        raws[name] = mine + [b"a", corpus.frame_bytes(5)[:40000], (dd[-3000:] + mine[3])[:6000],
                             b30 + content[-20:] + b30[:15] + rng.bytes(10) + content[-40:] + b30[:25],
                             content[-300:] + content[-300:] + rng.bytes(5) + content[-64:] + content[-300:-250]]
    return blobs, raws


def _ref_dict_frames(ref, raws, level, blob):
    with ThreadPoolExecutor(16) as pool:
        return list(pool.map(lambda r: ref.compress(r, level=level, dict_data=blob), raws))


def test_set_ddict_between_pending_decode_calls(zstd, dictionaries, ref):
    """Behind a delay: a decode of A's batch (level-3 frames made with A; one frame made without a dictionary among them); at once, nothing
    waited for, zhip_ctx_set_ddict(B); a decode of B's batch. zhip_ctx_set_ddict uploads with blocking copies and digests on stream 0, neither
    ordered against the slot streams or a non-blocking caller stream: the contract (include/zstd_hip.h, "Setters") is that a setter which
    re-uploads waits for the device first. Both batches entirely right."""
    import torch
    blobs, raws = dictionaries
    work = []
    for name in "AB":
        frames = _ref_dict_frames(ref, raws[name], 3, blobs[name]) + [ref.compress(raws[name][0])]
        want = raws[name] + [raws[name][0]]
        work.append((frames, np.array([len(r) for r in want], dtype=np.int64), want, np.zeros(len(want), dtype=bool)))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ts = [_decode_tensors(b, np.random.default_rng(600 + k)) for k, b in enumerate(work)]
    delay = _Delay(s)
    from zstandard_amd.device import DeviceBatchContext
    ctx = DeviceBatchContext(dict_data=blobs["A"])
    try:
        ctx.set_size_hint(4096)
        keep = C.create_string_buffer(blobs["B"], len(blobs["B"]))
        delay.queue(MIN_DELAY_MS)
        _call(ctx, "decompress", ts[0], s)
        rc = ctx.L.zhip_ctx_set_ddict(ctx.ctx, C.cast(keep, C.c_void_p), len(blobs["B"]), 0)
        assert rc == 0, rc
        _call(ctx, "decompress", ts[1], s)
        s.synchronize()
        for k, name in enumerate("AB"):
            _check_decode_call(("set_ddict", name), work[k], 65536, ts[k])
    finally:
        ctx.close()


def test_set_cparams_between_pending_compress_calls(zstd, dictionaries, ref):
    """Behind a delay, on one context and one stream, nothing waited for: compress with dictionary A at level 3; zhip_ctx_set_cparams(A, level
    1) -- the same dictionary digested for another level: the fingerprint must tell them apart --; compress; set_cparams(B, level 1); compress;
    set_cparams(no dictionary, level 1); compress. 8 192 documents + the odd sources per call (below the placement pick, which waits on the
    host by design). Every frame of the four batches libzstd's for that dictionary and level."""
    import torch
    from zstandard_amd import _lib
    from zstandard_amd.device import DeviceBatchContext
    blobs, raws = dictionaries
    steps = [("A", 3), ("A", 1), ("B", 1), (None, 1)]
    tables = []
    for name, level in steps:
        src = raws[name or "A"][N_DOCS - 8192:]
        tables.append(_table(src, _ref_dict_frames(ref, src, level, blobs[name] if name else None)))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ts = [_compress_tensors(tab, np.random.default_rng(700 + k)) for k, tab in enumerate(tables)]
    delay = _Delay(s)
    ctx = DeviceBatchContext(dict_data=blobs["A"], level=3)
    try:
        ctx.set_size_hint(4096)
        ctx._ensure_cparams()
        s.synchronize()
        keep = []
        delay.queue(MIN_DELAY_MS)
        for k, (name, level) in enumerate(steps):
            if k:
                p = _lib.CParams()
                p.level, p.contentSizeFlag, p.checksumFlag, p.dictIDFlag = level, 1, 0, 1
                if name:
                    keep.append(C.create_string_buffer(blobs[name], len(blobs[name])))
                    p.dict, p.dictSize = C.cast(keep[-1], C.c_void_p), len(blobs[name])
                rc = ctx.L.zhip_ctx_set_cparams(ctx.ctx, C.byref(p))
                assert rc == 0, (k, rc, _lib.last_error())
            _call(ctx, "compress", ts[k], s)
        s.synchronize()
        for k, step in enumerate(steps):
            _check_compress_call(("set_cparams", k) + step, tables[k], ts[k])
    finally:
        ctx.close()
