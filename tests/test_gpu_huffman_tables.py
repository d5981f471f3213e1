"""The Huffman literal decoders on the MI355X, driven by explicit code tables: tests/test_emu_huffman_tables.py's families through the device API.

Every frame carries a table given as a weight list (tests/huffamilies.py, written by tests/craft.py) and is expected to decode to what the plain
model of tests/hufmodel.py computes, or to be refused where the model refuses; libzstd 1.5.7 (reflib.checker()) is asked about every frame first,
and a disagreement there is a failure of the test's model, not of a kernel (the model may be stricter only for "a stream not consumed exactly",
only in the damaged-stream family). The routes are test_gpu_sequences.py's, each in a fresh context:

  (a) frames of one block, no hint:              K1 -> K1b / K2 -> K3 (a table of log 12 is decoded inside K1);
  (b) a 1-byte raw block in front, hint 131 073: the several-block mode (treeless blocks inherit; a deep table is rebuilt from the weights in LDS);
  (c) the frames of (b), no hint:                K1 lists every one for the generic kernel.

proved by the pipeline's count of the frames it handed to the generic kernel (decode_fallbacks: 0, 0, all). The set runs once on each route with
every frame placed so that its aimed stream starts at its aimed offset mod 16 (the family walks all sixteen), then the dictionary set (the trained
dictionary of tests/golden with tables of log 11 and 12 in place of its own), then the K1b groups, then replicated and shuffled to REPLICATED items
on (a) and (b) -- above K0's 6 144 frames and above K1b's resident waves x 12 frames -- with ~1 % refused frames and one at the last index.

Layout and checks are test_gpu_launch_shapes.py's: slots of exactly the content size at odd offsets with gaps in shuffled order, canaries between
them, status -1 and a size sentinel before the call, so a frame no kernel answered fails."""
import numpy as np
import pytest

from tests import huffamilies as H
from tests import hufmodel
from tests.test_emu_sequences import TRAINED, TRAINED_CONTENT_OFF
from tests.test_gpu_launch_shapes import (CANARY, DEC_TIMERS, SIZE_SENTINEL, _check_decode, _chunk_frames, _context, _dev, _odd_layout, _per_chunk, _segs, _t, zstd)  # noqa: F401  (zstd: the module fixture)
from tests.test_gpu_sequences import ITEM_SLOTS, REPLICATED, ROUTES, _handed_on

pytestmark = pytest.mark.gpu


def _judged(cases, ref, oracle):
    for c in cases:
        c.build(oracle.xxh64)
        try: hufmodel.check_model(ref, c.frame, c.want, c.cap, c.why, c.model_dict(), stricter_allowed=c.damaged and c.family == "damaged streams")
        except AssertionError as e: raise AssertionError("%s / %s: %s" % (c.family, c.name, e))
    return cases


class _Set:
    pass


@pytest.fixture(scope="module")
def frame_sets(ref, oracle):
    """the families as frames of one block (route a) and behind a raw block (routes b and c), each judged by libzstd once"""
    s = _Set()
    cases = [c for gen in H.FAMILIES.values() for c in gen()]
    s.one_block = _judged([c for c in cases if len(c.blocks) == 1], ref, oracle)
    s.led = _judged([c.with_lead() for c in cases], ref, oracle)
    return s


def _placed_layout(cases, rng):
    """source arena: every frame behind a gap of 1 ... 40 bytes, odd unless the case aims a stream at an offset mod 16 -- then the gap that puts it
    there (device allocations are aligned far above 16, so arena offsets are absolute alignments)"""
    offs, pos = np.zeros(len(cases), dtype=np.int64), 0
    for i, c in enumerate(cases):
        pos += int(rng.integers(1, 25))
        pos = pos + c.pad_for(pos) if c.align else pos | 1
        offs[i] = pos
        pos += len(c.frame)
    return offs, pos + int(rng.integers(1, 41))


def _decode(ctx, cases, rng):
    import torch
    n = len(cases)
    caps = np.array([c.cap for c in cases], dtype=np.int64)
    flens = np.fromiter((len(c.frame) for c in cases), dtype=np.int64, count=n)
    soffs, sarena = _placed_layout(cases, rng)
    src_np = np.full(sarena, 0x3C, dtype=np.uint8)
    for c, o in zip(cases, soffs): src_np[o:o + len(c.frame)] = np.frombuffer(c.frame, dtype=np.uint8)
    doffs, darena = _odd_layout(rng, caps, rng.permutation(n))
    src = _t(src_np)
    assert src.data_ptr() % 64 == 0
    dst = torch.full((darena,), CANARY, dtype=torch.uint8, device=_dev())
    out_sizes = torch.full((n,), SIZE_SENTINEL, dtype=torch.int64, device=_dev())
    status = torch.full((n,), -1, dtype=torch.int32, device=_dev())
    for k in DEC_TIMERS: ctx.kernel_time(k)
    ctx.decompress(src, _segs(soffs, flens), dst, _segs(doffs, caps), out_sizes, status)
    torch.cuda.synchronize()
    launches = {k: ctx.kernel_time(k)[1] for k in DEC_TIMERS}
    return launches, status.cpu().numpy(), out_sizes.cpu().numpy(), dst.cpu().numpy(), doffs, soffs


def _run(label, cases, hint, chunks, seed, fallbacks, dict_data=None):
    from zstandard_amd.device import DeviceBatchContext
    if dict_data is None: ctx = _context(hint=hint)
    else:
        ctx = DeviceBatchContext(dict_data=dict_data, dict_type=0)
        if hint: ctx.set_size_hint(hint)
    try:
        launches, st, sz, got, doffs, soffs = _decode(ctx, cases, np.random.default_rng(seed))
        handed_on = ctx.decode_fallbacks()
    finally:
        ctx.close()
    refused = [(c.family, c.name, int(s)) for c, s in zip(cases, st) if c.want is not None and s != 0][:6]
    wrong = [(c.family, c.name) for i, c in enumerate(cases) if c.want is not None and st[i] == 0 and got[doffs[i]: doffs[i] + sz[i]].tobytes() != c.want][:6]
    accepted = [(c.family, c.name, c.why) for c, s in zip(cases, st) if c.want is None and s == 0][:6]
    assert not refused and not wrong and not accepted, (label, "refused", refused, "wrong bytes", wrong, "accepted", accepted)
    batch = ([c.frame for c in cases], np.array([c.cap for c in cases], dtype=np.int64), [c.want for c in cases], np.zeros(len(cases), dtype=bool))
    _check_decode(label, batch, _chunk_frames(hint), st, sz, got, doffs)               # every frame answered, sizes, and no byte outside the slots
    assert handed_on == fallbacks, (label, "frames the pipeline handed to the generic kernel", handed_on, "expected", fallbacks, "of", len(cases))
    assert launches == _per_chunk(chunks), (label, "launches per timer", launches)
    return soffs


@pytest.mark.parametrize("route", list(ROUTES))
def test_huffman_families_on_three_routes(zstd, frame_sets, route):
    """the set once: every family, every frame, in one call of a fresh context; the streams family's frames lie where their streams start at every
    offset 0 .. 15 mod 16 (asserted from the census at the frames' places)"""
    which, hint = ROUTES[route]
    cases = getattr(frame_sets, which)
    assert len(cases) < _chunk_frames(hint)
    if hint: assert sum(len(c.blocks) for c in cases) <= min(6 * len(cases), ITEM_SLOTS)
    soffs = _run(route, cases, hint, 1, seed=len(cases) + hint, fallbacks=_handed_on(route, len(cases)))
    reached = set()
    for c, o in zip(cases, soffs):
        if c.family == "streams": reached |= c.huf_census(int(o))
    missing = [e for e in H.REQUIRED["streams"] if e not in reached]
    assert not missing, missing


@pytest.mark.parametrize("route", list(ROUTES))
def test_dictionary_tables_of_log_11_and_12(zstd, ref, oracle, route):
    """the trained dictionary with explicit tables of log 11 (shared with K1b where it lies) and log 12 (too deep: rebuilt in K1) in place of its
    own, a context per dictionary: frames whose first block is treeless in one and in four streams, frames with a table of their own"""
    which, hint = ROUTES[route]
    trained = open(TRAINED, "rb").read()
    for name, d, cases in H.dictionaries(trained, TRAINED_CONTENT_OFF):
        if which == "led": cases = [c.with_lead() for c in cases]
        else: cases = [c for c in cases if len(c.blocks) == 1]
        cases = _judged(cases, ref, oracle)
        assert any(c.want is not None for c in cases), "libzstd does not load the dictionary"
        _run("dictionary %s, %s" % (name, route), cases, hint, 1, seed=hint + len(name), fallbacks=_handed_on(route, len(cases)), dict_data=d)


def test_k1b_groups_with_damaged_neighbours(zstd, ref, oracle):
    """1, 11, 12, 13 and 25 Huffman frames among raw-literal ones, a damaged stream in the first and in the twelfth: every neighbour decodes"""
    for name, cases in H.k1b_groups():
        _judged(cases, ref, oracle)
        _run("K1b groups: " + name, cases, 0, 1, seed=len(cases), fallbacks=0)


def _replicated(cases, n, seed):
    """n items: the valid frames over and over in shuffled order (so K1b's groups mix table logs), ~1 % of the places given to frames that must be
    refused, one of them at the last index"""
    rng = np.random.default_rng(seed)
    good = [c for c in cases if c.want is not None]
    bad = [c for c in cases if c.want is None]
    assert len(bad) >= 8
    picks = [good[i] for i in rng.integers(0, len(good), n)]
    for i in list(rng.choice(n - 1, n // 100, replace=False)) + [n - 1]:
        picks[int(i)] = bad[int(rng.integers(0, len(bad)))]
    return picks


@pytest.mark.parametrize("route", ["a: one block", "b: several-block mode"])
def test_huffman_families_replicated(zstd, frame_sets, route):
    """REPLICATED items in shuffled order with ~1 % refused frames: K0 in front of K1 on route (a), K1b's groups of 12 over every resident wave
    several times, a refused frame at the last index; under the hint two pipeline chunks"""
    which, hint = ROUTES[route]
    cases = _replicated(getattr(frame_sets, which), REPLICATED, seed=hint + 11)
    chunk = _chunk_frames(hint)
    chunks = -(-REPLICATED // chunk)
    assert chunks == (2 if hint else 1)
    if hint: assert max(sum(len(c.blocks) for c in cases[i:i + chunk]) for i in range(0, REPLICATED, chunk)) <= ITEM_SLOTS * 7 // 8
    assert cases[-1].want is None and len({c.name for c in cases}) > 300
    _run(route + ", replicated", cases, hint, chunks, seed=hint + 12, fallbacks=0)
