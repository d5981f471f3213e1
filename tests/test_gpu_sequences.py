"""The decode kernels on the MI355X, driven by frames written from explicit sequences: tests/test_emu_sequences.py's families through the device API.

Every frame is described by its sequences (tests/seqfamilies.py), written by tests/craft.py and expected to decode to what the plain executor of
tests/seqmodel.py computes; libzstd 1.5.7 (reflib.checker()) is asked about every frame first, and a disagreement there is a failure of the
test's model, not of a kernel. The same set runs on three routes, each in a fresh context:

  (a) frames of one block, no hint:              K1 -> K2 -> K3;
  (b) a 1-byte raw block in front, hint 131 073: the several-block mode (symbolic repeat offsets from K2, resolved block by block in K3);
  (c) the frames of (b), no hint:                K1 lists every one for the generic kernel.

and in two sizes: the set once, and the set -- with checksummed copies, ~1 % invalid frames, an invalid one at the last index -- replicated and
shuffled to REPLICATED items, where K0, KX and the side stream run as they do in production.

The route is proved by the pipeline's own count of the frames it handed to the generic kernel (DeviceBatchContext.decode_fallbacks, read after
the call): 0 on (a) and (b), every frame on (c). The launch counts of the kernel timers are asserted too -- one K1 / K2 / K3 / K1b launch per
pipeline chunk, one of the generic kernel per call -- but they only say how the host cut the batch: a chunk is 65 536 frames without a hint and
10 922 under the hint of 131 073, so route (b)'s large batch comes as two chunks. Such a chunk has 65 536 item slots (one per block) and K1 hands
a frame that finds them used up to the generic kernel, so the large batch of (b) is drawn to stay below that (asserted), the frames of many
blocks -- the repeat-offset family -- among them at their share.

Layout and checks are test_gpu_launch_shapes.py's: frames and slots at odd offsets with gaps, slots of exactly the content size, canaries between
them, status -1 and a size sentinel before the call, so a frame no kernel answered fails."""
import struct

import numpy as np
import pytest

from tests import seqfamilies as F
from tests.seqmodel import K3, check_model
from tests.test_emu_sequences import TRAINED, TRAINED_CONTENT_OFF, TRAINED_REPS, trained_cases
from tests.test_gpu_launch_shapes import DEC_TIMERS, _check_decode, _chunk_frames, _context, _decode, _per_chunk, zstd  # noqa: F401  (zstd: the module fixture)

pytestmark = pytest.mark.gpu

HINT = 131073                        # the several-block mode at its smallest: six item slots per frame
REPLICATED = 12000                   # items of the large batches: above K0's 6 144 and above one several-block chunk (10 922)
ZE_DST_TOO_SMALL = 70


class _Set:
    pass


def _judged(cases, ref, oracle):
    for c in cases:
        c.build(oracle.xxh64)
        if not c.unjudged:
            try: check_model(ref, c.frame, c.want, c.cap, c.dict_data, c.raw_dict)
            except AssertionError as e: raise AssertionError("%s / %s: %s" % (c.family, c.name, e))
    return cases


def _with_checksums(cases):
    """copies of the valid frames with a content checksum (a right one; every 9th a wrong one)"""
    out = []
    for j, c in enumerate(c for c in cases if c.checksum is None and c.fcs == "auto" and not c.short_by and "claims" not in c.header):
        out.append(F.Case(c.family, c.name + " [checksum]", c.blocks, c.dict_data, c.raw_dict, checksum="wrong" if j % 9 == 4 else "right", start_reps=c.start_reps, header=dict(c.header)))
        if c.dict_data and not c.raw_dict: out[-1].content_off = c.content_off
    return out


@pytest.fixture(scope="module")
def frame_sets(ref, oracle):
    """the families as frames of one block (route a) and behind a raw block (routes b and c), each judged by libzstd once"""
    s = _Set()
    plain = F.plain_families(K3) + F.header_forms(K3, longest=True)
    s.one_block = _judged([c for c in plain if len(c.blocks) == 1], ref, oracle)
    s.led = _judged([c.with_lead() for c in plain], ref, oracle)
    s.one_block_ck = _judged(_with_checksums(s.one_block), ref, oracle)
    s.led_ck = _judged(_with_checksums(s.led), ref, oracle)
    return s


def _batch(cases):
    return ([c.frame for c in cases], np.array([c.cap for c in cases], dtype=np.int64), [c.want for c in cases], np.zeros(len(cases), dtype=bool))


def _replicated(valid, checksummed, n, seed, few_blocks=False):
    """n items: the valid and checksummed frames over and over in shuffled order, ~1 % of the places given to frames that must be refused
    (invalid sequences, wrong sizes, wrong checksums), one of them at the last index. few_blocks (the several-block mode, whose chunk has a
    pool of item slots): three picks in four among the frames of at most four blocks, the fourth among all"""
    rng = np.random.default_rng(seed)
    good = [c for c in valid + checksummed if c.want is not None and len(c.want) <= 70000]      # (the 128 KiB frames run in the small batch)
    bad = [c for c in valid + checksummed if c.want is None]
    assert len(bad) >= 8
    picks = [good[i] for i in rng.integers(0, len(good), n)]
    if few_blocks:
        small = [c for c in good if len(c.blocks) <= 4]
        for i in range(n):
            if i % 4: picks[i] = small[int(rng.integers(0, len(small)))]
    for i in list(rng.choice(n - 1, n // 100, replace=False)) + [n - 1]:
        picks[int(i)] = bad[int(rng.integers(0, len(bad)))]
    return picks


def _run(label, cases, hint, chunks, seed, fallbacks, dict_data=None, dict_type=0):
    from zstandard_amd.device import DeviceBatchContext
    batch = _batch(cases)
    if dict_data is None: ctx = _context(hint=hint)
    else:
        ctx = DeviceBatchContext(dict_data=dict_data, dict_type=dict_type)
        if hint: ctx.set_size_hint(hint)
    try:
        launches, st, sz, got, doffs = _decode(ctx, batch, np.random.default_rng(seed))
        handed_on = ctx.decode_fallbacks()
    finally:
        ctx.close()
    refused = [(c.family, c.name, int(s)) for c, s in zip(cases, st) if c.want is not None and s != 0][:6]
    wrong = [(c.family, c.name) for i, c in enumerate(cases) if c.want is not None and st[i] == 0 and got[doffs[i]: doffs[i] + sz[i]].tobytes() != c.want][:6]
    accepted = [(c.family, c.name, c.why) for c, s in zip(cases, st) if c.want is None and s == 0][:6]
    assert not refused and not wrong and not accepted, (label, "refused", refused, "wrong bytes", wrong, "accepted", accepted)
    _check_decode(label, batch, _chunk_frames(hint), st, sz, got, doffs)               # every frame answered, sizes, and no byte outside the slots
    short = [int(s) for c, s in zip(cases, st) if c.short_by]
    assert all(s == ZE_DST_TOO_SMALL for s in short), (label, "a slot one byte short", short)
    assert handed_on == fallbacks, (label, "frames the pipeline handed to the generic kernel", handed_on, "expected", fallbacks, "of", len(cases))
    assert launches == _per_chunk(chunks), (label, "launches per timer", launches)


ROUTES = {"a: one block": ("one_block", 0), "b: several-block mode": ("led", HINT), "c: generic kernel": ("led", 0)}
ITEM_SLOTS = 65536                   # of a several-block chunk (zhip_decompress_batch_device: the pool is at most the chunk maximum)


def _handed_on(route, n):
    return n if route.startswith("c") else 0


@pytest.mark.parametrize("route", list(ROUTES))
def test_sequence_families_on_three_routes(zstd, frame_sets, route):
    """the set once: every family, every frame, in one call of a fresh context"""
    which, hint = ROUTES[route]
    cases = getattr(frame_sets, which) + getattr(frame_sets, which + "_ck")
    assert len(cases) < _chunk_frames(hint)
    if hint: assert sum(len(c.blocks) for c in cases) <= max(6 * len(cases), min(12 * len(cases), ITEM_SLOTS))
    _run(route, cases, hint, 1, seed=len(cases) + hint, fallbacks=_handed_on(route, len(cases)))


@pytest.mark.parametrize("route", list(ROUTES))
def test_sequence_families_replicated_on_three_routes(zstd, frame_sets, route):
    """REPLICATED items in shuffled order with checksummed copies and ~1 % invalid frames: K0 in front of K1 (routes a and c), KX behind K3, K1b on
    the side stream; under the hint two pipeline chunks"""
    which, hint = ROUTES[route]
    cases = _replicated(getattr(frame_sets, which), getattr(frame_sets, which + "_ck"), REPLICATED, seed=hint + 5, few_blocks=bool(hint))
    chunk = _chunk_frames(hint)
    chunks = -(-REPLICATED // chunk)
    assert chunks == (2 if hint else 1)
    if hint:
        per_chunk = [sum(len(c.blocks) for c in cases[i:i + chunk]) for i in range(0, REPLICATED, chunk)]
        assert max(per_chunk) <= ITEM_SLOTS * 7 // 8, per_chunk
        assert sum(c.family == "repeat offsets" and len(c.blocks) > 6 for c in cases) >= REPLICATED // 16
    _run(route, cases, hint, chunks, seed=hint + 6, fallbacks=_handed_on(route, REPLICATED))


def test_ten_block_frame_under_its_own_hint(zstd, ref, oracle):
    """offsets of a mebibyte back to the frame's first byte, 51 extra bits in one sequence: a frame of ten blocks with slots for all of them, beside
    copies of itself, and without a hint (the generic kernel)"""
    cases = _judged(F.many_blocks(K3) * 3, ref, oracle)
    for hint in (max(len(c.want) for c in cases), 0):
        _run("ten blocks, hint %d" % hint, cases, hint, 1, seed=9, fallbacks=0 if hint else len(cases))


@pytest.mark.parametrize("route", list(ROUTES))
def test_dictionary_families(zstd, ref, oracle, route):
    """raw-content dictionary (sources wholly in it, ending at the frame's first byte, straddlers, the offset limit from both sides) and the small
    trained dictionary of tests/golden (frames that open with repeat codes), each in a context of its own, on the three routes: frames of one
    block, behind a raw block in the several-block mode, and the same without a hint (the generic kernel with a dictionary); with checksummed copies"""
    which, hint = ROUTES[route]
    d = open(TRAINED, "rb").read()
    assert struct.unpack("<3I", d[TRAINED_CONTENT_OFF - 12:TRAINED_CONTENT_OFF]) == TRAINED_REPS
    for cases, dict_type in ((F.raw_dictionaries(K3), 1), (trained_cases(K3), 0)):
        if which == "led": cases = [c.with_lead() for c in cases]
        cases = _judged(cases, ref, oracle)
        cases = cases + _judged(_with_checksums(cases), ref, oracle)
        _run("dictionary type %d, %s" % (dict_type, route), cases, hint, 1, seed=hint + dict_type, fallbacks=_handed_on(route, len(cases)),
             dict_data=cases[0].dict_data, dict_type=dict_type)
