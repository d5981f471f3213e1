"""The sequence decoders on the MI355X, driven by explicit FSE distributions: tests/test_emu_sequence_tables.py's families through the device API.

Every frame carries tables given as distributions, or "repeat"s of a chosen predecessor (tests/fsefamilies.py, written by tests/craft.py), and is
expected to decode to what the plain model of tests/fsemodel.py computes from the frame's own bytes, or to be refused where the model refuses; libzstd
1.5.7 is asked about every frame first and must give the same verdict and bytes -- there is no stricter class here. Nothing reads more than
tests/golden and oracle/_ref. The routes are test_gpu_sequences.py's, each in a fresh context and each proved by the pipeline's count of the frames it
handed to the generic kernel (decode_fallbacks):

  (a) the frames of one block, no hint:          K1 -> K2 -> K3 (0 handed on);
  (b) a 1-byte raw block in front, hint 131 073: the several-block mode -- a later block's "repeat" takes the previous block's tables inside K1 (handed
      on: only the frames whose offsets K2 cannot pack, [alphabets]' offset codes 29 .. 31);
  (c) the frames of (b), no hint:                K1 lists every one for the generic kernel (all handed on).

The set runs once on each route with every frame laid out by its pad_for -- the bit-rate family's heaviest four steps (277 bits) then lie with their
stream's first byte at every offset 0 .. 15 mod 16, asserted from the census at the frames' places --, then the dictionary family (the trained dictionary of tests/golden, and its bytes as raw content), then the K2 groups (and the same sizes under the dictionary: shared-table frames beside described ones),
then about 12 000 shuffled items on (a) and (b) -- above K0's 6 144 frames, so K0 parses the distributions K1 takes -- with ~1 % refused frames, one at
the last index, and every fifth frame carrying a content checksum. Layout and checks are test_gpu_launch_shapes.py's: slots of exactly the content size
at odd offsets in shuffled order, canaries between them, status -1 and a size sentinel before the call."""
import numpy as np
import pytest

from tests import fsefamilies as X
from tests.seqmodel import check_model
from tests.test_emu_sequences import TRAINED, TRAINED_CONTENT_OFF, TRAINED_REPS
from tests.test_gpu_launch_shapes import _chunk_frames, zstd  # noqa: F401  (zstd: the module fixture)
from tests.test_gpu_huffman_tables import _run as _run_placed          # (lays every frame out by its pad_for and returns the frames' offsets)
from tests.test_gpu_sequences import ITEM_SLOTS, REPLICATED, ROUTES, _handed_on, _run

pytestmark = pytest.mark.gpu

OF_LIMIT = 0x1E000000                # ZP_OF_LIMIT: offsets K2 cannot pack (the several-block mode hands such a frame to the generic kernel)


def _judged(cases, ref, oracle):
    for c in cases:
        c.build(oracle.xxh64)
        try: check_model(ref, c.frame, c.want, c.cap, c.dict_data, c.raw_dict)
        except AssertionError as e: raise AssertionError("%s / %s (%s): %s" % (c.family, c.name, c.why, e))
    return cases


def _checksummed(c):
    k = X.FseCase(c.family, c.name + " [checksum]", c.blocks, dict_data=c.dict_data, raw_dict=c.raw_dict, checksum="right", start_reps=c.start_reps, header=dict(c.header))
    if c.dict_data and not c.raw_dict: k.content_off = c.content_off
    return k


def _unpacked(cases):
    return sum(any(q[2] >= OF_LIMIT for b in c.blocks if b[0] == "seq" for q in b[2]) for c in cases)


class _Set:
    pass


@pytest.fixture(scope="module")
def frame_sets(ref, oracle):
    """the families as the frames of one block among them (route a) and every frame behind a raw block (routes b and c), each judged by libzstd once;
    and a checksummed copy of every valid one"""
    s = _Set()
    cases = [c for gen in X.FAMILIES.values() for c in gen()]
    s.one_block = _judged([c for c in cases if len(c.blocks) == 1], ref, oracle)
    s.led = _judged([c.with_lead() for c in cases], ref, oracle)
    s.one_block_ck = _judged([_checksummed(c) for c in s.one_block if c.want is not None], ref, oracle)
    s.led_ck = _judged([_checksummed(c) for c in s.led if c.want is not None], ref, oracle)
    assert all(c.want is not None for c in s.one_block_ck + s.led_ck)
    return s


def _fallbacks(route, cases):
    return _handed_on(route, len(cases)) or (_unpacked(cases) if route.startswith("b") else 0)


@pytest.mark.parametrize("route", list(ROUTES))
def test_sequence_table_families_on_three_routes(zstd, frame_sets, route):
    """the set once: every family, every frame the route takes, in one call of a fresh context"""
    which, hint = ROUTES[route]
    cases = getattr(frame_sets, which)
    assert 200 < len(cases) < _chunk_frames(hint)
    if hint: assert sum(len(c.blocks) for c in cases) <= min(6 * len(cases), ITEM_SLOTS)
    soffs = _run_placed(route, cases, hint, 1, seed=len(cases) + hint, fallbacks=_fallbacks(route, cases))
    # the bit-rate family's heaviest four steps lie where their stream's first byte is at every offset 0 .. 15 mod 16 (device allocations are aligned far above 16)
    reached = set()
    for c, o in zip(cases, soffs):
        if c.family == "bit rate": reached |= c.fse_census(int(o))
    wanted = [e for e in X.REQUIRED["bit rate"] if "mod 16" in e]                                # (the heaviest window's frames have one block: route (a) takes them too)
    missing = [e for e in wanted if e not in reached]
    assert len(wanted) == 16 and not missing, missing


@pytest.mark.parametrize("route", list(ROUTES))
def test_dictionary_families(zstd, ref, oracle, route):
    """the trained dictionary of tests/golden, a context of its own: every table "repeat" (the shared copy), one and two of three beside described /
    RLE / predefined ones, block 1 described and block 2 "repeat", repeat / described / repeat; and its bytes as a raw-content dictionary, under which a
    first block's "repeat" is refused"""
    which, hint = ROUTES[route]
    trained = open(TRAINED, "rb").read()
    for name, cases in X.dictionary_frames(trained, TRAINED_CONTENT_OFF, TRAINED_REPS):
        raw = name == "raw content"
        if which == "led": cases = [c.with_lead() for c in cases]
        else: cases = [c for c in cases if len(c.blocks) == 1]
        cases = _judged(cases, ref, oracle)
        assert any(c.want is None for c in cases) == raw
        _run("dictionary, %s, %s" % (name, route), cases, hint, 1, seed=hint + len(name), fallbacks=_fallbacks(route, cases), dict_data=cases[0].dict_data, dict_type=1 if raw else 0)


def test_k2_groups_with_refused_neighbours(zstd, ref, oracle):
    """1 / 14 / 15 / 16 / 31 frames of one block with different logs per frame (5 / 5 / 5 beside 9 / 8 / 9, single-symbol and predefined tables), every
    fifth refused for a log above its kind's maximum: one frame's logs must not leak into its neighbours of a K2 wave"""
    for name, cases in X.k2_groups():
        _judged(cases, ref, oracle)
        assert sum(c.want is None for c in cases) == len(cases) // 5
        _run("K2 groups: " + name, cases, 0, 1, seed=len(cases), fallbacks=0)


def test_k2_groups_under_a_dictionary(zstd, ref, oracle):
    """the same sizes in a context with the trained dictionary: frames whose tables are all the dictionary's (K2 copies the one shared set) beside frames
    with tables of their own, one and two of three "repeat", and refused ones"""
    trained = open(TRAINED, "rb").read()
    for name, cases in X.k2_dictionary_groups(trained, TRAINED_CONTENT_OFF, TRAINED_REPS):
        _judged(cases, ref, oracle)
        assert sum(c.want is None for c in cases) == len(cases) // 5
        _run("K2 dictionary groups: " + name, cases, 0, 1, seed=len(cases), fallbacks=0, dict_data=trained, dict_type=0)


def _replicated(cases, checksummed, n, seed):
    """n items: the valid frames over and over in shuffled order, every fifth place a checksummed copy, ~1 % of the places given to frames that must
    be refused, one of them at the last index (the frames above 70 000 bytes of content run in the single set only)"""
    rng = np.random.default_rng(seed)
    good = [c for c in cases if c.want is not None and len(c.want) <= 70000]
    ck = [c for c in checksummed if len(c.want) <= 70000]
    bad = [c for c in cases if c.want is None]
    assert len(bad) >= 8
    picks = [good[i] for i in rng.integers(0, len(good), n)]
    for i in range(0, n, 5): picks[i] = ck[int(rng.integers(0, len(ck)))]
    for i in list(rng.choice(n - 1, n // 100, replace=False)) + [n - 1]:
        picks[int(i)] = bad[int(rng.integers(0, len(bad)))]
    return picks


@pytest.mark.parametrize("route", ["a: one block", "b: several-block mode"])
def test_sequence_table_families_replicated(zstd, frame_sets, route):
    """REPLICATED items in shuffled order, refused ones mixed in at ~1 %, every fifth checksummed: K0 in front of K1 on route (a), K2's waves mixing
    logs 5 .. 9 and single-symbol tables, the frames laid out by their alignments; under the hint two pipeline chunks"""
    which, hint = ROUTES[route]
    cases = _replicated(getattr(frame_sets, which), getattr(frame_sets, which + "_ck"), REPLICATED, seed=hint + 21)
    chunk = _chunk_frames(hint)
    chunks = -(-REPLICATED // chunk)
    assert chunks == (2 if hint else 1)
    if hint: assert max(sum(len(c.blocks) for c in cases[i:i + chunk]) for i in range(0, REPLICATED, chunk)) <= ITEM_SLOTS * 7 // 8
    assert cases[-1].want is None and len({c.name for c in cases}) > 150
    _run_placed(route + ", replicated", cases, hint, chunks, seed=hint + 22, fallbacks=_fallbacks(route, cases))
