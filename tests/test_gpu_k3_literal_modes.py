"""K3's copies by literal mode on the MI355X: tests/k3litmodes.py's cases through the device API, as tests/test_gpu_sequences.py runs its families.

The families that aim at the batch loop's thresholds (far matches, near matches, batch shape, slot edges) with raw, Huffman-coded and RLE literals,
the frame that changes the mode from block to block, and the three modes interleaved frame by frame in one batch, on the three routes -- (a) frames
of one block, (b) a raw block in front under the hint of 131 073 (the several-block mode), (c) the same without a hint (the generic kernel, for
comparison) --; the raw-content dictionary family with Huffman and RLE literals for the dictionary instantiations. libzstd 1.5.7 judges every frame
first; the route is proved by DeviceBatchContext.decode_fallbacks; layout with gaps and canaries, every frame answered (test_gpu_launch_shapes.py's
_decode / _check_decode through test_gpu_sequences.py's _run). The sets run once per route: a few hundred frames, the largest of 128 KiB."""
import pytest

from tests import k3litmodes as L
from tests import seqfamilies as F
from tests.seqmodel import K3
from tests.test_gpu_launch_shapes import zstd  # noqa: F401  (the module fixture)
from tests.test_gpu_sequences import HINT, ROUTES, _handed_on, _judged, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mode_sets(ref, oracle):
    """the three modes' sets interleaved (raw, huf, rle, raw, ...) and the frame of changing modes: as they are, and behind a raw block"""
    cases = L.interleaved(K3) + L.changing_modes(K3)
    assert len(cases) == 3 * 42 + 1 and max(len(c.build(oracle.xxh64).content or b"") for c in cases) <= 131072
    return {"one_block": _judged([c for c in cases if len(c.blocks) == 1], ref, oracle), "led": _judged([c.with_lead() for c in cases], ref, oracle)}


@pytest.mark.parametrize("route", list(ROUTES))
def test_literal_modes_interleaved_on_three_routes(zstd, mode_sets, route):
    """one batch per route: neighbouring frames take different copies of the block code, and on route (b) the frame of four compressed blocks
    changes the copy inside one wave"""
    which, hint = ROUTES[route]
    cases = mode_sets[which]
    if hint: assert sum(len(c.blocks) for c in cases) <= 6 * len(cases)              # (the chunk's pool of item slots: six per frame under this hint)
    modes = {m for c in cases for m in L.block_modes(c)}
    assert modes >= {"raw", "huf1", "huf4", "rle"} and (which == "one_block" or "treeless4" in modes)
    _run("literal modes, " + route, cases, hint, 1, seed=len(cases) + hint, fallbacks=_handed_on(route, len(cases)))


@pytest.mark.parametrize("mode", L.MODES)
def test_each_literal_mode_alone_in_the_pipeline(zstd, ref, oracle, mode):
    """a batch of one mode: every wave stays in one copy (routes a and b)"""
    cases = L.family_cases(mode)
    one = _judged([c for c in cases if len(c.blocks) == 1], ref, oracle)
    _run("%s literals, one block" % mode, one, 0, 1, seed=7, fallbacks=0)
    led = _judged([c.with_lead() for c in cases], ref, oracle)
    _run("%s literals, several-block mode" % mode, led, HINT, 1, seed=8, fallbacks=0)


@pytest.mark.parametrize("mode", ("huf", "rle"))
def test_raw_dictionary_family_in_the_other_literal_modes(zstd, ref, oracle, mode):
    """the dictionary instantiations (plain and several-block) with Huffman and RLE literals, and the generic kernel with a dictionary"""
    for route, (which, hint) in ROUTES.items():
        cases = L.dictionary_cases(mode)
        if which == "led": cases = [c.with_lead() for c in cases]
        cases = _judged(cases, ref, oracle)
        _run("raw dictionary, %s literals, %s" % (mode, route), cases, hint, 1, seed=hint + 3, fallbacks=_handed_on(route, len(cases)),
             dict_data=cases[0].dict_data, dict_type=1)
