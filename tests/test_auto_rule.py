"""The rule of match_finder="auto" (the numpy model tests/auto_model.py) judged AGAINST LIBZSTD'S TWO SIZES PER FRAME -- ZSTD_compress2 at level 3 and
ZSTD_compressSequences with the list that is only the block delimiter, through reflib.checker() -- never against the GPU code: that the kernel computes what the model
computes is the emulator's and the GPU suite's test. Frames of 131 072 bytes, 4 groups of 131 072 elements, numpy seed 1 (tests/tools/auto_finder_rule.py records the
regret per set, and the same on a second seed)."""
import pytest

from tests import auto_model as am
from tests import reflib


@pytest.fixture(scope="module")
def judged():
    """{set: [(literals-only size, search size, choice)]} -- libzstd's sizes and the model's choices, once for every test here"""
    ref = reflib.checker()
    return {name: [am.both_sizes(ref, f) + (am.classify(f)[0],) for f in frames] for name, frames in am.data_sets(1)}


def _totals(rows):
    none = sum(r[0] for r in rows); search = sum(r[1] for r in rows)
    auto = sum(r[0] if r[2] == am.LITERALS else r[1] for r in rows)
    return none, search, auto


def test_mixed_batch_is_below_both_pure_totals(judged):
    rows = judged["text"] + judged["bf16 planes"] + judged["int64 sums planes"]
    none, search, auto = _totals(rows)
    print("mixed batch: all none %d, all level 3 %d, auto %d" % (none, search, auto))
    assert auto < none and auto < search, (none, search, auto)


@pytest.mark.parametrize("name", ["text", "bf16 planes", "fp32 planes", "int64 sums planes", "int64 sums planes, delta", "uint32 sorted planes"])
def test_homogeneous_set_is_closer_to_the_better_finder(judged, name):
    """at most the midpoint of the two pure totals"""
    none, search, auto = _totals(judged[name])
    print("%s: all none %d, all level 3 %d, auto %d, best per frame %d" % (name, none, search, auto, sum(min(r[0], r[1]) for r in judged[name])))
    assert 2 * auto <= none + search, (name, none, search, auto)


def test_equal_sizes_choose_literals_only(judged):
    ties = [(name, i) for name, rows in judged.items() for i, r in enumerate(rows) if r[0] == r[1]]
    assert len(ties) >= 16                                                   # (the noise planes: raw either way)
    assert all(judged[name][i][2] == am.LITERALS for name, i in ties), [t for t in ties if judged[t[0]][t[1]][2] != am.LITERALS]
