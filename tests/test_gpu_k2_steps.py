"""The sequence kernel's step (zp_seqq_body) on the MI355X, driven by tests/k2steps.py's frames -- tests/test_emu_k2_steps.py's case lists through
the device API, compared byte for byte and status for status with what libzstd 1.5.7 says about every frame.

The emulator computes every lane of every instruction and cannot see a wait state: a cross-lane (DPP) read too close behind the write of its
source, or a select too close behind the compare that feeds it, shows only here (is one that did). The cases: 1 ... 9, 63,
64 and 65 sequences (the trip count modulo the unrolled four; a one-sequence frame runs exactly two trips); batches of 1, 14, 15, 16 and 31
frames of mixed counts (lanes run past their frame's end beside neighbours that go on); every combination of predefined, one-cell and
compressed tables at the smallest and largest logs; the widest fields a 128 KiB frame can carry; every arm of the repeat-offset selects behind
every other; streams of 1 ... 17 bytes and of every size modulo the ring's blocks; damaged streams. Each set runs as frames of one block
(zhip_decode_seq_kernel) and, behind a raw block under a size hint, in the several-block mode (zhip_decode_seq_mb_kernel); the pipeline's own
count of frames handed to the generic kernel must be 0, so it is K2 that answered."""
import pytest

from tests import k2steps as S
from tests.test_gpu_launch_shapes import zstd  # noqa: F401  (the module fixture)
from tests.test_gpu_sequences import HINT, _judged, _run

pytestmark = pytest.mark.gpu

ROUTES = {"one block": 0, "several-block mode": HINT}


@pytest.fixture(scope="module")
def step_sets(ref, oracle):
    """the families as frames of one block and behind a raw block, each judged by libzstd once; seqfamilies' repeat offsets are frames of
    several blocks and run in the several-block mode only"""
    own = S.counts() + S.table_modes() + S.wide_fields() + S.selects() + S.ring_edges() + S.damaged()
    other = S.F.repeat_offsets() + S.F.invalid_frames()
    plain = own + [c for c in other if len(c.blocks) == 1]
    return {0: _judged(plain, ref, oracle), HINT: _judged([c.with_lead() for c in own + other], ref, oracle)}


@pytest.mark.parametrize("route", list(ROUTES))
def test_step_families_on_both_sequence_kernels(zstd, step_sets, route):
    hint = ROUTES[route]
    cases = step_sets[hint]
    assert sum(c.want is None for c in cases) >= 12
    _run(route, cases, hint, 1, seed=3 + hint, fallbacks=0)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("frames", S.BATCHES)
def test_batches_of_mixed_sequence_counts(zstd, ref, oracle, frames, route):
    """1, 14, 15, 16 and 31 frames, each batch in a fresh context: part of a group of fifteen, a whole one, a second group of one"""
    hint = ROUTES[route]
    cases = S.batch_of(frames)
    if hint: cases = [c.with_lead() for c in cases]
    _run("%d frames, %s" % (frames, route), _judged(cases, ref, oracle), hint, 1, seed=frames + hint, fallbacks=0)
