"""The sequence kernel's step (zp_seqq_body) under the wave emulator, driven by tests/k2steps.py's frames: the case lists of
tests/test_gpu_k2_steps.py, so that a slip in the step's LOGIC -- the select tree of the repeat offsets, the ring's upkeep, which every lane does
on every trip whether it has a block to take or not -- shows here before it reaches a GPU. (What only the hardware can show -- a DPP or VCC
wait state -- is the GPU file's.) Every frame runs as it is (zhip_decode_seq_kernel) and behind a 1-byte raw block in the several-block mode
(zhip_decode_seq_mb_kernel); libzstd and the C oracle judge every frame first."""
import pytest

from tests import k2steps as S
from tests.test_emu_sequences import SLOTS, build_cases, check_answers

FAMILIES = {"counts": S.counts, "table modes": S.table_modes, "wide fields": S.wide_fields, "selects": S.selects, "ring edges": S.ring_edges,
            "damaged": S.damaged, "repeat offsets": S.F.repeat_offsets, "invalid frames": S.F.invalid_frames}


@pytest.fixture(scope="module")
def emu():
    from tests import emulib
    return emulib.Emu()


def both_kernels(emu, cases, oracle, ref, label):
    build_cases(cases, oracle, ref)
    led = build_cases([c.with_lead() for c in cases], oracle, ref)
    one_block = [c for c in cases if len(c.blocks) == 1]
    try:
        emu.set_blocks(0)
        outs, st, nfb = emu.decompress_pipeline([c.frame for c in cases], [c.cap for c in cases], n_blocks=3, chunk=0)
        check_answers(label + ": frames of one block", cases, outs, st)
        assert nfb == len(cases) - len(one_block), (label, "frames handed to the generic kernel", nfb)
        emu.set_blocks(SLOTS)
        outs, st, nfb = emu.decompress_pipeline([c.frame for c in led], [c.cap for c in led], n_blocks=3, chunk=0)
        check_answers(label + ": several-block mode", led, outs, st)
        assert nfb == 0, (label, "several-block mode: frames handed to the generic kernel", nfb)
    finally:
        emu.set_blocks(0)
    return cases


@pytest.mark.parametrize("family", list(FAMILIES))
def test_step_families_through_both_sequence_kernels(emu, ref, oracle, family):
    cases = both_kernels(emu, FAMILIES[family](), oracle, ref, family)
    if family == "counts":
        assert [len(c.blocks[0][2]) for c in cases] == list(S.COUNTS)
    if family == "ring edges":
        sizes = [c.stream_bytes[0] for c in cases]
        assert sizes[:len(S.STREAM_BYTES)] == list(S.STREAM_BYTES)
        assert {n % 16 for n in sizes} == set(range(16)) and max(sizes) > 256, sorted(sizes)
    if family == "selects":
        assert sum(c.want is not None for c in cases) >= 2 and any(c.why == "repeat offset 1 minus one is zero" for c in cases), [c.why for c in cases]
    if family == "damaged":
        assert all(c.want is None for c in cases)


@pytest.mark.parametrize("frames", S.BATCHES)
def test_batches_of_mixed_sequence_counts(emu, ref, oracle, frames):
    """1, 14, 15, 16 and 31 frames: part of a group of fifteen, a whole one, a second group of one; every group mixes sequence counts"""
    cases = S.batch_of(frames)
    assert len(cases) == frames and len({len(c.blocks[0][2]) for c in cases}) >= min(frames, 8)
    both_kernels(emu, cases, oracle, ref, "%d frames" % frames)
