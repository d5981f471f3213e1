"""K3's copies by literal mode under the wave emulator: tests/k3litmodes.py's cases through K1 -> K2 -> K3 (frames of one block), the several-block
mode (a raw block in front) and the generic kernel, judged by libzstd 1.5.7 first and held against seqmodel.execute (tests/test_emu_sequences.py's
run_routes). The families that aim at the batch loop's thresholds run in each of the three modes, with the census asserting that each mode's set
still reaches them; a frame changes the mode from block to block; one batch interleaves the modes; the raw-content dictionary family runs in the
modes it did not have; the K3 cases also run in the -DZP_ASM_BYTES=2048 build.

Mutations tried on a scratch copy of csrc/, each alone, under the emulator only, with the tests of this file that fail (the 2048-byte test builds its
library from the tree and was not part of it):
  1 the ARENA copy's long-literal unit source shifted by 16 (ZP_UNIT: `litPtr + L.srcL[j_] + off_` plus 16 where LM == ZP_LM_ARENA):
        families [huf], the frame that changes modes, the interleaved batch
  2 the long-RLE fill loop behind the staging block skipped (`if (litRLE) {` made `if (false && litRLE) {`):
        families [rle], the frame that changes modes, the interleaved batch
  3 the block-level dispatch sending blocks with decoded literals to the raw-literal copy. A treeless block's record does not differ from a Huffman
    block's, so the mutation takes, in the several-block mode, every block whose literals came in four streams (the frame of changing modes has its
    Huffman AND its treeless block so): `m.litMode != 0 && m.litMode != 2` and `&& !(MB && ((m.litMode >> 16) & 1))`:
        families [huf], the frame that changes modes, the interleaved batch
The dictionary tests fail under none of them: the dictionary instantiations run the one copy that has the mode as a run-time value."""
import pytest

from tests import k3litmodes as L
from tests import seqfamilies as F
from tests.seqmodel import K3, K3_SMALL
from tests.test_emu_sequences import run_routes


@pytest.fixture(scope="module")
def emu():
    from tests import emulib
    return emulib.Emu()


def _reached(done, k):
    reached = set()
    for c in done:
        if c.content is not None: reached |= c.census(k)
    return reached


def _missing(reached, families=L.FAMILIES):
    return {f: [e for e in F.REQUIRED[f] if e not in reached] for f in families if [e for e in F.REQUIRED[f] if e not in reached]}


@pytest.mark.parametrize("mode", L.MODES)
def test_threshold_families_in_every_literal_mode(emu, ref, oracle, mode):
    """far matches, near matches, batch shape and slot edges with their literals raw, Huffman-coded and RLE: three routes, and every limit the
    families name is still reached in that mode -- but for the one the RLE set cannot reach (RLE runs are no units)"""
    cases = L.family_cases(mode)
    assert len(cases) == 42
    assert [c.base_name for c in cases if not L.in_its_mode(c)] == (sorted(L.STAYS_RAW_IN_HUF) if mode == "huf" else [])
    done = run_routes(emu, cases, oracle, ref, mode + " literals")
    assert _missing(_reached(done, K3)) == (L.NOT_REACHED_IN_RLE if mode == "rle" else {})


def test_a_frame_that_changes_the_literal_mode_from_block_to_block(emu, ref, oracle):
    """Huffman (four streams), treeless, RLE, raw, behind a raw block: every block's first matches read the block before, every block slides its
    history. The several-block mode runs it in one wave, copy after copy; as it is it is the generic kernel's."""
    cases = L.changing_modes(K3)
    assert L.block_modes(cases[0]) == ["huf4", "treeless4", "rle", "raw"]
    done = run_routes(emu, cases, oracle, ref, "changing modes")
    reached = _reached(done, K3)
    need = ["slide", "far match: source below the history", "far match: source inside the history", "huf literals: 1..15", "rle literals: 1..15", "raw literals: 1..15"]
    assert [e for e in need if e not in reached] == []


def test_one_batch_with_the_modes_interleaved(emu, ref, oracle):
    """raw, Huffman, RLE, raw, ... frame by frame: a wave that takes the next frame runs another copy"""
    cases = L.interleaved(K3)
    assert [c.lit_mode for c in cases[:6]] == ["raw", "huf", "rle"] * 2
    run_routes(emu, cases, oracle, ref, "interleaved modes", generic=False)


@pytest.mark.parametrize("mode", ("huf", "rle"))
def test_raw_dictionary_family_in_the_other_literal_modes(emu, ref, oracle, mode):
    """the dictionary instantiations (one copy, the mode a run-time value) with Huffman and RLE literals: sources in the dictionary, straddlers"""
    cases = L.dictionary_cases(mode)
    assert all(L.in_its_mode(c) for c in cases if len(c.blocks[0][1]) > 1), [c.name for c in cases if not L.in_its_mode(c)]
    try:
        assert emu.set_ddict(cases[0].dict_data, raw_content=True) == 0
        done = run_routes(emu, cases, oracle, ref, "raw dictionary, %s literals" % mode, generic=False)
        outs, st = emu.decompress_batch([c.frame for c in done], [c.cap for c in done], n_blocks=2, dict_content=cases[0].dict_data)
    finally:
        emu.set_ddict(None)
    from tests.test_emu_sequences import check_answers
    check_answers("raw dictionary, %s literals: generic kernel" % mode, done, outs, st)
    reached = _reached(done, K3)
    assert [e for e in F.REQUIRED["raw dictionaries"] if e not in reached] == []


def test_literal_modes_with_a_2048_byte_assembly_buffer(oracle, ref, tmp_path):
    """the same sets, and the frame that changes modes, generated for and run in the -DZP_ASM_BYTES=2048 build"""
    from tests import emulib
    emu = emulib.Emu(emulib.build_variant(str(tmp_path / "libzhip_emu_asm2048.so"), ["-DZP_ASM_BYTES=2048"]))
    cases = [c for m in L.MODES for c in L.family_cases(m, K3_SMALL)] + L.changing_modes(K3_SMALL)
    done = run_routes(emu, cases, oracle, ref, "ZP_ASM_BYTES=2048", generic=False)
    need = ["history exactly at the slide mark", "slide 16 bytes past the mark", "after a slide: source in the kept region", "after a slide: source just outside it",
            "batch fills the room exactly", "first sequence left out is one byte above the room", "big item after a history", "units in a batch: 64"]
    for mode in L.MODES:
        reached = _reached([c for c in done if "[%s literals]" % mode in c.name], K3_SMALL)
        # (this build's only batch of 64 units is sixteen pairs of a 17-byte literal run and a 17-byte far match: with RLE literals it has 32)
        assert [e for e in need if e not in reached] == (["units in a batch: 64"] if mode == "rle" else []), mode
