"""The decode kernels driven by frames written from explicit sequences (tests/craft.py write_frame, tests/seqfamilies.py), under the wave emulator.

The suite's other decode tests take libzstd-made frames of corpus or random data, so a size or position threshold of K3 (zp_exec_block: ~thirty of
them) is reached only when an encoder happens to emit a sequence that lands on it. Here every family aims at its limits from both sides, and
seqmodel.census -- a restatement of K3's batching, used for coverage only -- must report each one as reached. The expected bytes are those of a
plain Python executor (seqmodel.execute); libzstd 1.5.7 is asked about every frame first, and a disagreement there is reported as a failure of
the test's model, not of a kernel. Every family runs through K1 -> K2 -> K3 (frames of one block), the several-block mode (a 1-byte raw block
in front of every frame, set_blocks), the generic kernel, and the C oracle; dictionary families under set_ddict; the K3 families also in the
-DZP_ASM_BYTES=2048 build. tests/stress_emu_sequences.py is the open-ended form; tests/test_gpu_sequences.py the same frames on the GPU.

Single-line mutations tried on a scratch copy, each alone, with the tests of this file that fail (and what failed before this file existed):
  1 zp_sym_resolve's `d` made `d ? 1 : 0`:           [repeat offsets]                                          (before: nothing)
  2 hOff not reset after a big item:                 [literal runs], [batch shape]                             (before: three tests)
  3 the slide copying ZP_HIST_KEEP without carry:    [far matches], [near matches], [batch shape], dictionary  (before: thirteen tests)
  4 `L.mEnd[...] <= a0` made `<= a0 + 1`:            [near matches], [batch shape], five more                  (before: twelve tests)
  5 the straddler loop skipped:                      the dictionary families                                   (before: one checksum test, through its dictionary frames)
  6 generic kernel, `myOF >= myML` made `myOF + 1 >= myML`:          [near matches], seven more                (before: six tests)
  7 generic kernel, `send <= op + Frel` made `<= op + Frel + 1`:     [near matches], four more                 (before: four tests)
  8 the doubling copy's `c > 32` cap removed:        nothing, and nothing can: that path serves matches of at most 32 bytes"""
import os
import re
import struct

import pytest

from tests import seqfamilies as F
from tests import seqmodel
from tests.seqmodel import K3, K3_SMALL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAINED = os.path.join(ROOT, "tests", "golden", "dict_json4k_16k.bin")
TRAINED_CONTENT_OFF, TRAINED_REPS = 119, (1, 4, 8)          # where the dictionary's content starts and the history it leaves (pinned below against the device parser)
# (this dictionary's stored history IS the format's default: frames that open with repeat codes show that a decoder reads the dictionary's content
# behind them -- code 1 reaches its last byte, 4 and 8 further in --, not that it takes the history from the dictionary rather than the defaults)
SLOTS = 16                                                   # item slots per frame in the several-block mode: every frame here but the ten-block one fits


@pytest.fixture(scope="module")
def emu():
    from tests import emulib
    return emulib.Emu()


def trained_cases(k=K3):
    d = open(TRAINED, "rb").read()
    cases = F.trained_dictionaries(d, TRAINED_CONTENT_OFF, TRAINED_REPS, k)
    for c in cases: c.header["dict_id"] = struct.unpack("<I", d[4:8])[0]
    return cases


def build_cases(cases, oracle, ref):
    """writes every frame and holds the model against libzstd (and the C oracle): the executor's bytes, or a refusal, from both"""
    for c in cases:
        c.build(oracle.xxh64)
        try:
            if not c.unjudged: seqmodel.check_model(ref, c.frame, c.want, c.cap, c.dict_data, c.raw_dict)
        except AssertionError as e:
            raise AssertionError("%s / %s: %s" % (c.family, c.name, e))
        try: got = oracle.decompress(c.frame, c.cap, c.dict_data)
        except RuntimeError: got = None
        assert got == c.want, (c.family, c.name, "the C oracle", c.why)
    return cases


def check_answers(label, cases, outs, st):
    """status 0 and the executor's bytes for every valid frame, a refusal for every other one (70 = dstSize_tooSmall for the slot that is too short).
    The emulator's harness lays the slots back to back without canaries: a refused frame that wrote past its slot shows here only through the
    bytes of the valid frame behind it (every family mixes them); "nothing outside the slot" proper is tests/test_gpu_sequences.py's, with canaries."""
    bad = []
    for c, o, s in zip(cases, outs, st):
        if c.want is None:
            if s == 0 or (c.short_by and s != 70): bad.append((c.family, c.name, "accepted / wrong status", s, c.why))
        elif s != 0: bad.append((c.family, c.name, "refused", s))
        elif o != c.want:
            first = next((i for i, (x, y) in enumerate(zip(o, c.want)) if x != y), min(len(o), len(c.want)))
            bad.append((c.family, c.name, "wrong bytes from", first, "of", len(c.want)))
    assert not bad, (label, len(bad), bad[:6])


def run_routes(emu, cases, oracle, ref, label, slots=SLOTS, generic=True):
    """`cases` through the pipeline as they are, behind a raw block in the several-block mode, and through the generic kernel"""
    build_cases(cases, oracle, ref)
    led = build_cases([c.with_lead() for c in cases], oracle, ref)
    one_block = [c for c in cases if len(c.blocks) == 1]
    try:
        emu.set_blocks(0)
        outs, st, nfb = emu.decompress_pipeline([c.frame for c in cases], [c.cap for c in cases], n_blocks=3, chunk=0)
        check_answers(label + ": pipeline", cases, outs, st)
        assert nfb == len(cases) - len(one_block), (label, "frames of one block handed to the generic kernel", nfb, len(cases), len(one_block))
        emu.set_blocks(slots)
        outs, st, nfb = emu.decompress_pipeline([c.frame for c in led], [c.cap for c in led], n_blocks=3, chunk=0)
        check_answers(label + ": several-block mode", led, outs, st)
        assert nfb == 0, (label, "several-block mode: frames handed to the generic kernel", nfb)
    finally:
        emu.set_blocks(0)
    if generic:
        outs, st = emu.decompress_batch([c.frame for c in led], [c.cap for c in led], n_blocks=2)
        check_answers(label + ": generic kernel", led, outs, st)
    return cases + led


def test_census_constants_match_the_kernel_headers():
    """seqmodel.K3Consts restates six constants of the decode kernels; when one changes, update seqmodel.K3 (and look at what the generators of
    tests/seqfamilies.py aim at)"""
    csrc = os.path.join(ROOT, "python-zstandard_amd", "csrc")
    gen = open(os.path.join(csrc, "zhip_decode_kernel.hpp")).read()
    pipe = open(os.path.join(csrc, "zhip_decode_pipeline.hpp")).read()

    def define(text, name):
        m = re.search(r"^#define %s[ \t]+(.+?)[ \t]*(//.*)?$" % name, text, re.M)
        assert m, "no #define %s: update tests/seqmodel.py" % name
        return m.group(1).strip()
    assert int(define(gen, "ZD_ASM_BYTES")) == K3.asm_bytes, "seqmodel.K3.asm_bytes"
    assert define(pipe, "ZP_ASM_BYTES") == "ZD_ASM_BYTES", "K3's buffer is no longer the generic kernel's: seqmodel.K3.asm_bytes"
    assert int(define(gen, "ZD_COOP_LEN")) == K3.coop_len, "seqmodel.K3.coop_len"
    assert int(define(pipe, "ZP_LIT_SHORT")) == K3.lit_short, "seqmodel.K3.lit_short"
    assert int(define(pipe, "ZP_FAR_SHORT")) == K3.far_short, "seqmodel.K3.far_short"
    assert define(pipe, "ZP_HIST_KEEP") == "((ZP_ASM_BYTES * 5u / 16u) & ~15u)", "seqmodel.K3Consts.hist_keep restates this formula"
    assert define(pipe, "ZP_HIST_SLIDE") == "(2u * ZP_HIST_KEEP + 16u)", "seqmodel.K3Consts.hist_slide restates this formula"
    assert "avail = nbSeq - done < 64 ? nbSeq - done : 64" in pipe, "seqmodel.K3.batch_seqs: a batch is no longer the next 64 sequences"
    assert (K3.hist_keep, K3.hist_slide, K3_SMALL.hist_keep, K3_SMALL.hist_slide) == (1280, 2576, 640, 1296)


def test_the_writer_leaves_the_pinned_frames_alone_and_reaches_every_code(ref, oracle):
    """craft.py's generalised writer: every LL / ML code and offset codes up to 28 on the predefined tables and in RLE mode, the three sequence-count
    forms, frames libzstd decodes to the executor's bytes; and sequences_block() -- pinned by golden/edge_frames.json -- agrees with it byte for byte"""
    import numpy as np
    from tests import craft
    rng = np.random.default_rng(31)
    old = craft.sequences_block(b"abcdefgh", [(8, 30, 5), (0, 3, 3), (0, 4, 2)])
    new = craft.block(2, craft.literals_section(b"abcdefgh") + craft.sequences_section([(8, 30, 5), (0, 3, 3), (0, 4, 2)]), True)
    assert old == new
    seen = [set(), set(), set()]
    cases = []
    for lc in range(36):
        for mc in (lc, 52 - lc, (lc * 7) % 53):
            ll = craft._LL_BASE[lc] + int(rng.integers(0, 1 << craft._LL_BITS[lc]))
            ml = craft._ML_BASE[mc] + int(rng.integers(0, 1 << craft._ML_BITS[mc]))
            if ll + ml + 40 > 131072: ll, ml = (ll, 3 + lc) if lc > 30 else (lc, ml)
            blocks = [("raw", bytes(rng.integers(0, 256, 40, dtype=np.uint8)))]
            b = F.Builder(rng, 40).seq(ll, ml, int(rng.integers(1, 41))).seq(3, 4, 9)
            blocks.append(b.block(rest=lc % 2))
            for q in b.seqs:
                for k, c in enumerate(craft.seq_codes(*q)): seen[k].add(c[0])
            cases.append(F.Case("writer", "LL code %d, ML code %d" % (lc, mc), blocks, header={"window_log": 18}))
    for oc in range(2, 29):                                    # offset codes: valid behind 2^oc bytes of RLE blocks up to 1 MiB, above that refused (the frame is too small)
        ofv = (1 << oc) + 1 + oc % 2
        seen[1].add(craft.seq_codes(4, 3, ofv)[1][0])
        fill = [("rle", oc, min(1 << oc, 131072))] * max(1, (1 << oc) >> 17) if oc <= 20 else []
        cases.append(F.Case("writer", "offset code %d" % oc, fill + [("seq", b"abcd", [(4, 3, ofv)], {"modes": (0, oc % 2, 0)})], header={"claims": 7, "window_log": 21}))
        assert (cases[-1].build(oracle.xxh64).want is not None) == (oc <= 20)
    assert seen[0] == set(range(36)) and seen[2] == set(range(53)) and seen[1] >= set(range(2, 29)), seen
    build_cases(cases, oracle, ref)


FAMILIES = {
    "literal runs": F.literal_runs, "far matches": F.far_matches, "near matches": F.near_matches, "batch shape": F.batch_shapes,
    "slot edges": F.slot_edges, "extremes": F.extremes, "repeat offsets": F.repeat_offsets, "invalid frames": F.invalid_frames, "header forms": F.header_forms,
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_sequence_families_through_the_emulated_kernels(emu, ref, oracle, family):
    """one family: K1 -> K2 -> K3, the several-block mode, the generic kernel, the C oracle; the census must list every limit the family names"""
    done = run_routes(emu, FAMILIES[family](K3), oracle, ref, family)
    reached = set()
    for c in done:
        if c.content is not None: reached |= c.census(K3)
    missing = [e for e in F.REQUIRED.get(family, []) if e not in reached]
    assert not missing, (family, "limits the generators no longer reach", missing)
    if family == "invalid frames":
        assert {c.why for c in done if c.want is None} == F.INVALID_REASONS


def test_the_three_byte_sequence_count(emu, ref, oracle):
    """a block of 32 512 sequences: libzstd, the oracle and K1 -> K2 -> K3 (half a minute per route under the emulator: the other routes are
    tests/stress_emu_sequences.py's and the GPU's)"""
    cases = build_cases(F.header_forms(K3, longest=True), oracle, ref)
    outs, st, nfb = emu.decompress_pipeline([c.frame for c in cases], [c.cap for c in cases], n_blocks=2, chunk=0)
    check_answers("pipeline", cases, outs, st)
    assert nfb == 0


def test_ten_block_frame_with_offsets_of_a_mebibyte(emu, ref, oracle):
    """offsets above 128 KiB back to the frame's first byte and 51 extra bits in one sequence, in a frame of ten blocks: the several-block mode with
    slots for all of them, and the generic kernel"""
    cases = build_cases(F.many_blocks(K3), oracle, ref)
    try:
        emu.set_blocks(12)
        outs, st, nfb = emu.decompress_pipeline([c.frame for c in cases], [c.cap for c in cases], n_blocks=2, chunk=0)
    finally:
        emu.set_blocks(0)
    check_answers("several-block mode", cases, outs, st)
    assert nfb == 0
    outs, st = emu.decompress_batch([c.frame for c in cases], [c.cap for c in cases], n_blocks=2)
    check_answers("generic kernel", cases, outs, st)
    reached = set().union(*[c.census(K3) for c in cases])
    assert not [e for e in F.REQUIRED["many blocks"] if e not in reached]


def test_dictionary_families_through_the_emulated_kernels(emu, ref, oracle):
    """raw-content dictionary: sources wholly inside it, ending at the frame's first byte, straddlers, the offset limit from both sides; the small
    trained dictionary of tests/golden: frames that open with repeat codes. Under set_ddict, in both pipeline modes, and the generic kernel."""
    raw = F.raw_dictionaries(K3)
    d = open(TRAINED, "rb").read()
    blob, content, dict_id = emu.parse_dict(d)
    assert len(d) - len(content) == TRAINED_CONTENT_OFF and struct.unpack("<3I", d[TRAINED_CONTENT_OFF - 12:TRAINED_CONTENT_OFF]) == TRAINED_REPS
    reached = set()
    try:
        for cases, raw_content in ((raw, True), (trained_cases(K3), False)):
            assert emu.set_ddict(cases[0].dict_data, raw_content=raw_content) == 0
            done = run_routes(emu, cases, oracle, ref, "raw dictionary" if raw_content else "trained dictionary", generic=False)
            for c in done:
                if c.content is not None: reached |= c.census(K3)
            if raw_content: outs, st = emu.decompress_batch([c.frame for c in done], [c.cap for c in done], n_blocks=2, dict_content=cases[0].dict_data)
            else: outs, st = emu.decompress_batch([c.frame for c in done], [c.cap for c in done], n_blocks=2, dict_content=content, dict_id=dict_id, dict_entropy=blob)
            check_answers(("raw" if raw_content else "trained") + " dictionary: generic kernel", done, outs, st)
    finally:
        emu.set_ddict(None)
    missing = [e for e in F.REQUIRED["raw dictionaries"] if e not in reached]
    assert not missing, missing


def test_k3_families_with_a_2048_byte_assembly_buffer(oracle, ref, tmp_path):
    """the K3 families generated for, and run in, the -DZP_ASM_BYTES=2048 build (test_emu_kernels.py::test_decode_shape_variants_stay_correct's third
    shape): room, history and slide marks at half their size"""
    from tests import emulib
    emu = emulib.Emu(emulib.build_variant(str(tmp_path / "libzhip_emu_asm2048.so"), ["-DZP_ASM_BYTES=2048"]))
    done = run_routes(emu, F.k3_families(K3_SMALL), oracle, ref, "ZP_ASM_BYTES=2048", generic=False)
    reached = set()
    for c in done:
        if c.content is not None: reached |= c.census(K3_SMALL)
    need = ["history exactly at the slide mark", "slide 16 bytes past the mark", "after a slide: source in the kept region", "after a slide: source just outside it",
            "batch fills the room exactly", "first sequence left out is one byte above the room", "big item after a history", "units in a batch: 64"]
    assert not [e for e in need if e not in reached], [e for e in need if e not in reached]


def test_census_reaches_every_named_limit():
    """the union over all families, each frame as it is and behind a raw block: every event of tests/seqfamilies.py REQUIRED"""
    reached = set()
    for c in F.k3_families(K3) + F.raw_dictionaries(K3) + F.extremes(K3) + F.many_blocks(K3) + F.repeat_offsets(K3):
        for x in (c, c.with_lead()):
            try: seqmodel.execute(x.blocks, x.dict_content(), x.start_reps)
            except seqmodel.Invalid: continue
            reached |= x.census(K3)
    required = sorted({e for v in F.REQUIRED.values() for e in v})
    assert [e for e in required if e not in reached] == []
