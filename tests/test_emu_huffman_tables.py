"""The Huffman literal decoders driven by EXPLICIT code tables (tests/craft.py HufTable.from_weights, tests/huffamilies.py), under the wave emulator.

The decode side of the Huffman code -- zd_read_huf_weights, zd_build_huf, zd_huf_stream (zhip_decode_kernel.hpp); K0's zp_pre_weights, K1's hand-over
(ZdLitDefer) and K1b's zb_init / zp_huf_stream / zp_huf_body (zhip_decode_pipeline.hpp) -- otherwise sees the tables libzstd's encoder emits (at most
11 bits deep, shaped by the corpus) and craft.HufTable's natural trees (symbols up to 128, direct weights). Here a table is a weight list, its
description a chosen form, its section a chosen layout; every family of tests/huffamilies.py sits on both sides of its limit and hufmodel.census
must report each limit as reached (huffamilies.REQUIRED). The expected value is tests/hufmodel.py's -- a plain description parser, table builder and
backward stream decoder -- held against libzstd 1.5.7 first: a disagreement is reported as the model's fault, and the one class where the model may
refuse what libzstd decodes ("a stream not consumed exactly") is allowed only in the damaged-stream family (the K1b groups'
damaged members are refused by libzstd too, and must be).

Routes: the pipeline as frames of one block with K0 and without it, the several-block mode (a raw block in front), the generic kernel, the C oracle;
the dictionary families under set_ddict on all of them. The emulator's hooks prove the routes: zd_stat[10] (weights taken from K0's record), [4]
(Huffman streams decoded inside K1: the table too deep for K1b's slots), [5] (treeless blocks rebuilt from the weights in LDS), [6] (frames that met a
dictionary table too deep to share) -- each nonzero exactly where a family aims at it.

WHAT THIS FOUND. libzstd refuses FSE-compressed weights whose distribution has accuracy log 6 AND names weight 12 (its work area for that decode is
sized for log 6 and the weights 0 .. 11: FSE_decompress_wksp_body's tableLog_tooLarge); the kernels, K0 and the C oracle's parser decoded such a
description. All three now refuse it (zd_weights_dist_ok); [FSE descriptions] holds the case on both sides (log 5 with weight 12 decodes).

Single-token mutations tried on a scratch copy of the headers, each alone, CPU only, with the tests of this file that fail (before this file: what failed in
the rest of the CPU suite's decode tests, test_emu_kernels.py and test_emu_sequences.py):
   1 `(nOnes & 1)` dropped (zd_read_huf_weights):      nothing, and nothing can: once the rest is a power of two the total 2^log is even and so is the sum over the
                                                       weights of 2 and up, hence the number of weights of 1; the test is implied by the one before it   (before: nothing)
   2 `log > 12` made `> 11`:                           [depth], [alphabet], [FSE descriptions], [refused tables], [streams], [inheritance], dictionaries  (before: nothing)
   3 `lg <= defer->maxLog` made `<`:                   [depth], [alphabet], [FSE descriptions], [streams], [damaged streams], [inheritance] -- by hook [4]'s exact
                                                       count: the bytes stay right, log-11 tables are decoded inside K1                                  (before: nothing)
   4 `cnt > 253` made `> 254`, K1 / K0 (each alone):   [alphabet], the list one weight too long                                                          (before: nothing / nothing)
   5 the weight at an over-read exit dropped, K0 only,
     first / second exit (each alone):                 [alphabet], [FSE descriptions]                                    (before: five tests of test_emu_kernels.py, each)
   6 `hb < 2` accepted:                                nothing, and nothing can: a description of 0 or 1 bytes cannot hold a distribution (4 + 6 bits at least) and
                                                       zd_read_ncount refuses it; [FSE descriptions] holds size bytes 0, 1 and 2                         (before: nothing)
   7 `i + 8 <= count` made `<` (zp_huf_stream):        nothing, and nothing can: a count that is a multiple of 8 then leaves its last 8 symbols to the tail loop, which
                                                       decodes them one by one behind the same burst -- the same bits, the same bytes; only the last store differs in
                                                       width ([streams] runs every tail 0 .. 7 at 1 .. 17 and 63 .. 65 literals)                         (before: nothing)
   8 `B.used` off by one (zb_init):                    every family, K1b groups, dictionaries                                                            (before: eight tests)
   9 `6 + s1 + s2 + s3 > streamBytes` made `>=`, K1b,
     and the same line in zd_literals (each alone):    nothing, and nothing can: at equality the fourth stream has no byte and zb_init / zd_pb_init refuse it;
                                                       [damaged streams] holds the jump table one past the section and the one that equals it           (before: nothing)
  10 `seg = (litSize + 3) / 4` made `litSize / 4`:     [depth], [alphabet], [FSE descriptions], [refused tables], [streams], [inheritance], dictionaries  (before: eight tests)
  11 `else { prevTable = nullptr; ... }` removed:      [inheritance]                                                                                     (before: nothing)
  12 zp_lit_shared_try's `hufLog > ZP_HUF_LOGMAX`
     guard removed:                                    the dictionary tables of log 12                                                                   (before: nothing)
  13 the direct form's nibble order swapped:           [depth], [alphabet], [refused tables], [streams], [damaged streams], [inheritance], K1b groups,
                                                       dictionaries                                  (before: three tests of test_emu_kernels.py, [literal runs])
  14 the fix taken back (log 6 naming weight 12
     decoded), K1 / K0 (each alone):                   [FSE descriptions]                                                                                (before: nothing / nothing)
"before" is the earlier decode tests: test_emu_sequences.py (but its variant build and the 32 512-sequence block) and the ten decode tests of test_emu_kernels.py
that take frames through the generic kernel and the pipeline (golden frames, oracle parity, varied frames, dictionaries, damaged frames, frames no encoder writes,
several blocks, the K0 / K1 lane passes).

WHAT IS LEFT STRICTER. K1 refuses a weights distribution that NAMES a symbol above 12 even where no weight uses it; libzstd decodes one at accuracy log 5 (its
work area holds symbols up to 91). That refusal is what keeps every FSE-decoded weight at 12 or below, which zd_read_huf_weights' sum and zd_build_huf's shifts
rely on: [FSE descriptions] holds four and eight weights of 33 .. 44, each in a lane of its own, which a decoder that let them through would add up to a
power of two again. No encoder writes such a distribution; the families keep to the case the format's users can meet, weight 13 in use (refused by all)."""
import os
import re

import pytest

from tests import huffamilies as H
from tests import hufmodel
from tests.test_emu_sequences import SLOTS, TRAINED, TRAINED_CONTENT_OFF, check_answers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOK_K0, HOOK_DEEP, HOOK_REBUILT, HOOK_DICT_DEEP = 10, 4, 5, 6


@pytest.fixture(scope="module")
def emu():
    from tests import emulib
    return emulib.Emu()


def judged(cases, oracle, ref):
    """writes every frame; the model's verdict against libzstd's (stricter only in the damaged-stream family, only for inexact consumption) and the
    C oracle's. Returns how many frames fell into the stricter class."""
    stricter = 0
    for c in cases:
        c.build(oracle.xxh64)
        try: stricter += hufmodel.check_model(ref, c.frame, c.want, c.cap, c.why, c.model_dict(), stricter_allowed=c.damaged and c.family == "damaged streams")
        except AssertionError as e: raise AssertionError("%s / %s: %s" % (c.family, c.name, e))
        try: got = oracle.decompress(c.frame, c.cap, c.dict_data)
        except RuntimeError: got = None
        assert got == c.want, (c.family, c.name, "the C oracle", c.why)
    return stricter


def placed(cases):
    """(pads, absolute offsets): every frame behind the filler that puts its aimed stream at its aimed offset mod 16"""
    pads, at, o = [], [], 0
    for c in cases:
        p = c.pad_for(o)
        pads.append(p); at.append(o + p); o += p + len(c.frame)
    return pads, at


def stats(emu):
    return {k: emu.stat(k) for k in (HOOK_K0, HOOK_DEEP, HOOK_REBUILT, HOOK_DICT_DEEP)}


def delta(emu, before):
    return {k: emu.stat(k) - v for k, v in before.items()}


def run_routes(emu, cases, led, label, generic_kwargs=None):
    """`cases` through the pipeline with K0 and without it, `led` (the same behind a raw block) in the several-block mode and through the generic kernel.
    Returns the hook counts per route and the census of everything that ran, every frame at its absolute place."""
    hooks, reached = {}, set()
    one_block = sum(len(c.blocks) == 1 for c in cases)
    try:
        for k0 in (1, 0):
            emu.set_k0(k0); emu.set_blocks(0)
            pads, at = placed(cases)
            before = stats(emu)
            outs, st, nfb = emu.decompress_pipeline([c.frame for c in cases], [c.cap for c in cases], n_blocks=3, chunk=0, pads=pads)
            hooks["K0" if k0 else "no K0"] = delta(emu, before)
            check_answers("%s: pipeline, K0 %s" % (label, "on" if k0 else "off"), cases, outs, st)
            assert nfb == len(cases) - one_block, (label, "frames handed to the generic kernel", nfb, len(cases), one_block)
            if k0:
                for c, a in zip(cases, at): reached |= c.huf_census(a)
        emu.set_k0(1); emu.set_blocks(SLOTS)
        pads, at = placed(led)
        before = stats(emu)
        outs, st, nfb = emu.decompress_pipeline([c.frame for c in led], [c.cap for c in led], n_blocks=3, chunk=0, pads=pads)
        hooks["several blocks"] = delta(emu, before)
        check_answers(label + ": several-block mode", led, outs, st)
        assert nfb == 0, (label, "several-block mode: frames handed to the generic kernel", nfb)
        for c, a in zip(led, at): reached |= c.huf_census(a)
    finally:
        emu.set_blocks(0); emu.set_k0(1)
    outs, st = emu.decompress_batch([c.frame for c in led], [c.cap for c in led], n_blocks=2, pads=pads, **(generic_kwargs or {}))
    check_answers(label + ": generic kernel", led, outs, st)
    return hooks, reached


def aimed(reached, event):
    return any(e.startswith(event) for e in reached)


def check_hooks(label, hooks, reached, cases, led, dictionary_deep=False):
    """each hook nonzero exactly where the frames aim at it"""
    one = sum(c.deep_blocks for c in cases if len(c.blocks) == 1)
    deep_blocks = {"K0": one, "no K0": one, "several blocks": sum(c.deep_blocks for c in led)}
    deep = aimed(reached, "table above K1b's slots")
    deep_one = any(e == "table above K1b's slots" for e in reached)
    k0_work = "FSE description in a frame of one block" in reached
    rebuilt = "treeless block rebuilds a table above K1b's slots" in reached
    want = {
        "K0": {HOOK_K0: k0_work, HOOK_DEEP: deep_one or dictionary_deep, HOOK_REBUILT: dictionary_deep, HOOK_DICT_DEEP: dictionary_deep},
        "no K0": {HOOK_K0: False, HOOK_DEEP: deep_one or dictionary_deep, HOOK_REBUILT: dictionary_deep, HOOK_DICT_DEEP: dictionary_deep},
        "several blocks": {HOOK_K0: False, HOOK_DEEP: deep or dictionary_deep, HOOK_REBUILT: rebuilt or dictionary_deep, HOOK_DICT_DEEP: dictionary_deep},
    }
    for route, w in want.items():
        got = {k: hooks[route][k] > 0 for k in w}
        assert got == w, (label, route, "hook counts", hooks[route], "expected nonzero", w)
        # and the streams decoded inside K1 counted: every section the model reaches on a table above K1b's slots, no other
        assert hooks[route][HOOK_DEEP] == deep_blocks[route], (label, route, "Huffman sections decoded inside K1", hooks[route][HOOK_DEEP], "expected", deep_blocks[route])


def test_census_constants_match_the_kernel_headers():
    """hufmodel.DEEP and RING restate ZP_HUF_LOGMAX and K1b's ring; the three guards on the table log are where the families aim"""
    csrc = os.path.join(ROOT, "python-zstandard_amd", "csrc")
    fmt = open(os.path.join(csrc, "zhip_format.hpp")).read()
    pipe = open(os.path.join(csrc, "zhip_decode_pipeline.hpp")).read()
    assert int(re.search(r"^#define ZP_HUF_LOGMAX (\d+)", fmt, re.M).group(1)) == hufmodel.DEEP
    assert int(re.search(r"^#define ZP_HUF_RING (\d+)", pipe, re.M).group(1)) * 4 == hufmodel.RING
    assert pipe.count("hufLog <= ZP_HUF_LOGMAX") == 2 and pipe.count("hufLog > ZP_HUF_LOGMAX") == 1
    assert re.search(r"^#define ZP_HUF_FRAMES (\d+)", fmt + pipe, re.M).group(1) == "12", "huffamilies.k1b_groups aims at 12 frames a wave trip"


def test_the_writer_leaves_earlier_frames_alone(ref):
    """craft.py's additions are additive: the natural-tree table, its description and both section layouts give the bytes they gave; an explicit table of
    the same weights gives the same code; the FSE form of a description decodes (the model, libzstd) to the weights of the direct one"""
    import hashlib
    import numpy as np
    from tests import craft
    rng = np.random.default_rng(5)
    lits = bytes(np.minimum(rng.integers(0, 101, 900), rng.integers(0, 101, 900)).astype(np.uint8))
    t = craft.HufTable(lits)
    frames = [craft.write_frame([("seq", lits[:n], [(5, 4, 5)], {"lit": mode})], content=b"x" * (n + 4)) for n, mode in ((300, "huf1"), (900, "huf4"))]
    assert hashlib.sha256(b"".join(frames)).hexdigest() == WRITER_PIN, "craft.py no longer writes the frames it wrote before HufTable.from_weights"
    e = craft.HufTable.from_weights(t.weights)
    assert (e.code, e.nbits, e.description()) == (t.code, t.nbits, t.description())
    for log in (5, 6):
        rep = {}
        d = e.description("fse", log, report=rep)
        w, lg, used = hufmodel.read_description(d)
        assert (w, lg, used) == (t.weights, t.max_bits, len(d)) and rep["weights"] == len(t.weights) - 1


WRITER_PIN = "6a2a7e31157c3b8eac18a3b7c2c39d8b4df710a54cd6e7de4dc5dfb076bcdea4"            # (computed with the frame writer of the commit before these additions)


@pytest.mark.parametrize("family", list(H.FAMILIES))
def test_huffman_families_through_the_emulated_kernels(emu, ref, oracle, family):
    """one family: the model against libzstd and the C oracle, then every route; the census must list every limit the family names, the refusals
    every reason, and the hooks must count where the family aims"""
    cases = H.FAMILIES[family]()
    led = [c.with_lead() for c in cases]
    stricter = judged(cases, oracle, ref) + judged(led, oracle, ref)
    assert (stricter > 0) == (family == "damaged streams"), (family, "frames the model refuses and libzstd decodes", stricter)
    hooks, reached = run_routes(emu, cases, led, family)
    missing = [e for e in H.REQUIRED[family] if e not in reached]
    assert not missing, (family, "limits the generators no longer reach", missing)
    if family in H.REFUSALS:
        assert {c.why for c in cases if c.want is None} >= H.REFUSALS[family], (family, H.REFUSALS[family] - {c.why for c in cases if c.want is None})
    check_hooks(family, hooks, reached, cases, led)


def test_dictionary_tables_of_log_11_and_12(emu, ref, oracle):
    """the trained dictionary of tests/golden with explicit tables of log 11 and 12 in place of its own: libzstd loads them; frames whose first block
    is treeless (one and four streams), frames with a table of their own, on every route under set_ddict. The log-11 table is shared with K1b where it
    lies, the log-12 ones are too deep: K1 rebuilds them from the weights and decodes in place (hooks [4], [5], [6])"""
    trained = open(TRAINED, "rb").read()
    reached = set()
    try:
        for name, d, cases in H.dictionaries(trained, TRAINED_CONTENT_OFF):
            blob, content, dict_id = emu.parse_dict(d)
            assert len(d) - len(content) == cases[0].content_off and dict_id == cases[0].header["dict_id"]
            led = [c.with_lead() for c in cases]
            assert judged(cases, oracle, ref) + judged(led, oracle, ref) == 0
            assert any(c.want is not None for c in cases), "libzstd does not load the dictionary"
            assert emu.set_ddict(d) == 0
            hooks, got = run_routes(emu, cases, led, "dictionary " + name, generic_kwargs={"dict_content": content, "dict_id": dict_id, "dict_entropy": blob})
            reached |= got
            check_hooks("dictionary " + name, hooks, got, cases, led, dictionary_deep="dictionary table log 12" in got)
    finally:
        emu.set_ddict(None)
    missing = [e for e in H.REQUIRED["dictionaries"] if e not in reached]
    assert not missing, missing


def test_k1b_groups_with_damaged_neighbours(emu, ref, oracle):
    """1, 11, 12, 13 and 25 Huffman frames among raw-literal ones (K1b decodes 12 frames a wave trip), a damaged stream in the first and in the twelfth:
    the damaged frame is refused and every neighbour decodes"""
    for name, cases in H.k1b_groups():
        judged(cases, oracle, ref)
        assert sum(c.want is None for c in cases) == sum(c.damaged for c in cases), name
        for blocks in (1, 2):
            outs, st, nfb = emu.decompress_pipeline([c.frame for c in cases], [c.cap for c in cases], n_blocks=blocks, chunk=0)
            check_answers("K1b groups: %s, %d workgroups" % (name, blocks), cases, outs, st)
            assert nfb == 0
