"""The sequence decoders driven by EXPLICIT FSE distributions (tests/craft.py described() / mode 3, tests/fsefamilies.py), under the wave emulator.

The three sequence tables of a block -- literal lengths, offsets, match lengths -- reached the decode kernels in mode 2 (a distribution written in the
block) and mode 3 (repeat) only as libzstd's encoder chose them for some corpus. Here a table is a distribution and an accuracy log, its description
the writer's or raw bytes, a "repeat" the inheritance of a chosen predecessor; every family of tests/fsefamilies.py sits on both sides of its limit and
fsemodel.census must report each limit as reached (fsefamilies.REQUIRED). The code under test: zd_read_ncount_to (the serial parser: K1 on lane 0, K0 on
every lane), zd_build_fse (the wave-parallel spread), zd_seq_table's modes 2 and 3 (zhip_decode_kernel.hpp); zp_pack_fse, zp_block_tables with its
dictionary paths, K2's cells and bit ring (zhip_decode_pipeline.hpp); the C oracle's reader.

The expected value is tests/fsemodel.py's: the frame's own bytes decoded in plain Python (description reader, table builder, three interleaved states
over the backward stream), then seqmodel.execute. It is held against libzstd 1.5.7 for every frame first and a disagreement is reported as the model's
fault. There is NO stricter class: on every case verdict and bytes equal libzstd's.

Routes: the pipeline as the frames are, with K0 and without it (frames of one block take K0 -> K1 -> K2 -> K3, the others the generic kernel: the
count handed on is asserted); the several-block mode (a raw block in front of every frame); the generic kernel; the C oracle; the dictionary family
under set_ddict on all of them. Hook zd_stat[11] counts the distributions K1 took from K0's record: asserted EXACTLY (the count fsemodel predicts from
the frames' bytes) with K0 on, zero with K0 off and in the several-block mode.

WHAT THIS FOUND. A table whose cells are ALL "less than one" -- 32 symbols at accuracy log 5, which the LL, OF and ML alphabets can hold -- is valid and
libzstd decodes it. zd_build_fse computed `high = S - 1 - nLow` unsigned: with nLow = S it wrapped, the spread walk took every position for free and its
search over empty counts wrote symbol 63 into every cell, over the ballot's placements; the sequences then came from cells of a symbol no alphabet has
(the emulator's process dies on them). `high` is signed now and the walk places nothing; [less than one] holds the three
tables with all 32 cells "less than one" beside the ones with every symbol but one. K0 and the C oracle were right. Everything else agrees with libzstd.
Three cases one might look for do not exist, and the families say so where they would have stood:
  * a count that leaves `remaining < 1` cannot be written: the long form's largest field value stands for exactly `remaining` (mutation 7 below);
  * `high` cannot fall below a 64-cell boundary of a table: that takes 64 "less than one" symbols, the largest alphabet has 53 ([less than one]
    holds 35 / 31 / 52 of them at every log 7 .. 9 instead: the walk then skips positions in every 64-lane trip);
  * a block of thousands of sequences cannot carry 16-extra-bit length codes (its output ends at 128 KiB): [alphabets] and [single symbol] hold LL 35
    and ML 52 one sequence to a block. What stresses K2's bit ring is a few consecutive heavy steps (it is fed one burst of four ahead), and those fit:
    [bit rate] holds the heaviest step a frame of 128 KiB admits -- 26 state bits, offset code 16, LL code 35 and ML code 51: fsefamilies.MOST_BITS = 73
    bits -- and the heaviest four consecutive steps -- MOST_WINDOW = 277 bits of the 4 x 89 the ring is sized for, found by fsefamilies.heaviest_window's
    exhaustive search and pinned below -- at every offset mod 16 of the stream's first byte; both asserted from the census.
libzstd reads and builds a table one symbol owns entirely (norm[s] = 2^log; no state ever reads a bit), and so do the kernels: [single symbol].

Single-token mutations tried on a scratch copy of the headers, each alone, CPU only, with the families of this file that fail ("before": what failed in
tests/test_emu_sequences.py and tests/test_emu_huffman_tables.py, the suite before this file):
   1 `tl > maxLog` made `>=`:                         [accuracy logs] and eight more (every table at its kind's highest log)                (before: nothing)
   2 `tl > maxLog` dropped:                           [accuracy logs] (the process dies: a table of 1 024 cells in a slot of 512), K2 groups      (before: nothing)
   3 the limit one higher for LL / ML / OF, each
     alone:                                           [accuracy logs] (LL: and the K2 groups; ML: the process dies)                    (before: nothing, each)
   4 `sym <= maxS` made `<` (the loop's):             [alphabets], [less than one], [description ends], [bit rate], dictionaries
                                                      (before: the two dictionary tests: the trained dictionary's tables name their last symbol)
   5 `r != 3` made `r < 3 - 1`:                       [zero runs], [alphabets], [single symbol], [bit rate], K2 groups                       (before: nothing)
   6 `low < max` made `<=`:                           [count widths] and ten more                (before: the dictionary tests, Huffman [alphabet] and [FSE descriptions])
   7 `remaining < 1` made `< 0`:                      nothing, and nothing can: the long form's largest field value, 2 * threshold - 1, stands for the value `remaining`, a count of
                                                      `remaining` - 1, which leaves 1 ([count widths] holds the field at that value)                       (before: nothing)
   8 `remaining != 1` dropped:                        [count widths] (a total below 2^log at the alphabet's last symbol)                      (before: nothing)
   9 `p <= high` made `<`:                            every family with a "less than one" count (five of them die)      (before: test_emu_sequences.py dies, four Huffman families)
  10 `S - 1 - popc` made `S - 2 - popc`:              [less than one], [alphabets], [spread] (die), five more          (before: test_emu_sequences.py dies, Huffman [FSE descriptions])
  11 the binary search's `<=` made `<`:               every family                                                      (before: every decode test of both files)
  12 `L.run[s] = x + 1` dropped:                      [spread], [accuracy logs] and seven more: every table above 64 cells   (before: nothing -- the predefined tables have 64 cells and fewer)
  13 zp_pack_fse's `<< 10` made `<< 9`:               every family (the process dies)                                   (before: both files die)
  14 zp_pack_fse's masks `511u : 255u` exchanged:     nothing, and nothing can: the mask only feeds the test `local + k < (1 << lg)` that zeroes the cells above the table's
                                                      size; exchanged it is too small for the LL and ML halves, so cells above 2^log keep what lay in LDS -- cells no state
                                                      can name, a state being below 2^log; for the offsets' quarter both masks give the same value            (before: nothing)
  15 `*pLog == 0xFF` dropped:                         [mixed modes], [repeat chains], dictionaries (raw content): the process dies on a table never built    (before: nothing)
  16 `!dictInLds` made true always:                   dictionaries (block 1 described, block 2 "repeat": the dictionary's table again)         (before: nothing)
  17 `allShared` made "any table repeat":             dictionaries (one and two of three "repeat")                                            (before: nothing)
  18 `pre->t[kind].valid` read for the next kind:     every family of one-block frames, by bytes and by hook [11]'s exact count                (before: nothing)
  19 the fix taken back (`high` unsigned):            [less than one] (the process dies)                                                       (before: nothing)
"before" is tests/test_emu_sequences.py and tests/test_emu_huffman_tables.py, the two files of explicit frames, run with each mutant; tests/test_emu_kernels.py's
corpus-driven decode tests take a quarter of an hour a mutant and were not run with them. Twenty-one mutants (3 counts three), two argued equivalent."""
import hashlib
import os
import re

import pytest

from tests import fsefamilies as X
from tests import fsemodel, hufmodel, seqmodel
from tests.test_emu_sequences import SLOTS, TRAINED, TRAINED_CONTENT_OFF, TRAINED_REPS, check_answers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOK_K0_SEQ = 11
WRITER_PIN = "ecd770d895b64f4d0c4052459e11725ec0a5e8259767278bb12126c2505afb4a"            # (computed with the frame writer of the commit before modes 2 and 3)


@pytest.fixture(scope="module")
def emu():
    from tests import emulib
    return emulib.Emu()


def judged(cases, oracle, ref):
    """writes every frame; the model's verdict and bytes against libzstd's -- equal, no exception class -- and the C oracle's"""
    for c in cases:
        c.build(oracle.xxh64)
        try: seqmodel.check_model(ref, c.frame, c.want, c.cap, c.dict_data, c.raw_dict)
        except AssertionError as e: raise AssertionError("%s / %s (%s): %s" % (c.family, c.name, c.why, e))
        try: got = oracle.decompress(c.frame, c.cap, c.dict_data)
        except RuntimeError: got = None
        assert got == c.want, (c.family, c.name, "the C oracle", c.why)
    return cases


def k0_taken(c):
    """how many distributions K1 takes from K0's record for the frame of `c`: K0 walks a frame of ONE compressed block -- LL, OF, ML in order, over at
    most 256 staged bytes, stopping at the first description that does not parse and at a "repeat" --, and K1 takes what it reaches before it refuses"""
    blocks = hufmodel.walk(c.frame)
    if len(blocks) != 1 or blocks[0][0] != 2: return 0
    _, pos, size, _ = blocks[0]
    buf = c.frame[pos:pos + size]
    try: _, used, _ = hufmodel.literals_section(buf, None)
    except hufmodel.Refused: return 0
    sec = buf[used:]
    if len(sec) < 3 or sec[0] == 0: return 0
    at = 1 if sec[0] < 128 else 3 if sec[0] == 255 else 2
    modes = sec[at]; at += 1
    if modes & 3: return 0
    kinds = [(modes >> s) & 3 for s in (6, 4, 2)]
    valid, p = [None] * 3, at
    for k, m in enumerate(kinds):                               # K0
        if m == 3: break
        if m == 1:
            if p >= len(sec): break
            p += 1
        if m == 2:
            try: norm, log, n = hufmodel.read_ncount(sec[p:at + fsemodel.STAGED], fsemodel.MAX_SYMBOL[k])
            except hufmodel.Refused: break
            valid[k] = log; p += n
    taken, p = 0, at
    for k, m in enumerate(kinds):                               # K1
        if m == 3: break                                        # (no dictionary frame has one block AND a described table in front of a repeat that K0 reached)
        if m == 1:
            if p >= len(sec) or sec[p] > fsemodel.MAX_SYMBOL[k]: break
            p += 1
        if m == 2:
            if valid[k] is None: break
            taken += 1
            if valid[k] > fsemodel.MAX_LOG[k]: break
            p += hufmodel.read_ncount(sec[p:], fsemodel.MAX_SYMBOL[k])[2]
    return taken


def placed(cases):
    pads, at, o = [], [], 0
    for c in cases:
        p = c.pad_for(o)
        pads.append(p); at.append(o + p); o += p + len(c.frame)
    return pads, at


def run_routes(emu, cases, led, label, generic_kwargs=None, k0_runs=True):
    """`cases` through the pipeline with K0 and without it, `led` (the same behind a raw block) in the several-block mode and through the generic kernel;
    the hook count of every route asserted; returns the census of everything that ran, every frame at its absolute place"""
    reached = set()
    one_block = sum(len(c.blocks) == 1 for c in cases)
    expect = sum(k0_taken(c) for c in cases) if k0_runs else 0          # (K0 is not launched for a batch under a trained dictionary: zhip_decode_plan.hpp)
    try:
        for k0 in (1, 0):
            emu.set_k0(k0); emu.set_blocks(0)
            pads, at = placed(cases)
            before = emu.stat(HOOK_K0_SEQ)
            outs, st, nfb = emu.decompress_pipeline([c.frame for c in cases], [c.cap for c in cases], n_blocks=3, chunk=0, pads=pads)
            took = emu.stat(HOOK_K0_SEQ) - before
            check_answers("%s: pipeline, K0 %s" % (label, "on" if k0 else "off"), cases, outs, st)
            assert nfb == len(cases) - one_block, (label, "frames handed to the generic kernel", nfb, len(cases), one_block)
            assert took == (expect if k0 else 0), (label, "K0 %s: distributions K1 took from K0's record" % ("on" if k0 else "off"), took, "expected", expect if k0 else 0)
            if k0:
                for c, a in zip(cases, at): reached |= c.fse_census(a)
        emu.set_k0(1); emu.set_blocks(SLOTS)
        pads, at = placed(led)
        before = emu.stat(HOOK_K0_SEQ)
        outs, st, nfb = emu.decompress_pipeline([c.frame for c in led], [c.cap for c in led], n_blocks=3, chunk=0, pads=pads)
        check_answers(label + ": several-block mode", led, outs, st)
        # (an offset K2 cannot pack, ZP_OF_LIMIT and up -- [alphabets] uses the offset codes 29 .. 31 --, sends its frame on to the generic kernel, which refuses it)
        unpacked = sum(any(q[2] >= 0x1E000000 for b in c.blocks if b[0] == "seq" for q in b[2]) for c in led)
        assert nfb == unpacked, (label, "several-block mode: frames handed to the generic kernel", nfb, "expected", unpacked)
        assert emu.stat(HOOK_K0_SEQ) == before, (label, "several-block mode: K0 has no record of these frames")
        for c, a in zip(led, at): reached |= c.fse_census(a)
    finally:
        emu.set_blocks(0); emu.set_k0(1)
    outs, st = emu.decompress_batch([c.frame for c in led], [c.cap for c in led], n_blocks=2, pads=pads, **(generic_kwargs or {}))
    check_answers(label + ": generic kernel", led, outs, st)
    return reached, expect


def test_census_constants_match_the_kernel_headers():
    """fsemodel restates the format's limits as the headers name them, K2's slot and the bytes K0 and K1 stage; the guards the families aim at are where
    they were"""
    csrc = os.path.join(ROOT, "python-zstandard_amd", "csrc")
    fmt = open(os.path.join(csrc, "zhip_format.hpp")).read()
    gen = open(os.path.join(csrc, "zhip_decode_kernel.hpp")).read()
    pipe = open(os.path.join(csrc, "zhip_decode_pipeline.hpp")).read()

    def define(name): return re.search(r"^#define %s[ \t]+\(?(\d+)" % name, fmt + gen + pipe, re.M).group(1)
    assert tuple(int(define(n)) for n in ("ZF_MAXLL", "ZF_MAXOFF", "ZF_MAXML")) == fsemodel.MAX_SYMBOL
    assert tuple(int(define(n)) for n in ("ZF_LL_LOGMAX", "ZF_OF_LOGMAX", "ZF_ML_LOGMAX")) == fsemodel.MAX_LOG
    assert "u < 256 ? llLog : u < 512 ? mlLog : ofLog" in pipe and sum(fsemodel.K2_CELLS) == 1280
    assert pipe.count("< 256u ? ") == 2 and fsemodel.STAGED == 256, "K0 and K1 stage 256 bytes of a block's descriptions"
    assert "if (r < 0 || tl > maxLog) return -ZE_CORRUPTION;" in gen and "if (*pLog == 0xFF) return -ZE_CORRUPTION;" in gen


def test_the_writer_leaves_earlier_frames_alone(ref, oracle):
    """craft.py's additions are additive: every frame the sequence and Huffman families wrote before modes 2 and 3 existed has the bytes it had"""
    from tests import huffamilies as H
    from tests import seqfamilies as F
    h, n = hashlib.sha256(), 0
    for c in F.plain_families() + [x for g in H.FAMILIES.values() for x in g()]:
        c.build(lambda b: 0)
        h.update(len(c.frame).to_bytes(4, "little") + c.frame); n += 1
    assert (n, h.hexdigest()) == (959, WRITER_PIN), "craft.py no longer writes the frames it wrote before described() and mode 3"


def test_the_longest_descriptions_fit_what_k0_and_k1_stage():
    """the longest descriptions found (fsefamilies.longest_description: every zero count spelled out) -- 50 + 41 + 73 bytes, 164 together in one block of
    [description ends] -- and the bound no description exceeds: a symbol costs at most a count of log + 1 bits and a 2-bit flag, so 4 + 36 * 12,
    4 + 32 * 11 and 4 + 53 * 12 bits: 55 + 45 + 80 = 180 bytes, below the 256 that K0 and K1 stage"""
    sizes = [len(X.longest_description(k)[2]) for k in range(3)]
    assert sizes == [50, 41, 73], sizes
    bound = [(4 + (fsemodel.MAX_SYMBOL[k] + 1) * (fsemodel.MAX_LOG[k] + 3) + 7) // 8 for k in range(3)]
    assert bound == [55, 45, 80] and sum(bound) < fsemodel.STAGED


@pytest.mark.parametrize("family", list(X.FAMILIES))
def test_sequence_table_families_through_the_emulated_kernels(emu, ref, oracle, family):
    """one family: the model against libzstd and the C oracle, then every route; the census must list every limit the family names, the refusals
    every reason, hook [11] the exact count"""
    cases = judged(X.FAMILIES[family](), oracle, ref)
    led = judged([c.with_lead() for c in cases], oracle, ref)
    reached, taken = run_routes(emu, cases, led, family)
    missing = [e for e in X.REQUIRED[family] if e not in reached]
    assert not missing, (family, "limits the generators no longer reach", missing)
    assert {c.why for c in cases if c.want is None} >= X.REFUSALS.get(family, set()), (family, X.REFUSALS[family] - {c.why for c in cases if c.want is None})
    assert any(c.want is not None for c in cases)
    # (K0 walks the descriptions of the frames of one block; the families about what a later block inherits have none)
    assert (taken > 0) == any(len(c.blocks) == 1 for c in cases), (family, taken)


def test_dictionary_families(emu, ref, oracle):
    """the trained dictionary of tests/golden: every table "repeat" in the first block (the shared copy: ZP_LOGS_SHARED), one and two of three "repeat"
    beside described / RLE / predefined ones (the dictionary's cells dropped into LDS), block 1 described and block 2 "repeat" (block 1's table, not the
    dictionary's again), repeat / described / repeat over three blocks; and the same frames under its bytes as a raw-content dictionary: refused"""
    trained = open(TRAINED, "rb").read()
    reached = set()
    try:
        for name, cases in X.dictionary_frames(trained, TRAINED_CONTENT_OFF, TRAINED_REPS):
            raw = name == "raw content"
            judged(cases, oracle, ref)
            led = judged([c.with_lead() for c in cases], oracle, ref)
            # (a raw-content dictionary gives no tables: a frame whose first block repeats one is refused, "block 1 described, block 2 repeat" decodes)
            for c in cases: assert (c.want is None) == (raw and 3 in c.blocks[0][3]["modes"]), (name, c.name, c.why)
            assert emu.set_ddict(cases[0].dict_data, raw_content=raw) == 0
            if raw: kw = {"dict_content": cases[0].dict_data}
            else:
                blob, content, dict_id = emu.parse_dict(trained)
                kw = {"dict_content": content, "dict_id": dict_id, "dict_entropy": blob}
            got, _ = run_routes(emu, cases, led, "dictionary, " + name, generic_kwargs=kw, k0_runs=raw)
            if not raw: reached |= got
    finally:
        emu.set_ddict(None)
    missing = [e for e in X.REQUIRED["dictionaries"] if e not in reached]
    assert not missing, missing


def test_k2_groups_with_refused_neighbours(emu, ref, oracle):
    """1 / 14 / 15 / 16 / 31 frames with different logs per frame (5 / 5 / 5 beside 9 / 8 / 9, single-symbol and predefined tables) and refused members
    among them: one frame's logs must not leak into its neighbours of a K2 wave"""
    reached = set()
    for name, cases in X.k2_groups():
        judged(cases, oracle, ref)
        assert sum(c.want is None for c in cases) == len(cases) // 5, name
        for blocks in (1, 2):
            outs, st, nfb = emu.decompress_pipeline([c.frame for c in cases], [c.cap for c in cases], n_blocks=blocks, chunk=0)
            check_answers("K2 groups: %s, %d workgroups" % (name, blocks), cases, outs, st)
            assert nfb == 0
        reached |= fsemodel.group_census([c.frame for c in cases])
    missing = [e for e in X.REQUIRED["K2 groups"] if e not in reached]
    assert not missing, missing


def test_k2_groups_under_a_dictionary(emu, ref, oracle):
    """the same sizes under the trained dictionary: frames whose tables are all the dictionary's -- K2 copies the one shared set (ZP_LOGS_SHARED) -- beside
    frames with tables of their own in the arena, one and two of three "repeat", and refused ones"""
    trained = open(TRAINED, "rb").read()
    reached = set()
    try:
        assert emu.set_ddict(trained) == 0
        for name, cases in X.k2_dictionary_groups(trained, TRAINED_CONTENT_OFF, TRAINED_REPS):
            judged(cases, oracle, ref)
            assert sum(c.want is None for c in cases) == len(cases) // 5, name
            for blocks in (1, 2):
                outs, st, nfb = emu.decompress_pipeline([c.frame for c in cases], [c.cap for c in cases], n_blocks=blocks, chunk=0)
                check_answers("K2 dictionary groups: %s, %d workgroups" % (name, blocks), cases, outs, st)
                assert nfb == 0
            reached |= fsemodel.group_census([c.frame for c in cases], trained)
    finally:
        emu.set_ddict(None)
    missing = [e for e in X.REQUIRED["K2 dictionary groups"] if e not in reached]
    assert not missing, missing


def test_the_heaviest_steps_are_the_search_s():
    """fsefamilies.HEAVIEST / MOST_WINDOW restate heaviest_window()'s exhaustive search; MOST_BITS is 26 state bits, offset code 16 and the two length codes
    of 16 + 15 extra bits, the most whose sizes (65 536 + 32 771) leave room for the sequence that must follow in a frame of 128 KiB (16 + 16: 131 075)"""
    bits, steps, lead = X.heaviest_window()
    assert (bits, steps, lead) == (X.MOST_WINDOW, X.HEAVIEST, 0)
    assert X.MOST_BITS == 73 and 65536 + 65539 > 131072 >= 65536 + 32771 + 200 + 200 + 8


def test_the_fixture_of_descriptions_is_current():
    """tests/golden/fse_descriptions.bin (the sanitizer program's input) holds every description the families write"""
    import struct
    want = sorted(set(X.all_descriptions()))
    assert max(len(d) for _, d in want) == fsemodel.STAGED and any(k == 2 and d.startswith(X.longest_description(2)[2]) for k, d in want), "the longest description, whole"
    raw = open(X.FIXTURE, "rb").read()
    n, at, got = struct.unpack_from("<I", raw)[0], 4, []
    for _ in range(n):
        k, m, ln = struct.unpack_from("<BBH", raw, at); at += 4
        got.append((k, raw[at:at + ln])); at += ln
        assert m == fsemodel.MAX_SYMBOL[k]
    assert at == len(raw) and got == want, "run python -m tests.fsefamilies --write-fixture"


def test_the_parser_under_asan_and_ubsan(tmp_path):
    """tests/emu/ncount_bounds_main.cpp, a program of its own built with -fsanitize=address,undefined: zd_read_ncount_to over every description of the
    fixture and every proper prefix of each, source and counts in heap blocks of exactly their sizes"""
    import subprocess
    exe = str(tmp_path / "ncount_bounds")
    subprocess.check_call(["sh", os.path.join(ROOT, "tests", "emu", "build_ncount_bounds.sh"), exe])
    p = subprocess.run([exe, X.FIXTURE], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok: "), (p.returncode, p.stdout[-400:], p.stderr[-2000:])
    assert int(p.stdout.split()[1]) > 600, p.stdout
