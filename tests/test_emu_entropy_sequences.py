"""The entropy kernel driven by explicit sequences (tests/entropy_families.py), under the wave emulator: the loader (ze_load_sequences_body), the entropy
kernel (ze_entropy_body / ze_frame<false> / ze_compress_block<false>) and the trailer kernel, launched as zhip_compress_sequences_device launches them
(tests/emu/emu_entropy_sequences.cpp).

The suite's other encode tests take whatever sequences the project's own match searches find in a corpus, so a decision of the entropy kernel -- a table mode,
a header width, a normalisation path, a literal threshold -- is reached only when a search happens to produce the list that lands on it. Here every family
aims at its decisions from both sides. The expected frame is libzstd 1.5.7's ZSTD_compressSequences (explicit block delimiters, no validation) on the same
list, byte for byte; every list is handed over in two forms -- canonical repeat codes with ZSTD_c_searchForExternalRepcodes enabled in the reference, plain
offsets with it disabled -- and through both loader routes (sequences only: the entropy kernel gathers the literals; sequences and literals). Before a
kernel is looked at, the test's model is held against libzstd: the list must reproduce the source (seqmodel.execute, in both forms), the reference must
accept it, and the reference's frame must decode back to the source with libzstd; a failure there is reported as the model's or the generator's.
One limit of that attribution: ANY consistent coding of the same offsets reproduces the source, so a wrong repeat-code CHOICE in seqmodel.canonical would pass the
model checks and show as "differs from libzstd's frame" in the canonical form only (the plain form would still agree). What guards canonical() itself are the
hand-written expectations of test_canonical_restates_libzstds_repeat_offset_search; a mismatch confined to the canonical form should be read with that in mind.

Where the two forms of a list are the same list (no offset meets the repeat-offset history) the kernels run on it once per route and the one answer is
held against both of the reference's frames, which must then be equal too: the every-count and normalisation sweeps are built that way (offsets that stay clear
of the history), so they cost one run per route. The three lists of 0x7EFF .. 0x7F01 sequences and the other near-full-block cases run on one loader route each
(Case.route). Wall time with the emulator libraries built: 45 s on a quiet build host, 56 s beside another compile, against the 36 s of test_emu_sequences.py -- 1.3 to
1.5 x (building the two libraries first adds ~20 s, once). What it buys: ~1 150 cases (3 000 emulated frames at ~17 ms each, most of it the emulator's fiber switches, not bytes); the
table-mode sweep (every count 20 .. 80, three tables, two strategies: 16 s) and the normalisation sweep (11 s) are what the time goes to, not the near-full-block cases.

What the families reach together is asserted from a census of the REFERENCE's frames (entropy_families.frame_census), never of ours.
tests/stress_emu_entropy_sequences.py is the open-ended form, tests/test_gpu_entropy_sequences.py the same lists on the GPU."""
import collections
import os
import re

import numpy as np
import pytest

from tests import entropy_families as E
from tests import seqmodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("canonical", "plain")


@pytest.fixture(scope="module")
def emu():
    from tests import emulib
    return emulib.Emu()


@pytest.fixture(scope="module")
def ref():
    from tests import reflib
    return reflib.checker()          # libzstd 1.5.7 itself, or an error: never a skip


@pytest.fixture(scope="module")
def dicts():
    return E.load_dicts(ROOT)


def reference_frames(ref, cases, dicts):
    """c.want[form] = libzstd's frame for every good case (a refusal there is a generator bug), held against libzstd's own decoder; libzstd's verdict on the
    refused lists it checks too"""
    for c in cases:
        c.build(dicts)
        cfg = c.cfg
        d, _, _, raw = dicts[cfg.dict_name] if cfg.dict_name else (None, 0, None, False)
        params = dict(cfg.params, **({"format": 1} if cfg.magicless else {}))
        if c.refused is not None:
            if c.ref_refuses:
                with pytest.raises(RuntimeError, match="External sequences are not valid"):
                    ref.compress_sequences(c.source, [(ll, ml, max(o - 3, 1)) for ll, ml, o in c.seqs], 0, level=cfg.level, flags=cfg.flags())
            continue
        c.want = {}
        for form in FORMS:
            try:
                f = ref.compress_sequences(c.source, c.seqs, c.tail, level=cfg.level, flags=cfg.flags(), dict_data=d, dict_type=1 if raw else 0, rep_search=form == "canonical", **params)
            except RuntimeError as e:
                raise AssertionError("GENERATOR BUG, not a kernel: libzstd refuses %s / %s (%s): %s" % (c.family, c.name, form, e))
            back = ref.decompress_advanced(f, len(c.source), dict_data=d, dict_type=1 if raw else 0, format=1 if cfg.magicless else 0)
            assert back == c.source, "TEST MODEL, not a kernel: libzstd's frame for %s / %s (%s) does not decode to the source" % (c.family, c.name, form)
            c.want[form] = f
        c.one_list = np.array_equal(c.packed("canonical"), c.packed("plain"))
        if c.one_list: assert c.want["canonical"] == c.want["plain"], ("TEST MODEL, not a kernel: one list, two reference frames", c.family, c.name)
    return cases


def run_cases(emu, cases, dicts, n_blocks=3, chunk=0):
    """every case through the emulated kernels in its batch (one per Config), both forms, both loader routes; returns how many kernel answers were compared"""
    groups = collections.OrderedDict()
    for c in cases: groups.setdefault(c.cfg.key(), []).append(c)
    bad, compared = [], 0
    for cs in groups.values():
        cfg = cs[0].cfg
        d, _, reps, raw = dicts[cfg.dict_name] if cfg.dict_name else (None, 0, (1, 4, 8), False)
        assert emu.seq_set_dict(d, cfg.level, cfg.params, raw) == reps, "TEST MODEL, not a kernel: the lists start from other repeat offsets than the digested dictionary's"
        answers = {}
        for form in FORMS:
            for route in (0, 1):
                idx = [i for i, c in enumerate(cs) if c.route in (None, route) and (form == "canonical" or c.refused is not None or not c.one_list)]
                if not idx: continue
                frames, st = emu.entropy_sequences([cs[i].source for i in idx], [cs[i].packed(form) for i in idx], level=cfg.level, flags=cfg.flags(), load_flags=route,
                                                   params=cfg.params, dict_data=d, raw_dict=raw, magicless=cfg.magicless, n_blocks=n_blocks, chunk=chunk)
                for j, i in enumerate(idx):
                    c = cs[i]
                    compared += 1
                    if c.refused is not None:
                        if st[j] != c.refused or frames[j] != b"": bad.append((c.family, c.name, form, route, "not refused as it must be", st[j], len(frames[j])))
                        continue
                    wants = [c.want[form]] + ([c.want["plain"]] if c.one_list else [])
                    if st[j] != 0: bad.append((c.family, c.name, form, route, "status", st[j]))
                    elif any(frames[j] != w for w in wants):
                        w = wants[0]
                        first = next((k for k, (x, y) in enumerate(zip(frames[j], w)) if x != y), min(len(frames[j]), len(w)))
                        bad.append((c.family, c.name, form, route, "differs from libzstd's frame at byte", first, "sizes", len(frames[j]), len(w), E.frame_census(w, cfg.magicless)))
                    answers.setdefault((i, form), []).append(frames[j])
        for (i, form), fs in answers.items():
            assert all(f == fs[0] for f in fs), (cs[i].family, cs[i].name, form, "the two loader routes give different frames")
    assert not bad, (len(bad), bad[:8])
    return compared


@pytest.fixture(scope="module")
def plain_cases(ref, dicts):
    return reference_frames(ref, E.plain_families(), dicts)


@pytest.fixture(scope="module")
def dict_cases(ref, dicts):
    return reference_frames(ref, E.dictionary_families(dicts), dicts)


def test_the_models_constants_match_the_kernel_headers(emu, dicts):
    """entropy_families restates the slot's sequence capacity, the two status codes and where the trained dictionary's content starts"""
    fmt = open(os.path.join(ROOT, "python-zstandard_amd", "csrc", "zhip_format.hpp")).read()
    assert int(re.search(r"^#define ZE_MAX_SEQ (\d+)", fmt, re.M).group(1)) == E.SEQ_CAPACITY == emu.seq_capacity()
    assert re.search(r"ZE_SEQ_INVALID = (\d+)", fmt).group(1) == str(E.INVALID) and re.search(r"ZE_PARAM_UNSUPPORTED = (\d+)", fmt).group(1) == str(E.UNSUPPORTED)
    assert "#define ZE_SEQ_PACK(off, ll, ml) ((uint64_t)(off) | ((uint64_t)(ll) << 28) | ((uint64_t)(ml) << 46))" in fmt, "Case.packed restates this layout"
    d = dicts["json4k"][0]
    _, content, _ = emu.parse_dict(d)
    assert len(d) - len(content) == E.JSON4K_CONTENT_OFF
    assert [b for b in E.LL_BASE if b >= 16][:3] == [16, 18, 20] and len(E.LL_BASE) == 36 and len(E.ML_BASE) == 53


def test_canonical_restates_libzstds_repeat_offset_search(emu, dicts):
    """seqmodel.canonical, pinned by hand-written expectations: the history starts at (1, 4, 8) without a dictionary and at the dictionary's with one; an
    offset equal to a history entry becomes that entry's code; without literals the codes shift and 'entry one minus one' exists"""
    def codes(seqs, reps=(1, 4, 8)):
        return [c for _, _, c in seqmodel.canonical([("seq", b"", [(ll, ml, o + 3) for ll, ml, o in seqs], {})], reps)[0][2]]
    assert codes([(5, 3, 1)]) == [1] and codes([(5, 3, 4)]) == [2] and codes([(5, 3, 8)]) == [3] and codes([(5, 3, 2)]) == [5]
    assert codes([(0, 3, 4)]) == [1] and codes([(0, 3, 8)]) == [2] and codes([(0, 3, 1)]) == [4], "without literals: entries two and three, entry one is a plain offset"
    assert codes([(5, 3, 9), (0, 3, 8)]) == [12, 3], "'entry one minus one' without literals"
    assert codes([(5, 3, 9), (2, 3, 8)]) == [12, 11], "with literals there is no 'entry one minus one'"
    assert codes([(1, 3, 20), (1, 3, 30), (1, 3, 20), (0, 3, 20), (0, 3, 19)]) == [23, 33, 2, 23, 3], "entry one cannot be named without literals; the history moves with every code"
    assert codes([(5, 3, 7), (5, 3, 30), (0, 3, 100)], E.OTHER_REPS) == [1, 2, 2], "the history starts from the dictionary's"
    assert emu.seq_set_dict(dicts["json4k, other repeat offsets"][0]) == E.OTHER_REPS and emu.seq_set_dict(None) == (1, 4, 8)
    assert emu.seq_set_dict(dicts["json4k"][0]) == (1, 4, 8) and emu.seq_set_dict(dicts["raw content"][0], raw_dict=True) == (1, 4, 8)
    emu.seq_set_dict(None)


@pytest.mark.parametrize("family", [f for f in E.PLAIN if f != "refused lists"])
def test_family_against_libzstd(emu, plain_cases, dicts, family):
    cases = [c for c in plain_cases if c.family == family]
    assert cases
    n = run_cases(emu, cases, dicts)
    assert n >= 2 * sum(1 for c in cases if c.route is None), "every case on both loader routes"


def test_refused_lists_among_good_ones(emu, plain_cases, dicts):
    """every refused list between two good neighbours in one batch: it gets its status and no bytes, and the neighbours' frames are libzstd's -- the batch is cut
    into launches of five sources, so refusals also sit at a launch's first and last place"""
    bad = [c for c in plain_cases if c.refused is not None]
    good = [c for c in plain_cases if c.refused is None and c.cfg is E.DEFAULT and c.route is None and len(c.source) < 3000]
    assert len(bad) >= 8 and len(good) > 2 * len(bad)
    mixed = []
    for i, c in enumerate(bad): mixed += [good[2 * i], c, good[2 * i + 1]]
    run_cases(emu, mixed[1:], dicts, n_blocks=2, chunk=5)


def test_dictionary_families_against_libzstd(emu, dict_cases, dicts):
    run_cases(emu, dict_cases, dicts)


def census_of(cases):
    seen = collections.Counter()
    for c in cases:
        if c.refused is not None: continue
        for form in FORMS:
            k = E.frame_census(c.want[form], c.cfg.magicless)
            seen[("block", k["block"])] += 1
            if k["block"] != "compressed": continue
            seen[("literals", k["lit_type"], k["lit_format"])] += 1
            if "streams" in k: seen[("streams", k["streams"])] += 1
            seen[("count width", k["count_width"])] += 1
            if k["modes"]:
                for t, m in zip(("ll", "of", "ml"), k["modes"]): seen[(t, m)] += 1
    return seen


# what the families must reach together, read from libzstd's frames. Literal types 0 raw, 1 RLE, 2 compressed, 3 treeless with the size formats each can take:
# libzstd writes raw and RLE sections with formats 0, 1 and 3 (never 2), and no RLE section with the 1-byte header at these strategies -- below 64 literals it does
# not try to compress, and with a valid dictionary table (where it tries from 6) it reuses that table for up to 1 024 literals before it looks for a single value.
REQUIRED_PLAIN = [("block", "raw"), ("block", "compressed"), ("literals", 0, 0), ("literals", 0, 1), ("literals", 0, 3), ("literals", 1, 1), ("literals", 1, 3),
                  ("literals", 2, 0), ("literals", 2, 1), ("literals", 2, 2), ("literals", 2, 3), ("streams", 1), ("streams", 4),
                  ("count width", 1), ("count width", 2), ("count width", 3)] + [(t, m) for t in ("ll", "of", "ml") for m in (0, 1, 2)]
# Treeless sections: formats 0 and 2. These dictionaries' Huffman tables are VALID ones (every byte value has a code), and with a valid table libzstd writes up to 1 023
# literals in ONE stream -- format 0, never format 1 --; from 1 024 on it is four streams in format 2. Format 3 needs 16 384 literals or more in a source the dictionary
# call still takes (16 384 bytes at most: a source of nothing but literals), and at that size libzstd builds a new table for this text (probed with the reference: new
# tables from ~2 000 literals of the dictionary's own text on), so it is out of reach here.
REQUIRED_DICT = [("block", "raw"), ("block", "compressed"), ("literals", 3, 0), ("literals", 3, 2)] + [(t, 3) for t in ("ll", "of", "ml")]


def test_census_of_the_references_frames(plain_cases, dict_cases):
    seen = census_of(plain_cases)
    missing = [k for k in REQUIRED_PLAIN if not seen[k]]
    assert not missing, ("the families do not reach", missing, dict(seen))
    seen = census_of(dict_cases)
    missing = [k for k in REQUIRED_DICT if not seen[k]]
    assert not missing, ("the dictionary families do not reach", missing, dict(seen))


def test_the_stand_alone_programs_fixture_is_current(ref, dicts, plain_cases):
    """tests/golden/entropy_sequences.bin (input of the stand-alone emulator program, tests/emu/build_asan.sh) holds what the generators and libzstd give today"""
    from tests import stress_emu_entropy_sequences as S
    want = S.fixture_bytes(ref, dicts, plain_cases)
    have = open(os.path.join(ROOT, "tests", "golden", "entropy_sequences.bin"), "rb").read()
    assert have == want, "regenerate it: python tests/stress_emu_entropy_sequences.py --write-fixture"
