"""K3's long-item units and scalar-base addressing under the wave emulator: tests/k3units.py's cases through K1 -> K2 -> K3 (frames of one block),
the several-block mode (a raw block in front) and the generic kernel, judged by libzstd 1.5.7 first and held against seqmodel.execute
(tests/test_emu_sequences.py's run_routes). tests/k3units.batches restates the unit staging, and every shape a test is named for is asserted to be
in what it ran: the unit counts, the items around unit 64, the record's fields at their largest, the sources against the LDS history, the literal
modes. tests/test_gpu_k3_units.py runs the same frames on the GPU.

Mutations tried on a scratch copy of csrc/, each alone, under the emulator only, with what this file does then ("dies": a unit computes a wild offset and
the emulator's process ends with a segmentation fault in the test named, which fails the run all the same):
  1 the record's literal source one bit too narrow (`r_.w[1] & 0x1FFFFu` made `& 0xFFFFu`):
        test_record_fields_at_their_largest [raw] and [huf] fail (the runs that start above 65 535); nothing else has 64 KiB of literals in a block
  2 the record's match length one bit too narrow (`lenMi << 13` made `(lenMi & 0xFFFu) << 13`):
        dies in test_unit_counts_in_one_batch, at the far match of exactly the buffer's size (4 096: the only length that needs the thirteenth bit)
  3 the start mask off by one (a unit looks below its own slot only: `starts & (~0ull >> (63 - lane))` shifted right once more, bit 0 kept):
        dies in test_unit_counts_in_one_batch
  4 an item lane whose first unit is 63 leaves no mark (`first < 64` made `first < 63`):
        test_unit_counts_in_one_batch fails in all three modes (the item over units 63 | 64)
  5 the unit prefix sums written only above 65 units (`U > 64` made `U > 65`):
        dies in test_unit_counts_in_one_batch (65 units: unit 64 searches an array nobody wrote)
  6 the flush's 32-bit offset cut to 16 bits (`o0 = SB ? ob : 0u` made `ob & 0xFFFFu`):
        test_record_fields_at_their_largest [raw] and [huf] and test_sources_above_2_17_and_2_20 fail (the frames above 64 KiB)"""
import pytest

from tests import k3units as U
from tests import seqfamilies as F
from tests.seqmodel import K3
from tests.test_emu_sequences import build_cases, check_answers, run_routes


@pytest.fixture(scope="module")
def emu():
    from tests import emulib
    return emulib.Emu()


def _modes(cases):
    return [U.in_mode(c, m) for c in cases for m in U.MODES]


def _ran(done):
    return [b for c in done if c.content is not None for b in U.all_batches(c)]


def _blocks_present(done, modes=("raw", "huf1", "huf4", "rle")):
    seen = {m for c in done for m in U.block_modes(c)}
    assert seen >= set(modes), seen


@pytest.mark.parametrize("mode", U.MODES)
def test_unit_counts_in_one_batch(emu, ref, oracle, mode):
    """2 to 129 units and the most a batch admits, with raw, Huffman-coded and RLE literals (RLE runs are filled, not staged: those batches keep
    their far-match units only)"""
    done = run_routes(emu, [U.in_mode(c, mode) for c in U.unit_counts(K3)], oracle, ref, "unit counts, %s literals" % mode)
    ran = _ran(done)
    counts = {b["U"] for b in ran}
    if mode == "rle":
        assert counts >= {62, 63, 64} and max(counts) >= 239
        return
    assert counts >= {2, 63, 64, 65, 127, 128, 129, 239, 256}, sorted(counts)
    firsts = {(b["U"], i["first"], i["n"]) for b in ran for i in b["items"]}
    assert (64, 62, 2) in firsts and (65, 63, 2) in firsts and (69, 64, 2) in firsts and (68, 63, 3) in firsts       # the last item of 64; an item over units 63 | 64; one from 64
    assert any(b["carry"] == 15 and b["end"] == K3.asm_bytes and i["dst"] + i["len"] == b["end"] - b["hOff"] for b in ran for i in b["items"] if i["kind"] == "far")
    assert any(b["carry"] == 15 and b["end"] == K3.asm_bytes and i["kind"] == "lit" and i["n"] == 239 for b in ran for i in b["items"])
    assert any(i["n"] == 256 for b in ran for i in b["items"])                                                       # the record's literal-unit count at its largest
    both = [b for b in ran if len({i["lane"] for i in b["items"]}) < len(b["items"])]
    assert {b["U"] for b in both} >= {63, 64, 65, 127, 128, 129}                                                      # a literal run and a far match in one lane


def test_item_shapes(emu, ref, oracle):
    """lanes 0 and 63, every last-unit shift in both kinds, a pre-batch part above 16 bytes beside long items"""
    done = run_routes(emu, _modes(U.item_shapes(K3)), oracle, ref, "item shapes")
    _blocks_present(done, ("raw", "huf1", "rle"))
    items = [(i["lane"], i["kind"], i["len"]) for b in _ran(done) if b["lit"] != "rle" for i in b["items"]]
    for lane in (0, 63):
        assert {k for l, k, n in items if l == lane} >= {"lit", "far"}, lane
    for kind in ("lit", "far"):
        assert {n for l, k, n in items if k == kind} >= set(U.ITEM_LENGTHS), kind
    assert ("pre", 38) in {(k, n) for l, k, n in items} and ("pre", 17) not in {(k, n) for l, k, n in items}


@pytest.mark.parametrize("mode", ("raw", "huf"))
def test_record_fields_at_their_largest(emu, ref, oracle, mode):
    """a long literal run that starts above 65 535 in the block's literals, and long runs that end with a literal section of almost a block's size"""
    done = run_routes(emu, [U.in_mode(c, mode) for c in U.record_fields(K3)], oracle, ref, "record fields, %s literals" % mode)
    assert {m for c in done for m in U.block_modes(c)} == ({"raw"} if mode == "raw" else {"huf4"})
    lits = [(i["src"], i["len"], b["lit_size"]) for b in _ran(done) for i in b["items"] if i["kind"] == "lit"]
    assert any(src > 65535 for src, n, size in lits)
    assert any(src + n == size and size > 129000 for src, n, size in lits)
    assert any(0 < size - (src + n) < 32 for src, n, size in lits)


def test_sources_against_the_history(emu, ref, oracle):
    """long far matches wholly inside the LDS history, from one byte before it, across its first byte and wholly below it, before and after a slide"""
    done = run_routes(emu, _modes(U.history(K3)), oracle, ref, "history")
    for slid in (False, True):
        where = {i["where"] for b in _ran(done) if b["after_slide"] == slid for i in b["items"] if i["kind"] == "far"}
        assert where >= {"inside", "one before", "straddles", "below"}, (slid, where)


def test_sources_above_2_17_and_2_20(emu, ref, oracle):
    """far matches in units from above 2^17 and 2^20: frames of several blocks, in the several-block mode with slots for all of them and in the
    generic kernel"""
    cases = build_cases(_modes(U.distant_sources(K3)), oracle, ref)
    for c, lowest in zip(cases[::3], (1 << 17, 1 << 20)):
        srcs = [i["src"] for b in U.all_batches(c) for i in b["items"] if i["kind"] == "far"]
        assert sum(s >= lowest for s in srcs) >= 5 and min(srcs) < 1000, (c.name, srcs)
    try:
        emu.set_blocks(12)
        outs, st, nfb = emu.decompress_pipeline([c.frame for c in cases], [c.cap for c in cases], n_blocks=2, chunk=0)
    finally:
        emu.set_blocks(0)
    check_answers("several-block mode", cases, outs, st)
    assert nfb == 0
    outs, st = emu.decompress_batch([c.frame for c in cases], [c.cap for c in cases], n_blocks=2)
    check_answers("generic kernel", cases, outs, st)


def test_long_items_from_a_dictionary(emu, ref, oracle):
    """the dictionary instantiations: long far matches wholly inside a raw-content dictionary, a straddler beside long items"""
    cases = _modes(U.dictionary_cases(K3))
    try:
        assert emu.set_ddict(cases[0].dict_data, raw_content=True) == 0
        done = run_routes(emu, cases, oracle, ref, "raw dictionary", generic=False)
        outs, st = emu.decompress_batch([c.frame for c in done], [c.cap for c in done], n_blocks=2, dict_content=cases[0].dict_data)
    finally:
        emu.set_ddict(None)
    check_answers("raw dictionary: generic kernel", done, outs, st)
    ran = _ran(done)
    assert sum(i["where"] == "dictionary" for b in ran for i in b["items"] if i["kind"] == "far") >= 8
    reached = set()
    for c in done: reached |= c.census(K3)
    assert "dictionary straddler: self-overlapping" in reached and "dictionary: source wholly inside, ending at the frame's first byte" in reached


def test_small_slots(emu, ref, oracle):
    """slots of 0 to 33 and 40 bytes (the slack test's two arms: below 32 bytes the exact loads), short far matches and far units within 32 bytes of
    the slot's end; the slots lie back to back, so their starts take every alignment"""
    cases = _modes(U.small_slots(K3) + F.slot_edges(K3))
    done = run_routes(emu, cases, oracle, ref, "small slots")
    assert {c.cap for c in done} >= set(range(0, 35))
    starts, pos = set(), 0
    for c in cases: starts.add(pos % 16); pos += c.cap
    assert starts == set(range(16))
    reached = set()
    for c in done:
        if c.content is not None: reached |= c.census(K3)
    assert not [e for e in F.REQUIRED["slot edges"] if e not in reached]
    _blocks_present(done, ("raw", "huf1", "rle"))


def test_the_sanitizer_programs_fixture_is_what_the_generator_writes(ref, oracle):
    """tests/golden/k3_units.bin, which tests/emu/emu_k3_units.cpp decodes under ASan + UBSan, holds the frames tests/k3units.py writes today"""
    import os
    n, blob = U.fixture_blob(ref, oracle)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), U.FIXTURE)
    assert n >= 60 and open(path, "rb").read() == blob, "python -m tests.k3units --write-fixture"


def test_the_a_b_builds_stay_correct(oracle, ref, tmp_path):
    """csrc/build_variants.sh's nosbase + nounitown in one emulator build (every unit through the search, 64-bit lane addresses) and k3r8 (round 8's
    hand-off from this source): the unit counts and the history through the pipeline"""
    from tests import emulib
    for name, flags in (("search", ["-DZP_K3_SBASE=0", "-DZP_K3_UNITOWN=0"]), ("k3r8", ["-DZP_K3_SBASE=0", "-DZP_K3_UNITREC=0"])):
        emu = emulib.Emu(emulib.build_variant(str(tmp_path / ("libzhip_emu_%s.so" % name)), flags))
        run_routes(emu, _modes(U.unit_counts(K3) + U.history(K3)), oracle, ref, name, generic=False)
