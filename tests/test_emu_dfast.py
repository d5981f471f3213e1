"""The double-fast searches on the host (emu/emu_dfast.cpp: ze_dfast, ze_dfast_flat_np with two, three and four probes a trip, its block form, ze_dfast_g under a window),
sequence by sequence against libzstd 1.5.7's own parse (ZSTD_generateSequences): position, matchLength and resolved offset of every sequence, the last literals of every block.
The sources are tests/dfast_sources.py's. For each one the test FIRST asserts, from libzstd's sequences, the property the source exists for -- a failure there is the source's
fault and says so -- and then compares every form. The expected value is never another form of the project's own search."""
import os
import subprocess

import numpy as np
import pytest

from tests import dfast_sources as ds

from tests.dfast_check import FORMS, HERE, Emu, Lz, build_emu, differences, param_sets, property_failures  # noqa: F401


@pytest.fixture(scope="module")
def lz():
    from tests import reflib
    if not reflib.have_ref():
        pytest.skip("no libzstd 1.5.7 available")
    return Lz()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return Emu(build_emu(tmp_path_factory.mktemp("emu_dfast")))


def _all_same(cases, lz, emu):
    total = 0
    for c in cases:
        d = differences(c, lz, emu)
        assert not d, "%r (%d bytes): %d differences from libzstd, the first in form %s under %r, block %d: %s (last literals %s) against libzstd's %s (%s)" % ((c.name, len(c.raw), len(d)) + d[0])
        total += 1
    return total


def test_step_growth_and_the_long_cell_behind_a_match(lz, emu):
    cases = ds.step_sources()
    assert {int(c.name.split()[1]) for c in cases} == {1, 2, 3, 4, 5}
    assert _all_same(cases, lz, emu) >= 30


def test_end_of_source(lz, emu):
    cases = ds.end_sources()
    assert {len(c.raw) for c in cases} >= set(range(8, 81)) | {4095, 4096, 4097, 131071, 131072}
    assert _all_same(cases, lz, emu) > 500


def test_which_candidate_wins(lz, emu):
    assert _all_same(ds.candidate_sources(), lz, emu) >= 11


def test_long_candidate_at_the_lowest_index(lz, emu):
    """only ze_dfast_g has a lowest index above the frame's first byte (a window shorter than the frame); the other forms do not take these sources"""
    cases = ds.lowest_index_sources()
    for c in cases:
        for p, cp in param_sets(c, lz): assert (1 << cp["window_log"]) < len(c.raw)
    assert _all_same(cases, lz, emu) == 4


def test_equal_cells_inside_a_trip(lz, emu):
    assert _all_same(ds.equal_cell_sources(), lz, emu) > 40


def test_catch_up_backwards(lz, emu):
    assert _all_same(ds.catch_up_sources(), lz, emu) >= 14


def test_repeat_offsets(lz, emu):
    assert _all_same(ds.repeat_offset_sources(), lz, emu) >= 3


def test_insertions_behind_a_match(lz, emu):
    assert _all_same(ds.insertion_sources(), lz, emu) == len(ds.INSERTIONS)


def test_blocks_tables_and_repeat_offsets_carried(lz, emu):
    cases = ds.block_sources()
    for c in cases: assert len(lz(c.raw)) >= 2
    assert _all_same(cases, lz, emu) == 6


def test_table_copy_mode_against_a_dictionary(lz, emu):
    """ze_dfast_ext, sequence by sequence: a raw-content dictionary digested by the product's own kernels, sources above the attach cutoff and of two blocks. libzstd's first
    sequence must begin in the dictionary (an offset larger than the position): the reference did search with the dictionary as an external segment."""
    cases = ds.ext_sources()
    assert len(cases) > 150 and all(len(c.raw) > 16384 for c in cases) and sum(1 for c in cases if len(c.raw) > ds.BLOCK) == 2
    for c in cases:
        first = lz(c.raw, dict_data=c.dict_data)[0][0][0]
        assert first[2] > first[0], (c.name, first)
    assert _all_same(cases, lz, emu) == len(cases)


def test_launch_numbers_in_tables_that_are_never_zeroed_again(lz, emu):
    """one allocation, zeroed once, launches 1 ... 63 each with another aimed source (and other parameters) in the slot: cells of earlier launches read as empty"""
    cases = [c for c in ds.one_block_sources() if 64 <= len(c.raw) <= 4200]
    tables = np.zeros((1 << 17) + (1 << 16), dtype=np.uint32)
    for epoch in range(1, 64):
        c = cases[(epoch * 37) % len(cases)]
        sets = param_sets(c, lz)
        p, cp = sets[epoch % len(sets)]
        want = lz(c.raw, **p)
        assert not property_failures(c, want), "the SOURCE %r misses its aim under %r" % (c.name, p)
        got = emu.flat(c.raw, cp, 2 + epoch % 3, epoch=epoch, tables=tables)
        assert got == want, (epoch, c.name, p)
    assert int((tables >> 26).max()) == 63 and np.count_nonzero(tables) > 2000          # (the launches really shared the cells)


def test_dictionary_forms_on_whole_frames(ref):
    """the end-of-source and step families with their match targets in a raw-content dictionary, through the emulated kernels (emulib's compress_batch), whole frames against
    libzstd. That the attach-mode searches ran is held by the emulator's hooks: in the pipeline every source is counted by the flat match kernel (hook 15) while the
    dictionary-less flat search makes no trip (hook 10) -- so ze_dfast_dict_flat searched --; without the pipeline the flat kernel counts nothing, the dictionary's resolved
    strategy is double-fast and every source is below the attach cutoff, which leaves ze_dfast_dict."""
    from tests import emulib
    emulib.build()
    kernels = emulib.Emu()
    checked = 0
    for d, raws in ds.dictionary_batches():
        assert ref.cdict_params(3, len(d))["strategy"] == ds.STRATEGY_DFAST and all(64 <= len(r) <= 16384 for r in raws)
        want = [ref.compress(r, level=3, dict_data=d) for r in raws]
        assert sum(1 for r, w in zip(raws, want) if w != ref.compress(r, level=3)) > len(raws) // 2, "the dictionary holds the match targets: frames differ from those without it"
        for pipeline in (True, False):
            flat0, trips0 = kernels.stat(15), kernels.stat(10)
            outs, st = kernels.compress_batch(raws, level=3, flags=5, pipeline=pipeline, dict_data=d)
            bad = [i for i in range(len(raws)) if st[i] != 0 or outs[i] != want[i]]
            assert not bad, (pipeline, len(d), bad[:8], [len(raws[i]) for i in bad[:8]])
            assert kernels.stat(15) - flat0 == (len(raws) if pipeline else 0) and kernels.stat(10) == trips0, (pipeline, kernels.stat(15) - flat0, kernels.stat(10) - trips0)
            checked += len(raws)
    assert checked > 60


def test_table_copy_mode_on_whole_frames(ref):
    """the sources of ze_dfast_ext as whole frames through the emulated kernels (the generic kernel's ze_compress_block in copy mode, with and without the pipeline in front):
    every frame libzstd's. What the GPU file's copy-mode case runs on the device."""
    from tests import emulib
    emulib.build()
    kernels = emulib.Emu()
    checked = 0
    for d, raws in ds.ext_batches(24):
        assert all(len(r) > 16384 for r in raws)
        want = [ref.compress(r, level=3, dict_data=d) for r in raws]
        for pipeline in (True, False):
            outs, st = kernels.compress_batch(raws, level=3, flags=5, pipeline=pipeline, dict_data=d)
            bad = [i for i in range(len(raws)) if st[i] != 0 or outs[i] != want[i]]
            assert not bad, (pipeline, len(d), bad[:8], [len(raws[i]) for i in bad[:8]])
            checked += len(raws)
    assert checked == 2 * 174


def test_sanitizer_program_over_the_fixture(lz, tmp_path):
    """emu/emu_dfast.cpp as a stand-alone program (its own main, nothing loaded into Python) under AddressSanitizer and UBSan over golden/dfast_sources.bin: every source in an
    allocation of exactly its size. This is what found the flat search, at three and four probes a trip, reading a candidate's 8 bytes from a position behind ilimit -- up to
    (probes - 1) * step bytes past the source's end -- when two speculative probes past ilimit shared a cell; the 16-byte sources of the end-of-source family show it.
    The fixture must be what the generators give now."""
    path = os.path.join(HERE, ds.FIXTURE)
    fresh = str(tmp_path / "dfast_sources.bin")
    n = ds.write_fixture(fresh)
    assert open(fresh, "rb").read() == open(path, "rb").read(), "tests/golden/dfast_sources.bin is stale: python -m tests.dfast_sources --write-fixture"
    assert n > 500 and any(len(c.raw) == 16 for c in ds.fixture_cases()) and any(len(c.raw) > ds.BLOCK for c in ds.fixture_cases())
    exe = str(tmp_path / "emu_dfast_asan")
    emu = os.path.join(HERE, "emu")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-I" + emu, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-w", "-DEMU_DFAST_MAIN",
                           "-o", exe, os.path.join(emu, "zhemu.cpp"), os.path.join(emu, "emu_dfast.cpp")])
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "%d sources" % n in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-1500:])
