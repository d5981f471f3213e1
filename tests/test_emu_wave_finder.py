"""The wave-parallel match finder (ZHIP_FINDER_WAVE: ze_match_wave_body, one wave per source, hash table in LDS, 64 positions per trip) on the 64-fiber host
emulator, with the entropy kernel and the trailer kernel behind it (tests/emu/emu_wave_finder.cpp). Its frames are valid zstd, not libzstd's bytes, so the checks
are: every sequence list replays to its source, every frame decodes under libzstd 1.5.7 and under the oracle decoder, repeat codes are used, the output is the
same on every run and for every grid, and it is what tests/golden/wave_finder.json records (which tests/test_gpu_wave_finder.py holds the MI355X to)."""
import hashlib
import json
import os
import subprocess

import pytest

from tests import seqmodel, wave_emu
from tests import wave_sources as ws

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return wave_emu.build(tmp_path_factory.mktemp("emu_wave_finder"))


@pytest.fixture(scope="module")
def sources(corpus):
    return ws.all_sources(corpus)


@pytest.fixture(scope="module")
def level3(lib, sources):
    """the whole set at level 3, default flags, computed once: (frames, statuses, sequence lists, modes)"""
    return wave_emu.frames(lib, [r for _, r in sources], level=3, want_seqs=True)


def _literals(raw, seqs):
    lits, pos = bytearray(), 0
    for ll, ml, _ in seqs:
        lits += raw[pos:pos + ll]; pos += ll + ml
    assert pos <= len(raw), "the lengths sum to more than the source"
    return bytes(lits + raw[pos:])


def _check_lists(sources, lists, modes, what):
    total = 0
    for (name, raw), seqs, mode in zip(sources, lists, modes):
        assert mode == (1 if len(raw) < 7 else 4), (what, name, mode)
        if mode != 4:
            continue
        assert all(ml >= 3 and ofb >= 1 for _, ml, ofb in seqs), (what, name)
        assert sum(ll + ml for ll, ml, _ in seqs) <= len(raw), (what, name)
        assert len(seqs) * 4 <= len(raw), (what, name)
        got = seqmodel.execute([("seq", _literals(raw, seqs), seqs)])          # raises Invalid for an offset beyond the history or a repeat code that resolves to 0
        assert got == raw, "%s: %s: the sequence list does not replay to the source" % (what, name)
        total += len(seqs)
    return total


def test_every_sequence_list_replays_to_its_source(lib, sources, level3):
    _, st, lists, modes = level3
    assert not any(st), st
    assert _check_lists(sources, lists, modes, "level 3") > 10000
    by = dict(zip([n for n, _ in sources], lists))
    # the second half copies the first at offset 65 536, over random bytes, which publish EVERY position: a cell keeps its last writer, and for position 65 536 + k to find k
    # no position between them may fall into its cell -- (1 - 2^-H)^65536, e^-16 per position with the product's 4 096 cells, so the copy is not found (a raw block);
    # with 8 192 and 16 384 cells it is e^-8 and e^-4, some position finds it, catch-up walks back to the half's first byte and the whole wave extends to the end
    assert by["half copy"] == [], by["half copy"]
    for hlog in (13, 14):
        _, sth, listh, _ = wave_emu.frames(lib, [ws.half_copy()], level=3, hlog=hlog, want_seqs=True)
        assert sth == [0] and listh[0] == [(65536, 65536, 65536 + 3)], (hlog, listh[0][:4])
    assert len(by["constant 131072"]) == 1 and by["constant 131072"][0][:2] == (1, 131071)
    assert by["four bytes at the fourth-last"] == [] and by["far match"] == []                # their loads would cross the end: literals
    n, off = ws.FAR_FOUND
    assert by["far match found"][-1] == (0, 64, off + 3), by["far match found"]
    assert by["match to the last byte"] == [(4970, 30, 4870 + 3)]
    assert by["match past the end"] == [(5003 - 301, 301, 5003 - 301 - 100 + 3)]
    # sequence-count pressure: where 4-byte matches are taken (min_match 4) the set's densest list, far inside the slot's capacity
    raw = ws.sequence_pressure()
    _, st4, lists4, modes4 = wave_emu.frames(lib, [raw], level=3, want_seqs=True, min_match=4)
    assert st4 == [0] and _check_lists([("sequence pressure", raw)], lists4, modes4, "min_match 4") > 6000, len(lists4[0])
    for level, hlog in ((1, 12), (-3, 12), (3, 13), (3, 14)):
        small = [(n, r) for n, r in sources if len(r) <= 20000]
        _, st, lists, modes = wave_emu.frames(lib, [r for _, r in small], level=level, hlog=hlog, want_seqs=True)
        assert not any(st), (level, hlog, st)
        _check_lists(small, lists, modes, "level %d, table log %d" % (level, hlog))


def test_frames_decode_under_libzstd_and_the_oracle(lib, sources, level3, ref, oracle):
    small = [(n, r) for n, r in sources if len(r) <= 20000]
    runs = 0
    for level in (-3, 1, 3):
        for k, (content_size, checksum) in enumerate(((True, False), (False, True), (True, True), (False, False))):
            use = sources if k == 0 else small                                             # (the large sources once per level)
            if level == 3 and k == 0:
                got, st = level3[0], level3[1]
            else:
                got, st = wave_emu.frames(lib, [r for _, r in use], level=level, checksum=checksum, content_size=content_size)
            for (name, raw), f, s in zip(use, got, st):
                what = (level, content_size, checksum, name)
                assert s == 0, what
                assert ref.decompress(f, len(raw)) == raw, what
                assert oracle.decompress(f, len(raw)) == raw, what
                if content_size:
                    assert ref.frame_content_size(f) == len(raw), what
                if name.startswith("random"):                                              # incompressible: a raw block, what libzstd writes too
                    assert len(f) == len(ref.compress(raw, level=level, flags=_flags(content_size, checksum))) == len(raw) + _overhead(len(raw), content_size, checksum), what
            runs += 1
    assert runs == 12


def _flags(content_size, checksum):
    from tests import reflib
    return (reflib.F_CONTENTSIZE if content_size else 0) | (reflib.F_CHECKSUM if checksum else 0) | reflib.F_DICTID


def _overhead(n, content_size, checksum):
    """magic, frame header descriptor, window byte or content size, one block header, optional checksum"""
    fcs = (1 if n < 256 else 2 if n < 65536 + 256 else 4) if content_size else 0
    return 4 + 1 + (fcs if content_size else 1) + 3 + (4 if checksum else 0)


def test_repeat_codes_are_used(sources, level3):
    """census of the offBase field on the periodic sources with changed bytes: behind each changed byte the match resumes at the offset of the one before, which must
    cost a repeat code (offBase 1 behind literals), not 17 bits of offset"""
    lists = dict(zip([n for n, _ in sources], level3[2]))
    for p in ws.PERIODS:
        seqs = lists["period %d glitched" % p]
        glitches = len(ws.glitches_for(20000, p))
        assert glitches == 7 and len(seqs) >= 3, (p, seqs)
        assert seqs[0][2] == (1 if p == 1 else p + 3), (p, seqs[0])                          # the period itself (period 1 IS the frame's first repeat offset)
        if p >= 5:
            # the changed byte at g: the repeat offset matches again from g + 1 for p - 1 bytes (up to the changed byte's image), then from g + p + 1 on
            assert len(seqs) == 1 + 2 * glitches and all(q[2] == 1 and q[0] == 1 for q in seqs[1:]), (p, seqs)
        elif p >= 2:
            # p - 1 < minMatch bytes match behind a changed byte, so ONE other offset has to come in (a multiple of the period); every sequence after it repeats it
            assert seqs[1][2] > 3 and (seqs[1][2] - 3) % p == 0 and all(q[2] == 1 and q[0] > 0 for q in seqs[2:]) and len(seqs) >= 2 + glitches, (p, seqs)
        else:
            assert seqs[1][2] == 1 and seqs[1][0] == 2, seqs                               # the byte behind the changed one has no repeat match, the next one has
    one = lists["period 3 one block"]
    assert len(one) >= 9 and all(q[2] == 1 for q in one[2:]), one


def test_output_is_deterministic_and_independent_of_the_grid(lib, sources, level3):
    raws = [r for _, r in sources]
    again, st = wave_emu.frames(lib, raws, level=3)
    assert not any(st) and again == level3[0]
    one, st = wave_emu.frames(lib, raws, level=3, blocks=1)                                 # one wave takes every source in turn
    assert not any(st) and one == level3[0]
    rev, st = wave_emu.frames(lib, raws[::-1], level=3, blocks=5)                            # other neighbours, another wave
    assert not any(st) and rev[::-1] == level3[0]


def test_frames_are_the_fixtures(corpus, sources, level3):
    fx = json.load(open(os.path.join(HERE, "golden", "wave_finder.json")))
    assert fx["level"] == 3 and fx["table_log"] == 12 and 20 <= len(fx["frames"]) <= 30
    got = dict(zip([n for n, _ in sources], level3[0]))
    raws = dict(sources)
    assert [row["name"] for row in fx["frames"]] == [n for n, _ in ws.small_sources(corpus)]
    for row in fx["frames"]:
        name = row["name"]
        assert hashlib.sha256(raws[name]).hexdigest() == row["src_sha256"] and len(raws[name]) == row["src_size"], "the source %r changed" % name
        assert (len(got[name]), hashlib.sha256(got[name]).hexdigest()) == (row["size"], row["sha256"]), name


def test_default_finder_still_writes_libzstds_frames(lib, sources, ref):
    """the emulator program's own finder switch: with the finder left at its default it runs the lane-serial match kernel and the frames are libzstd's, byte for byte.
    (The product's dispatch in zhip_compress_batch_device is host code the emulator does not run: tests/test_gpu_wave_finder.py's alternating-finder test guards that.)"""
    use = [(n, r) for n, r in sources if len(r) <= 20000 or n in ("text 131072", "half copy")]
    got, st = wave_emu.frames(lib, [r for _, r in use], level=3, finder="libzstd")
    for (name, raw), f, s in zip(use, got, st):
        assert s == 0 and f == ref.compress(raw, level=3), name
    wave, _ = wave_emu.frames(lib, [r for _, r in use], level=3)
    assert wave != got


def test_refusals(lib, corpus):
    text = corpus.frame_bytes(9)
    big, bigger = text + text[:1], (text * 3)[:300000]
    raws = [text[:5000], big, text[:70000], bigger, b"abc"]
    got, st = wave_emu.frames(lib, raws, level=3)
    assert st == [0, 40, 0, 40, 0] and got[1] == b"" and got[3] == b""                      # several blocks: refused at their own index
    assert wave_emu.frames(lib, [text[:40000], text[:900]], level=3, window_log=10)[1] == [40, 0]      # a window that does not cover the source
    assert wave_emu.frames(lib, [text[:40000], text[:9000]], level=4)[1] == [0, 40]                    # level 4: greedy at 16 KiB and below
    assert wave_emu.frames(lib, [text], level=3, hash_log=18)[1] == [40]                               # table logs the entropy kernel refuses
    for kw in (dict(level=5), dict(level=6), dict(level=3, strategy=4)):
        with pytest.raises(RuntimeError):
            wave_emu.frames(lib, [text[:40000]], **kw)


def test_bounds_program_is_clean(tmp_path, sources):
    """AddressSanitizer + UBSan over the match kernel, the literal gather and the trailer kernel with EVERY source of the set in an exactly sized heap block, at level 3
    and at level 1 with min_match 4, at the product's table size: a stand-alone program (tests/emu/wave_bounds_main.cpp), nothing sanitized is loaded into this
    process. (Without -q the program adds level -3 and the other two table sizes: a run by hand, tests/emu/build_wave_bounds.sh.)"""
    exe = str(tmp_path / "wave_bounds")
    subprocess.check_call(["sh", os.path.join(HERE, "emu", "build_wave_bounds.sh"), exe])
    files = []
    for i, (name, raw) in enumerate(sources):
        p = str(tmp_path / ("%03d.bin" % i))
        open(p, "wb").write(raw)
        files.append(p)
    r = subprocess.run([exe, "-q"] + files, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.startswith("ok: %d sources, %d runs" % (len(sources), 2 * len(sources))), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
