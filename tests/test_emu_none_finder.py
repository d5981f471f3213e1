"""match_finder="none" (ZHIP_FINDER_NONE: ze_none_body, one wave per source, the source itself read as the block's literals) on the 64-fiber host emulator with the
trailer kernel behind it (tests/emu/emu_none_finder.cpp). Its frames are libzstd's: every frame is compared byte for byte with what libzstd 1.5.7's
ZSTD_compressSequences writes for the list that is only the block delimiter (RefZstd.compress_sequences(data, [], len(data))) and with what the sequence loader and the
entropy kernel write for count 0 (the path that exists without this finder), and is decompressed by libzstd. Refusals, the launch plan, the size claim of the typed
bf16 stream (libzstd alone), and the stand-alone bounds program."""
import os
import subprocess

import numpy as np
import pytest

from tests import none_emu, reflib
from tests import none_sources as ns

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return none_emu.build(tmp_path_factory.mktemp("emu_none_finder"))


@pytest.fixture(scope="module")
def aimed(corpus):
    return ns.aimed_sources(corpus)


@pytest.fixture(scope="module")
def classes(corpus):
    return ns.corpus_class_sources(corpus)


def _flags(content_size, checksum):
    return (reflib.F_CONTENTSIZE if content_size else 0) | (reflib.F_CHECKSUM if checksum else 0) | reflib.F_DICTID


def _hold_to_libzstd(lib, ref, named, level, content_size=True, checksum=False, decode=True, **params):
    raws = [r for _, r in named]
    got, st, modes = none_emu.frames(lib, raws, level=level, checksum=checksum, content_size=content_size, **params)
    for (name, raw), f, s, mode in zip(named, got, st, modes):
        what = (name, level, content_size, checksum, params)
        assert s == 0, what
        assert mode == (1 if len(raw) < 7 else 4), what
        assert f == ref.compress_sequences(raw, [], len(raw), level=level, flags=_flags(content_size, checksum), **params), what
        if decode:
            assert ref.decompress(f, len(raw)) == raw, what
    return got


def test_aimed_sources_aim_where_they_should(ref, aimed):
    """the property first, from libzstd's own frame"""
    for name, raw, prop in aimed:
        ns.check_property(name, ref.compress_sequences(raw, [], len(raw), level=3), prop)
    assert ns.huffman_depth(ns.skewed_256()) > 11
    assert [len(r) for _, r, _ in aimed[:len(ns.SIZES)]] == list(ns.SIZES)


@pytest.mark.parametrize("level", [3, 1, 4, -1])
def test_frames_are_libzstds_literals_only_frames(lib, ref, aimed, classes, level):
    named = [(n, r) for n, r, _ in aimed] + classes
    if level == 4:
        named = [(n, r) for n, r in named if len(r) > 16384]                               # (level 4's row for smaller sources is greedy: refused, test_refusals)
    got = _hold_to_libzstd(lib, ref, named, level)
    if level == -1:                                                                        # raw literals: every block comes out raw
        from tests import entropy_families
        assert all(entropy_families.frame_census(f)["block"] == "raw" for f in got)
    # the other oracle: the loader with empty lists and the entropy kernel, the path that exists without this finder
    small = [(n, r) for n, r in named if len(r) <= 41000 or n in ("text 131072", "bf16 exponent plane")]
    a, sta, _ = none_emu.frames(lib, [r for _, r in small], level=level)
    b, stb, _ = none_emu.frames(lib, [r for _, r in small], level=level, path="sequences")
    assert sta == stb and a == b


@pytest.mark.parametrize("content_size,checksum", [(True, True), (False, False), (False, True)], ids=["checksum", "no content size", "checksum, no content size"])
def test_frame_flags(lib, ref, aimed, classes, content_size, checksum):
    named = [(n, r) for n, r, _ in aimed] + classes[:14]
    _hold_to_libzstd(lib, ref, named, 3, content_size=content_size, checksum=checksum)


def test_explicit_parameters_and_magicless(lib, ref, aimed, classes):
    named = [(n, r) for n, r, _ in aimed] + classes[:14]
    _hold_to_libzstd(lib, ref, named, 3, window_log=17, strategy=1)
    raws = [r for _, r in named]
    got, st, _ = none_emu.frames(lib, raws, level=3, magicless=True)
    for (name, raw), f, s in zip(named, got, st):
        assert s == 0 and f == ref.compress_sequences(raw, [], len(raw), level=3, format=1), name


def test_output_is_independent_of_the_grid_and_the_chunk(lib, aimed):
    raws = [r for _, r, _ in aimed if len(r) <= 41000]
    base, st, _ = none_emu.frames(lib, raws, level=3, checksum=True)
    assert not any(st)
    one, st1, _ = none_emu.frames(lib, raws, level=3, checksum=True, blocks=1)             # one wave takes every source in turn
    rev, st2, _ = none_emu.frames(lib, raws[::-1], level=3, checksum=True, blocks=5)
    cut, st3, _ = none_emu.frames(lib, raws, level=3, checksum=True, echunk=7)             # chunks of 7: the counter starts again, meta is chunk-local
    assert not any(st1 + st2 + st3) and one == base and rev[::-1] == base and cut == base


def test_refusals(lib, ref, corpus):
    text = corpus.frame_bytes(9)
    big = ns.refused_source(corpus)
    assert len(big) == 131073
    raws = [text[:5000], big, text[:70000], (text * 3)[:300000], b"abc", text]
    got, st, modes = none_emu.frames(lib, raws, level=3)
    assert st == [0, 40, 0, 40, 0, 0] and got[1] == b"" and got[3] == b"" and modes == [4, 2, 4, 2, 1, 4]      # several blocks: refused at their own index
    for i in (0, 2, 4, 5):
        assert got[i] == ref.compress_sequences(raws[i], [], len(raws[i]), level=3), i
    got, st, _ = none_emu.frames(lib, [text[:40000], text[:16384], text[:16385]], level=4)                     # level 4: greedy at 16 KiB and below
    assert st == [0, 40, 0] and got[2] == ref.compress_sequences(text[:16385], [], 16385, level=4)
    assert none_emu.frames(lib, [text[:40000], text[:900]], level=3, window_log=10)[1] == [40, 0]             # a window that does not cover the source
    for kw in (dict(level=5), dict(level=3, strategy=3, search_log=4), dict(level=3, dictionary=True)):      # refused by the call
        with pytest.raises(RuntimeError):
            none_emu.frames(lib, [text[:40000]], **kw)


def test_plan(lib):
    """ze_none_plan: a chunk is 65 536 sources (what the context's meta buffer holds under every other finder), the grid is the entropy kernel's, capped by the chunk"""
    chunk = 65536
    assert none_emu.plan(lib, 1) == (1, 1, 16)
    assert none_emu.plan(lib, chunk) == (chunk, 256 * 14, chunk * 16)
    assert none_emu.plan(lib, chunk + 1) == (chunk, 256 * 14, chunk * 16)
    assert none_emu.plan(lib, 1000, num_cu=8, e2_per_cu=4) == (1000, 32, 16000)
    assert none_emu.plan(lib, 1000, echunk=100) == (100, 100, 1600)


def test_typed_bf16_stream_is_smaller_without_a_search(ref):
    """with libzstd alone: 1 MiB of bf16 N(0, 0.02) as byte planes of 131 072 -- the literals-only frames together are smaller than level 3's. With frame equality
    (above, and on the device) this fixes the product's sizes."""
    planes = np.frombuffer(ns.bf16_bytes(524288), dtype=np.uint8).reshape(-1, 2)
    level3 = none = 0
    for g in range(4):
        for p in range(2):
            plane = planes[g * 131072:(g + 1) * 131072, p].tobytes()
            level3 += len(ref.compress(plane, level=3))
            none += len(ref.compress_sequences(plane, [], len(plane), level=3))
    assert none < level3, (none, level3)
    assert 0.93 < none / level3 < 0.96, (none, level3)                                      # (measured 702 184 against 742 138)


def test_bounds_program_is_clean(tmp_path, aimed):
    """AddressSanitizer + UBSan over the literals-only kernel and the trailer kernel with EVERY aimed source in an exactly sized heap block and every destination an
    exactly zhip_compress_bound-sized one, at levels 3 and -1, with no arena and no workspace: a stand-alone program (tests/emu/none_bounds_main.cpp), nothing
    sanitized is loaded into this process. (Without -q the program adds level 1: a run by hand, tests/emu/build_none_bounds.sh.)"""
    exe = str(tmp_path / "none_bounds")
    subprocess.check_call(["sh", os.path.join(HERE, "emu", "build_none_bounds.sh"), exe])
    files = []
    for i, (name, raw, _) in enumerate(aimed):
        p = str(tmp_path / ("%03d.bin" % i))
        open(p, "wb").write(raw)
        files.append(p)
    r = subprocess.run([exe, "-q"] + files, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.startswith("ok: %d sources, %d runs" % (len(aimed), 2 * len(aimed))), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
