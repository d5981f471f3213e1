"""The delta filter of typed seekable streams (python-zstandard_amd/csrc/zhip_seekable_typed.hpp and zhip_seekable_typed_calls.hpp) on the host
wave emulator, against the numpy model of tests/delta_model.py: the split-with-delta body and the three launches of the delta join over the shapes at which
they take another path and over values that wrap and carry, zh_scan_add64, the read plan under the filter, typed ranges of a filtered stream, the marker's
filter bits, the refusals, and the size the filter is there for (libzstd alone). No GPU."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import delta_model as dm
from tests import planes_model as pm
from tests import reflib
from tests import seekable_cases as sc
from tests.test_emu_seekable_typed import ELEMENTS, FRAME, RANGES_K4, UNSUPPORTED, _guarded, _intact

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
T_TYPED = 100                       # the trace's name of typed kernel k: 100 + k
K_SPLIT, K_JOIN, K_SPLIT_DELTA, K_SUMS, K_OFFSETS, K_JOIN_DELTA = 0, 1, 5, 6, 7, 8


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("emu_seekable_delta")), "libzhip_emu_seekable_delta.so")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + EMU, "-w", "-o", out, os.path.join(EMU, "zhemu.cpp"), os.path.join(EMU, "emu_seekable_delta.cpp")])
    lib = C.CDLL(out)
    vp, u64, u32, i32, i64, ci = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_int64, C.c_int
    lib.emu_scan_add64.restype = None; lib.emu_scan_add64.argtypes = [vp]
    lib.emu_delta_split.restype = None; lib.emu_delta_split.argtypes = [vp, u64, u32, u32, vp, u32, vp]
    lib.emu_delta_join.restype = u64; lib.emu_delta_join.argtypes = [vp, vp, vp, u32, u64, u32, u32, u32, vp]
    lib.emu_delta_planes_call.restype = ci; lib.emu_delta_planes_call.argtypes = [ci, ci, u32, vp, u64, u32, u32, vp, vp, u64, vp, vp, vp, vp]
    lib.emu_delta_compress.restype = ci; lib.emu_delta_compress.argtypes = [ci, u32, vp, u64, u32, u32, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp]
    lib.emu_delta_open.restype = ci; lib.emu_delta_open.argtypes = [vp, u64, vp]
    lib.emu_delta_plan.restype = ci; lib.emu_delta_plan.argtypes = [vp, u64, vp, u64, u64, ci, u64, vp, vp, vp, vp, vp]
    lib.emu_delta_check.restype = ci; lib.emu_delta_check.argtypes = [ci, u64, u32, u32, u32, vp, vp]
    lib.emu_typed_grid.restype = u32; lib.emu_typed_grid.argtypes = [ci, u64, u32, u32]
    lib.emu_typed_bound.restype = u64; lib.emu_typed_bound.argtypes = [u64, u32, u32, ci]
    lib.emu_typed_plan.restype = ci; lib.emu_typed_plan.argtypes = [vp, u64, vp, u64, u64, u64, vp, vp, vp, vp, vp]
    lib.emu_typed_ranges.restype = ci; lib.emu_typed_ranges.argtypes = [vp, u64, vp, vp, u64, vp, u64, u64, i64, i32, vp, vp, vp]
    return lib


def _shapes(m):
    """two full groups of m and a last group of 1, 15 and 17 elements (as far as a group holds them) -> the element counts"""
    return sorted({2 * m + min(last, m) for last in dm.LAST_GROUPS})


# ------------------------------------------------------------------------------------------------ the bodies
def test_scan_add64(lib):
    """against a serial sum: low halves that overflow in every lane (two 32-bit scans would lose every carry), full-range values, and a single 1 in lane 0"""
    rng = np.random.default_rng(5)
    for v in (np.full(64, 0xFFFFFFFF, dtype=np.uint64), np.full(64, 0x1FFFFFFFF, dtype=np.uint64) + np.arange(64, dtype=np.uint64), rng.integers(0, 1 << 64, 64, dtype=np.uint64),
              np.array([1] + [0] * 63, dtype=np.uint64)):
        buf = np.concatenate([v, np.zeros(64, dtype=np.uint64)])
        lib.emu_scan_add64(buf.ctypes.data)
        assert (buf[64:] == np.cumsum(v, dtype=np.uint64)).all()
    assert int(np.cumsum(np.full(64, 0xFFFFFFFF, dtype=np.uint64))[1]) >> 32 == 1       # (the case does carry)


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("m", dm.GROUP_SIZES)
def test_split_and_join_bodies(lib, k, m):
    """every value kind on every shape: split-delta is the model's planar bytes, the record table the planes', join-delta of them the source, and the tile-sums
    area behind the join holds the model's tile offsets; guard bytes all around; byte offsets 0, 1 and 3"""
    for elements in _shapes(m):
        for n_kind, kind in enumerate(dm.KINDS):
            src = dm.values(kind, k, elements, m, seed=100 * k + m)
            want = dm.split(src, k, m)
            assert dm.join(want, k, m).tobytes() == src.tobytes()
            off = (0, 1, 3)[(n_kind + elements) % 3]
            _, s, _ = _guarded(src.size, off); s[:] = src
            raw, d, at = _guarded(src.size, (off + 1) % 4 if off else 0)
            planes = dm.planes(src, k, m)
            records = np.zeros((len(planes), 2), dtype=np.uint64)
            grid = lib.emu_typed_grid(1, src.size, k, m)
            lib.emu_delta_split(s.ctypes.data, src.size, k, m, d.ctypes.data, grid, records.ctypes.data)
            assert (d == want).all(), (k, m, elements, kind)
            assert _intact(raw, at, src.size)
            assert all(d[int(o):int(o + ln)].tobytes() == p for (o, ln), p in zip(records, planes))
            raw2, back, at2 = _guarded(src.size, off)
            tiles = lib.emu_delta_join(d.ctypes.data, back.ctypes.data, None, 0, src.size, k, m, grid, None)
            raw3, sums, at3 = _guarded(tiles * 8, 0)
            assert lib.emu_delta_join(d.ctypes.data, back.ctypes.data, None, 0, src.size, k, m, grid, sums.ctypes.data) == tiles
            assert (back == src).all(), (k, m, elements, kind)
            assert _intact(raw2, at2, src.size) and _intact(raw3, at3, tiles * 8)
            assert sums.view(np.uint64).tolist() == dm.tile_offsets(src, k, m), (k, m, elements, kind)


@pytest.mark.parametrize("k", [2, 4, 8])
def test_fewer_waves_than_tiles(lib, k):
    """the grid-stride loops' later trips, and more than 64 tiles in one job (the offsets kernel's carry from trip to trip): one group of 65 * 1 024 + 5
    carrying elements and one of 7, on 1 and on 4 workgroups"""
    m, elements = 65 * 1024 + 5, 65 * 1024 + 5 + 7
    src = dm.values("carry", k, elements, m)
    want = dm.split(src, k, m)
    for grid in (1, 4):
        raw, d, at = _guarded(src.size, 1)
        lib.emu_delta_split(src.ctypes.data, src.size, k, m, d.ctypes.data, grid, None)
        assert (d == want).all() and _intact(raw, at, src.size)
        raw2, back, at2 = _guarded(src.size, 3)
        sums = np.zeros(2 * 66, dtype=np.uint64)                   # (a shorter last group has a group's tiles too)
        assert lib.emu_delta_join(d.ctypes.data, back.ctypes.data, None, 0, src.size, k, m, grid, None) == 2 * 66
        lib.emu_delta_join(d.ctypes.data, back.ctypes.data, None, 0, src.size, k, m, grid, sums.ctypes.data)
        assert (back == src).all() and _intact(raw2, at2, src.size)
        assert sums.tolist() == dm.tile_offsets(src, k, m)


@pytest.mark.parametrize("k", [2, 4, 8])
def test_join_jobs_with_skips_and_trims(lib, k):
    """jobs of 1 ... 2 100 elements that skip 0, 1, 15, 16, 17, 1 023, 1 024, 1 030 and 2 050 of them and trim their first and last element, all in ONE launch:
    every job's output is the slice of its own prefix sums, and nothing else is written"""
    rng = np.random.default_rng(41 + k)
    dt = dm.DTYPES[k]
    jobs, want, planar, at_p, at_d = [], [], [], 0, 0
    for m, skips in ((1, [0]), (16, [0, 1, 15]), (37, [0, 16, 17, 36]), (1030, [0, 15, 1023, 1024, 1029]), (2100, [17, 1030, 2050])):
        for skip in skips:
            for h, t in ((0, 0), (1, 0), (0, 1), (k - 1, k - 1)):
                if skip * k + h + t >= m * k:
                    continue
                d = rng.integers(0, 256, m * k, dtype=np.uint8)
                planar.append(d.reshape(m, k).T.reshape(-1))
                piece = np.cumsum(d.view(dt), dtype=dt).view(np.uint8)[skip * k + h:m * k - t]
                jobs.append((at_p, m, at_d, h, t, skip)); want.append(piece)
                at_p += m * k; at_d += piece.size
    planar = np.concatenate(planar); want = np.concatenate(want)
    table = np.array(jobs, dtype=np.uint64)
    for off, grid in ((0, 8), (1, 3), (3, 1)):
        _, p, _ = _guarded(planar.size, off); p[:] = planar
        raw, d, at = _guarded(want.size, off)
        tiles = lib.emu_delta_join(p.ctypes.data, d.ctypes.data, table.ctypes.data, len(jobs), 0, k, 1, grid, None)
        raw3, sums, at3 = _guarded(tiles * 8, 0)
        lib.emu_delta_join(p.ctypes.data, d.ctypes.data, table.ctypes.data, len(jobs), 0, k, 1, grid, sums.ctypes.data)
        assert (d == want).all(), (k, off)
        assert _intact(raw, at, want.size) and _intact(raw3, at3, tiles * 8)


# ------------------------------------------------------------------------------------------------ the stand-alone calls
def _planes_call(lib, which, via, filt, src, k, m):
    dst = np.full(src.size, 0x5A, dtype=np.uint8)
    trace = np.zeros(16, dtype=np.uint32); words = np.zeros(1, dtype=np.uint64); info = np.zeros(1, dtype=np.uint64); sums = np.zeros(4096, dtype=np.uint64)
    text = C.create_string_buffer(256)
    rc = lib.emu_delta_planes_call(which, via, filt, src.ctypes.data, src.size, k, m, dst.ctypes.data, trace.ctypes.data, 16, words.ctypes.data, info.ctypes.data, sums.ctypes.data, text)
    return rc, dst, trace[:int(words[0])].tolist(), int(info[0]), sums, text.value


def test_planes_calls(lib):
    """filter 0 through the new argument: the old call's bytes, kernels and grids, and no tile-sums area; filter 1: the delta kernels, three launches for the
    join, 8 bytes a tile"""
    k, m = 4, 1025
    src = dm.values("random", k, 3 * m + 17, m, seed=9)
    old = _planes_call(lib, 0, 0, 0, src, k, m)
    grid = old[2][1]
    new = _planes_call(lib, 0, 1, dm.NONE, src, k, m)
    assert old[0] == new[0] == 0 and (old[1] == new[1]).all() and old[2] == new[2] == [T_TYPED + K_SPLIT, grid] and (old[1] == pm.split(src, k, m)).all()
    rc, planar, trace, area, _, _ = _planes_call(lib, 0, 1, dm.DELTA, src, k, m)
    assert rc == 0 and (planar == dm.split(src, k, m)).all() and trace == [T_TYPED + K_SPLIT_DELTA, grid] and area == 0
    old = _planes_call(lib, 1, 0, 0, planar, k, m)
    new = _planes_call(lib, 1, 1, dm.NONE, planar, k, m)
    assert old[0] == new[0] == 0 and (old[1] == new[1]).all() and old[2] == new[2] == [T_TYPED + K_JOIN, grid] and new[3] == 0
    rc, back, trace, area, sums, _ = _planes_call(lib, 1, 1, dm.DELTA, planar, k, m)
    tiles = 4 * 2                                                 # four groups, the short one included, of two tiles
    assert rc == 0 and (back == src).all() and area == tiles * 8
    assert trace == [T_TYPED + K_SUMS, grid, T_TYPED + K_OFFSETS, 4, T_TYPED + K_JOIN_DELTA, grid]
    assert sums[:tiles].tolist() == dm.tile_offsets(src, k, m)


# ------------------------------------------------------------------------------------------------ the whole calls
_built = {}


def _stream(lib, k, checksum, filt=dm.DELTA, via=1, seed=5):
    """(source bytes, the stream the emulated call wrote, the planes' libzstd frames, the kernel trace): sorted ids (k = 4) or running sums"""
    key = (k, checksum, filt, via, seed)
    if key in _built:
        return _built[key]
    rng = np.random.default_rng(seed)
    src = (np.sort(rng.integers(0, 1 << 31, ELEMENTS)) if k == 4 else np.cumsum(rng.integers(0, 1000, ELEMENTS))).astype(dm.DTYPES[k]).view(np.uint8).copy()
    ref = reflib.checker()
    planes = dm.planes(src, k, FRAME) if filt else pm.planes(src, k, FRAME)
    frames = [ref.compress(p, level=3) for p in planes]
    blob = np.frombuffer(b"".join(frames), dtype=np.uint8)
    offs = np.cumsum([0] + [len(f) for f in frames]).astype(np.uint64)
    bound = lib.emu_typed_bound(src.size, FRAME, k, checksum)
    raw, d, at = _guarded(bound, 0)
    status = np.full(2, -1, dtype=np.int32); info = np.zeros(4, dtype=np.uint64); staging = np.zeros(src.size, dtype=np.uint8)
    trace = np.zeros(64, dtype=np.uint32); words = np.zeros(1, dtype=np.uint64)
    rc = lib.emu_delta_compress(via, filt, src.ctypes.data, src.size, FRAME, k, checksum, blob.ctypes.data, offs.ctypes.data, d.ctypes.data, bound, status.ctypes.data, staging.ctypes.data,
                                info.ctypes.data, trace.ctypes.data, 64, words.ctypes.data, None)
    assert rc == 0 and status.tolist() == [0, 0] and int(info[1]) == 0 and _intact(raw, at, bound)
    assert (staging == (dm.split(src, k, FRAME) if filt else pm.split(src, k, FRAME))).all()
    _built[key] = (src, d[:int(info[0])].tobytes(), frames, trace[:int(words[0])].tolist())
    return _built[key]


def _open(lib, stream):
    buf = np.frombuffer(bytes(stream), dtype=np.uint8).copy()
    out = np.zeros(6, dtype=np.uint64)
    return lib.emu_delta_open(buf.ctypes.data, buf.size, out.ctypes.data), out.tolist()


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("checksum", [0, 1])
def test_compress_and_marker(lib, k, checksum):
    """the stream is the model's: libzstd's frames of the FILTERED planes, the marker's word k | 0x100, the table's checksums those of the filtered planar
    content; open reports filter 1"""
    src, stream, frames, trace = _stream(lib, k, checksum)
    planes = dm.planes(src, k, FRAME)
    assert stream == dm.stream_of(frames, planes, k, FRAME, bool(checksum))
    at = sum(len(f) for f in frames)
    assert struct.unpack_from("<I", stream, at + 16)[0] == k | 0x100 and struct.unpack_from("<I", stream, at + 12)[0] == 1
    entries, ck, _ = sc.parse(stream)
    assert ck == bool(checksum) and all(x is None or x == sc.xxh64(p) & 0xFFFFFFFF for (_, _, x), p in zip(entries, planes))
    assert trace[0] == T_TYPED + K_SPLIT_DELTA
    assert _open(lib, stream) == (0, [0, k, FRAME, 4 * k + 1, ELEMENTS * k, dm.DELTA])


def test_marker_verdicts(lib):
    src, stream, frames, _ = _stream(lib, 4, 0)
    at = sum(len(f) for f in frames) + 16
    n = 4 * 4                                                     # the marker's frame index
    for word, verdict in ((4 | 0x100, 0), (4, 0), (4 | 0x200, 20), (4 | 0x100 | 1 << 16, 20), (4 | 1 << 16, 20), (4 | 1 << 31, 20), (3 | 0x100, 20)):
        s = bytearray(stream); struct.pack_into("<I", s, at, word)
        code, out = _open(lib, s)
        assert code == verdict, hex(word)
        assert out == ([0, 4, FRAME, n + 1, ELEMENTS * 4, word >> 8] if not verdict else [n, 0, 0, 0, 0, 0]), hex(word)


def test_unfiltered_stream_is_the_old_calls(lib):
    """filter 0 through the new argument against the call without it: the same bytes, the same kernels on the same grids -- and today's marker"""
    for k, checksum in ((2, 0), (4, 1)):
        src, old, frames, old_trace = _stream(lib, k, checksum, filt=dm.NONE, via=0)
        _, new, _, new_trace = _stream(lib, k, checksum, filt=dm.NONE, via=1)
        assert old == new == pm.stream_of(frames, pm.planes(src, k, FRAME), k, FRAME, bool(checksum))
        assert old_trace == new_trace and old_trace[0] == T_TYPED + K_SPLIT
        assert _open(lib, new) == (0, [0, k, FRAME, 4 * k + 1, ELEMENTS * k, dm.NONE])


def _plan(lib, stream, rg, limit=0, force_none=0):
    buf = np.frombuffer(bytes(stream), dtype=np.uint8).copy()
    table = np.array([(o, n, 0) for o, n in rg], dtype=np.uint64).reshape(-1, 3)
    cap = 64
    planar = np.zeros((cap, 3), dtype=np.uint64); jobs = np.zeros((cap, 7), dtype=np.uint64); passes = np.zeros((cap, 2), dtype=np.uint64)
    owner = np.zeros((len(rg), 2), dtype=np.uint64); counts = np.zeros(3, dtype=np.uint64)
    assert lib.emu_delta_plan(buf.ctypes.data, buf.size, table.ctypes.data, len(rg), limit, force_none, cap, planar.ctypes.data, jobs.ctypes.data, passes.ctypes.data, owner.ctypes.data,
                              counts.ctypes.data) == 0
    q, j, p = (int(x) for x in counts)
    return planar[:q].tolist(), jobs[:j].tolist(), passes[:p].tolist(), owner.tolist()


def test_plan_against_the_model(lib):
    """one range at a time -- inside one element, across a group boundary, whole groups, empty: the planar ranges and the jobs are the model's; a partly covered
    group is k planar ranges that start at the planes' starts with skip = lo; with filter 0 the old plan, field for field"""
    _, stream, _, _ = _stream(lib, 4, 0)
    group_bytes = FRAME * 4
    for off, n in RANGES_K4:
        planar, jobs, passes, owner = _plan(lib, stream, [(off, n)])
        want_ranges, want_jobs = dm.plan(ELEMENTS, 4, FRAME, off, n)
        assert [(a, b) for a, b, _ in planar] == want_ranges, (off, n)
        assert [(m, h, t, skip) for _, _, m, _, h, t, skip in jobs] == want_jobs, (off, n)
        assert len(planar) <= 2 * 4 + 1 and owner == [[0, len(planar)]] and len(passes) == (1 if n else 0)
        at = 0
        for a, b, p in planar:                  # back to back in the planar buffer
            assert p == at
            at += b
        if n and (off // 4) % FRAME and (off // 4) // FRAME < 3:       # the range starts inside a full group: that group's k ranges start at its planes' starts
            g, lo = (off // 4) // FRAME, (off // 4) % FRAME
            assert [a for a, _, _ in planar[:4]] == [g * group_bytes + p * FRAME for p in range(4)] and jobs[0][6] == lo and jobs[0][2] == planar[0][1]
        # the same stream planned without a filter: what the typed plan says, and no skip anywhere
        planar0, jobs0, passes0, owner0 = _plan(lib, stream, [(off, n)], force_none=1)
        want_ranges0, want_jobs0 = pm.plan(ELEMENTS, 4, FRAME, off, n)
        assert [(a, b) for a, b, _ in planar0] == want_ranges0 and [(m, h, t, skip) for _, _, m, _, h, t, skip in jobs0] == [j + (0,) for j in want_jobs0]
    # an unfiltered stream through the entry point of before and through this one: the same six words per job
    _, plain, _, _ = _stream(lib, 4, 0, filt=dm.NONE)
    buf = np.frombuffer(plain, dtype=np.uint8).copy()
    rg = [(o, n) for o, n in RANGES_K4]
    table = np.array([(o, n, 0) for o, n in rg], dtype=np.uint64)
    planar = np.zeros((64, 3), dtype=np.uint64); jobs = np.zeros((64, 6), dtype=np.uint64); passes = np.zeros((64, 2), dtype=np.uint64)
    owner = np.zeros((len(rg), 2), dtype=np.uint64); counts = np.zeros(3, dtype=np.uint64)
    assert lib.emu_typed_plan(buf.ctypes.data, buf.size, table.ctypes.data, len(rg), 0, 64, planar.ctypes.data, jobs.ctypes.data, passes.ctypes.data, owner.ctypes.data, counts.ctypes.data) == 0
    planar1, jobs1, passes1, owner1 = _plan(lib, plain, rg)
    q, j, p = (int(x) for x in counts)
    assert planar[:q].tolist() == planar1 and [x[:6] for x in jobs1] == jobs[:j].tolist() and all(x[6] == 0 for x in jobs1) and passes[:p].tolist() == passes1


def _read(lib, stream, planar_content, rg, limit=0, code_frame=-1, code=0):
    buf = np.frombuffer(bytes(stream), dtype=np.uint8).copy()
    table = np.zeros((max(len(rg), 1), 3), dtype=np.uint64)
    at = 0
    for i, (o, n) in enumerate(rg):
        table[i] = (o, n, at); at += n
    raw, d, dat = _guarded(at, 1)
    status = np.full(2 + 2 * len(rg), -1, dtype=np.int32); stats = np.zeros(7, dtype=np.uint64)
    rc = lib.emu_typed_ranges(buf.ctypes.data, buf.size, planar_content.ctypes.data, table.ctypes.data, len(rg), d.ctypes.data, at, limit, code_frame, code, status.ctypes.data,
                              stats.ctypes.data, None)
    assert _intact(raw, dat, at)
    return rc, [d[int(table[i, 2]):int(table[i, 2] + table[i, 1])].tobytes() for i in range(len(rg))], status.tolist(), [int(x) for x in stats]


def _ranges(k, size):
    rg = [(o * k // 4, n * k // 4) if k != 4 else (o, n) for o, n in RANGES_K4]
    return [(o, min(n, size - o)) for o, n in rg]


@pytest.mark.parametrize("k", [2, 4, 8])
def test_typed_ranges(lib, k):
    """the elements read back through zsk_typed_ranges equal the source's slice: every range singly, all in one call"""
    src, stream, _, _ = _stream(lib, k, 1)
    content = dm.split(src, k, FRAME)
    rg_all = _ranges(k, src.size)
    for one in rg_all:
        rc, got, status, stats = _read(lib, stream, content, [one])
        assert rc == 0 and status == [0, 0, 0, 0]
        assert got[0] == src[one[0]:one[0] + one[1]].tobytes(), one
    rng = np.random.default_rng(11)
    many = list(rg_all)
    while len(many) < 40:
        o = int(rng.integers(0, src.size)); many.append((o, int(rng.integers(0, min(src.size - o, 3 * FRAME * k) + 1))))
    rc, got, status, stats = _read(lib, stream, content, many)
    assert rc == 0 and status == [0] * (2 + 2 * 40) and stats[4] == 1
    for (o, n), g in zip(many, got):
        assert g == src[o:o + n].tobytes(), (o, n)


def test_scratch_limit_forces_passes(lib):
    """under a limit of 20 000 bytes (a group is 16 384 planar bytes) the whole content goes in passes; under a limit below one group -- two passes for a range
    over two groups -- the planar buffer is one group, and a piece above the limit is alone in its pass"""
    src, stream, _, _ = _stream(lib, 4, 0)
    content = dm.split(src, 4, FRAME)
    rg = [(5, src.size - 7), (3 * FRAME * 4 - 2, 100), (7, 9)]
    for limit in (20000, 1000):
        rc, got, status, stats = _read(lib, stream, content, rg, limit=limit)
        assert rc == 0 and status == [0] * 8
        assert [g == src[o:o + n].tobytes() for (o, n), g in zip(rg, got)] == [True] * 3
    assert stats[5] == FRAME * 4
    # group 0 from element 1 is fetched whole under the filter (4 096 elements), so the first pass holds a whole group
    planar, jobs, passes, owner = _plan(lib, stream, rg, 20000)
    assert [int(b) for b, _ in passes][:2] == [FRAME * 4, FRAME * 4] and jobs[0][2] == FRAME and jobs[0][6] == 1
    two = [(FRAME * 4 - 8, 16)]                                   # the last two elements of group 0, the first two of group 1
    planar, jobs, passes, owner = _plan(lib, stream, two, 1000)
    assert len(passes) == 2 and [int(b) for b, _ in passes] == [FRAME * 4, 2 * 4] and [j[6] for j in jobs] == [FRAME - 2, 0]
    rc, got, status, stats = _read(lib, stream, content, two, limit=1000)
    assert rc == 0 and stats[4] == 2 and got[0] == src[FRAME * 4 - 8:FRAME * 4 + 8].tobytes()


def test_one_damaged_plane_frame(lib):
    """plane frame 6 (group 1, plane 2) fails with 20: exactly the ranges that need group 1 report {20, 6}; the others are right, bytes included"""
    src, stream, _, _ = _stream(lib, 4, 1)
    content = dm.split(src, 4, FRAME)
    g = FRAME * 4
    rg = [(10, 100), (g - 2, 4), (g, g), (2 * g + 1, 50), (0, src.size), (g + 77, 0), (2 * g - 1, 1), (2 * g, 1), (3 * g, 148)]
    touches = [o < 2 * g and o + n > g and n > 0 for o, n in rg]
    for limit in (0, 20000):
        rc, got, status, stats = _read(lib, stream, content, rg, limit=limit, code_frame=6, code=20)
        assert rc == 0 and status[:2] == [20, 1]
        for r, ((o, n), t) in enumerate(zip(rg, touches)):
            assert status[2 + 2 * r:4 + 2 * r] == ([20, 6] if t else [0, 0]), r
            if not t:
                assert got[r] == src[o:o + n].tobytes(), r


def test_refusals(lib):
    """an unknown filter, and a filter with element size 1: UNSUPPORTED, nothing launched, nothing written"""
    t = C.create_string_buffer(256); words = np.zeros(1, dtype=np.uint64)
    check = lambda which, size, frame, k, filt: (lib.emu_delta_check(which, size, frame, k, filt, words.ctypes.data, t), int(words[0]))
    for filt in (2, 3, 0x100, 0xFFFFFFFF):
        for k in (1, 2, 4, 8):
            assert check(0, 4096, 1024, k, filt) == (UNSUPPORTED, 0) and b"filter" in t.value
        assert check(1, 4096, 1024, 4, filt) == (UNSUPPORTED, 0) and b"filter" in t.value
    assert check(0, 4096, 1024, 1, dm.DELTA) == (UNSUPPORTED, 0) and b"element size" in t.value
    assert check(1, 4096, 1024, 1, dm.DELTA) == (UNSUPPORTED, 0)
    assert check(0, 4097, 1024, 2, dm.DELTA) == (UNSUPPORTED, 0) and check(1, 4096, 0, 2, dm.DELTA) == (UNSUPPORTED, 0)


# ------------------------------------------------------------------------------------------------ what the filter is for
def test_size_claim_with_libzstd_alone():
    """int64 running sums of uniform [0, 1000), four groups of 131 072 (seed 7): libzstd's level-3 frames of the filtered planes sum to at most 0.85 of those of
    the unfiltered planes (libzstd alone gives 0.762). The package's host model is what is measured; it is also checked against tests/delta_model.py"""
    import zstandard_amd.seekable as zs
    G = 131072
    x = np.cumsum(np.random.default_rng(7).integers(0, 1000, 4 * G)).astype("<i8")
    data = x.tobytes()
    ref = reflib.checker()
    total = {}
    for filt in (None, "delta"):
        planar = zs.elements_to_planes(data, 8, G, filter=filt)
        assert zs.planes_to_elements(planar, 8, G, filter=filt) == data
        assert planar == (dm.split(x.view(np.uint8), 8, G) if filt else pm.split(x.view(np.uint8), 8, G)).tobytes()
        total[filt] = sum(len(ref.compress(planar[at:at + G], level=3)) for at in range(0, len(planar), G))
    print("planes %d bytes, delta + planes %d bytes: %.3f" % (total[None], total["delta"], total["delta"] / total[None]))
    assert total["delta"] <= 0.85 * total[None]
    with pytest.raises(ValueError):
        zs.elements_to_planes(data, 8, G, filter="xor")


def test_sanitizer_program(tmp_path):
    """tests/emu/delta_planes_main.cpp under AddressSanitizer and UBSan: the split, sums, offsets and join bodies over the shapes above, heap buffers sized exactly"""
    exe = os.path.join(str(tmp_path), "delta_planes_asan")
    subprocess.check_call(["sh", os.path.join(EMU, "build_asan_planes.sh"), "delta_planes_main.cpp", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert b"cases" in r.stdout
