"""Typed seekable streams (one byte plane per frame; python-zstandard_amd/csrc/zhip_seekable_typed.hpp and zhip_seekable_typed_calls.hpp) on the host wave
emulator, against the numpy model of tests/planes_model.py: the split and join bodies over the shapes at which they take another path, the seal, and the whole
calls -- typed compress with libzstd's frames of the planes, the open call's verdicts, typed ranges in element order, passes under a scratch limit, one damaged
plane frame, the refusals -- over the emulator backend. No GPU."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import planes_model as pm
from tests import reflib
from tests import seekable_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
UNSUPPORTED = 6
GUARD = 64


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("emu_seekable_typed")), "libzhip_emu_seekable_typed.so")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + EMU, "-w", "-o", out, os.path.join(EMU, "zhemu.cpp"), os.path.join(EMU, "emu_seekable_typed.cpp")])
    lib = C.CDLL(out)
    vp, u64, u32, i32, i64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_int64
    lib.emu_planes_split.restype = None; lib.emu_planes_split.argtypes = [vp, u64, u32, u32, vp, u32, vp]
    lib.emu_planes_join.restype = None; lib.emu_planes_join.argtypes = [vp, vp, vp, u32, u64, u32, u32, u32]
    lib.emu_typed_seal.restype = u64; lib.emu_typed_seal.argtypes = [vp, u64, u64, u32, u32, u32, u32, u32, vp]
    lib.emu_typed_bound.restype = u64; lib.emu_typed_bound.argtypes = [u64, u32, u32, C.c_int]
    lib.emu_typed_grid.restype = u32; lib.emu_typed_grid.argtypes = [C.c_int, u64, u32, u32]
    lib.emu_typed_compress.restype = C.c_int; lib.emu_typed_compress.argtypes = [vp, u64, u32, u32, u32, vp, vp, vp, u64, vp, vp, vp, vp, vp]
    lib.emu_typed_plain.restype = u64; lib.emu_typed_plain.argtypes = [vp, u64, u32, u32, vp, vp, C.c_int, vp, u64, vp]
    lib.emu_typed_open.restype = C.c_int; lib.emu_typed_open.argtypes = [vp, u64, vp]
    lib.emu_typed_check.restype = C.c_int; lib.emu_typed_check.argtypes = [C.c_int, u64, u32, u32, C.c_int, vp]
    lib.emu_typed_plan.restype = C.c_int; lib.emu_typed_plan.argtypes = [vp, u64, vp, u64, u64, u64, vp, vp, vp, vp, vp]
    lib.emu_typed_ranges.restype = C.c_int; lib.emu_typed_ranges.argtypes = [vp, u64, vp, vp, u64, vp, u64, u64, i64, i32, vp, vp, vp]
    return lib


def _guarded(n, offset, fill=0x5A):
    """(the whole buffer, the view of n bytes at `offset` bytes behind a 64-byte aligned guard)"""
    raw = np.full(n + 2 * GUARD + 64 + offset, fill, dtype=np.uint8)
    skew = (-raw.ctypes.data) % 64
    at = skew + GUARD + offset
    return raw, raw[at:at + n], at


def _intact(raw, at, n, fill=0x5A):
    return (raw[:at] == fill).all() and (raw[at + n:] == fill).all()


def _data(n_bytes, seed):
    return np.random.default_rng(seed).integers(0, 256, n_bytes, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ the bodies
@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("m", pm.GROUP_SIZES)
def test_split_and_join_bodies(lib, k, m):
    """two groups of m elements and a shorter last one (where m > 1), at source / staging / destination offsets 0, 1 and 3; the record table; guard bytes"""
    elements = 2 * m + (max(1, m // 3) if m > 1 else 1)
    src = _data(elements * k, 100 * k + m)
    want = pm.split(src, k, m)
    n_frames = len(pm.groups(elements, m)) * k
    for off in (0, 1, 3):
        _, s, _ = _guarded(src.size, off); s[:] = src
        raw, d, at = _guarded(src.size, (off + 1) % 4 if off else 0)
        records = np.zeros((n_frames, 2), dtype=np.uint64)
        grid = lib.emu_typed_grid(1, src.size, k, m)
        lib.emu_planes_split(s.ctypes.data, src.size, k, m, d.ctypes.data, grid, records.ctypes.data)
        assert (d == want).all(), (k, m, off)
        assert _intact(raw, at, src.size)
        planes = pm.planes(src, k, m)
        assert [int(x) for x in records[:, 1]] == [len(p) for p in planes]
        assert all(d[int(o):int(o + ln)].tobytes() == p for (o, ln), p in zip(records, planes))
        raw2, back, at2 = _guarded(src.size, off)
        lib.emu_planes_join(d.ctypes.data, back.ctypes.data, None, 0, src.size, k, m, grid)
        assert (back == src).all(), (k, m, off)
        assert _intact(raw2, at2, src.size)


@pytest.mark.parametrize("k", [2, 4, 8])
def test_fewer_waves_than_tiles(lib, k):
    """the grid-stride loop's second trip: 3 groups of 1 025 elements are 6 tiles, on 1 and on 4 workgroups"""
    m, elements = 1025, 3 * 1025
    src = _data(elements * k, 7 + k)
    want = pm.split(src, k, m)
    for grid in (1, 4):
        raw, d, at = _guarded(src.size, 1)
        lib.emu_planes_split(src.ctypes.data, src.size, k, m, d.ctypes.data, grid, None)
        assert (d == want).all() and _intact(raw, at, src.size)
        raw2, back, at2 = _guarded(src.size, 3)
        lib.emu_planes_join(d.ctypes.data, back.ctypes.data, None, 0, src.size, k, m, grid)
        assert (back == src).all() and _intact(raw2, at2, src.size)


def _trims(k):
    return [(h, t) for h in range(k) for t in range(k)] if k == 4 else [(0, 0), (1, 0), (0, 1), (k - 1, k - 1)]


@pytest.mark.parametrize("k", [2, 4, 8])
def test_join_jobs_with_trims(lib, k):
    """jobs of 1, 16, 37 and 1 030 elements under every trim pair (k = 4) or the four corner pairs, all in ONE launch, the destinations back to back"""
    jobs, want, planar, at_p, at_d = [], [], [], 0, 0
    rng = np.random.default_rng(31 + k)
    for m in (1, 16, 37, 1030):
        for h, t in _trims(k):
            if h + t >= m * k:
                continue
            el = rng.integers(0, 256, (m, k), dtype=np.uint8)
            planar.append(el.T.reshape(-1))
            piece = el.reshape(-1)[h:m * k - t]
            jobs.append((at_p, m, at_d, h, t)); want.append(piece)
            at_p += m * k; at_d += piece.size
    planar = np.concatenate(planar); want = np.concatenate(want)
    table = np.array(jobs, dtype=np.uint64)
    for off, grid in ((0, 8), (1, 3), (3, 1)):
        _, p, _ = _guarded(planar.size, off); p[:] = planar
        raw, d, at = _guarded(want.size, off)
        lib.emu_planes_join(p.ctypes.data, d.ctypes.data, table.ctypes.data, len(jobs), 0, k, 1, grid)
        assert (d == want).all(), (k, off)
        assert _intact(raw, at, want.size)


@pytest.mark.parametrize("checksum", [0, 1])
def test_seal_alone(lib, checksum):
    """the two seal kernels behind a plain table of n entries: the model's bytes where the capacity holds the marker and its entry, 70 and no byte one short"""
    for n in (0, 1, 5, 300):
        frames = [bytes([i & 0xFF]) * (i % 7 + 1) for i in range(n)]
        contents = [b"x" * (i + 1) for i in range(n)]
        plain = sc.stream_of(frames, contents, bool(checksum))
        want = pm.stream_of(frames, contents, 4, 4096, bool(checksum))
        for short in (0, 1):
            cap = len(want) - short
            raw, d, at = _guarded(cap, 1)
            d[:len(plain)] = np.frombuffer(plain, dtype=np.uint8)
            status = np.full(2, -1, dtype=np.int32)
            size = lib.emu_typed_seal(d.ctypes.data, cap, len(plain), n, checksum, 4, 4096, 3, status.ctypes.data)
            assert _intact(raw, at, cap)
            if short:
                assert size == 0 and status.tolist() == [70, max(n - 1, 0)]
                assert d[:len(plain)].tobytes() == plain
            else:
                assert size == len(want) and d.tobytes() == want and status.tolist() == [-1, -1]


# ------------------------------------------------------------------------------------------------ the whole calls
FRAME = 4096
ELEMENTS = 3 * FRAME + 37


def _text():
    return C.create_string_buffer(256)


_built = {}


def _typed_stream(lib, k, checksum, seed=5):
    """(source bytes, the typed stream the emulated call wrote, the planes' libzstd frames)"""
    key = (k, checksum, seed)
    if key in _built:
        return _built[key]
    rng = np.random.default_rng(seed)
    src = (rng.normal(0, 0.02, ELEMENTS).astype(np.float32).view(np.uint8) if k == 4 else rng.integers(0, 50000, ELEMENTS * k // 4 + 1, dtype=np.int32).view(np.uint8))[:ELEMENTS * k].copy()
    ref = reflib.checker()
    planes = pm.planes(src, k, FRAME)
    frames = [ref.compress(p, level=3) for p in planes]
    blob = np.frombuffer(b"".join(frames), dtype=np.uint8)
    offs = np.cumsum([0] + [len(f) for f in frames]).astype(np.uint64)
    bound = lib.emu_typed_bound(src.size, FRAME, k, checksum)
    want = pm.stream_of(frames, planes, k, FRAME, bool(checksum))
    assert bound >= len(want)
    raw, d, at = _guarded(bound, 0)
    status = np.full(2, -1, dtype=np.int32); info = np.zeros(4, dtype=np.uint64)
    staging = np.zeros(src.size, dtype=np.uint8); records = np.zeros((len(frames), 2), dtype=np.uint64)
    rc = lib.emu_typed_compress(src.ctypes.data, src.size, FRAME, k, checksum, blob.ctypes.data, offs.ctypes.data, d.ctypes.data, bound, status.ctypes.data, staging.ctypes.data,
                                records.ctypes.data, info.ctypes.data, None)
    assert rc == 0 and status.tolist() == [0, 0] and int(info[1]) == 0
    assert int(info[2]) == src.size                                 # the staging area: the source's bytes
    assert _intact(raw, at, bound)
    assert (staging == pm.split(src, k, FRAME)).all()
    _built[key] = (src, d[:int(info[0])].tobytes(), frames, blob, offs)
    return _built[key]


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("checksum", [0, 1])
def test_typed_compress(lib, k, checksum):
    src, stream, frames, blob, offs = _typed_stream(lib, k, checksum)
    planes = pm.planes(src, k, FRAME)
    entries, ck, table_at = sc.parse(stream)
    assert ck == bool(checksum) and len(entries) == 4 * k + 1
    at = 0
    for i, (c, d, x) in enumerate(entries[:-1]):
        assert stream[at:at + c] == frames[i], "plane frame %d is not libzstd's" % i
        assert d == len(planes[i]) and (x is None or x == sc.xxh64(planes[i]) & 0xFFFFFFFF)
        at += c
    assert entries[-1] == (24, 0, pm.XXH_EMPTY if checksum else None)
    assert stream[at:at + 24] == pm.marker(k, FRAME) and at + 24 == table_at
    assert stream == pm.stream_of(frames, planes, k, FRAME, bool(checksum))
    # one byte short: 70, and nothing written at all
    cap = len(stream) - 1
    raw, d, dat = _guarded(cap, 3)
    status = np.full(2, -1, dtype=np.int32); info = np.zeros(4, dtype=np.uint64)
    rc = lib.emu_typed_compress(src.ctypes.data, src.size, FRAME, k, checksum, blob.ctypes.data, offs.ctypes.data, d.ctypes.data, cap, status.ctypes.data, None, None, info.ctypes.data, None)
    assert rc == 0 and int(status[0]) == 70 and int(info[0]) == 0
    assert (raw == 0x5A).all()
    # and the capacity that just holds it
    raw, d, dat = _guarded(len(stream), 3)
    rc = lib.emu_typed_compress(src.ctypes.data, src.size, FRAME, k, checksum, blob.ctypes.data, offs.ctypes.data, d.ctypes.data, len(stream), status.ctypes.data, None, None, info.ctypes.data, None)
    assert rc == 0 and status.tolist() == [0, 0] and d.tobytes() == stream and _intact(raw, dat, len(stream))


def test_typed_compress_of_nothing(lib):
    """no elements: the marker and a table of one entry"""
    offs = np.zeros(1, dtype=np.uint64)
    raw, d, at = _guarded(64, 0)
    status = np.full(2, -1, dtype=np.int32); info = np.zeros(4, dtype=np.uint64)
    rc = lib.emu_typed_compress(None, 0, FRAME, 2, 0, None, offs.ctypes.data, d.ctypes.data, 64, status.ctypes.data, None, None, info.ctypes.data, None)
    assert rc == 0 and status.tolist() == [0, 0]
    stream = d[:int(info[0])].tobytes()
    assert stream == pm.stream_of([], [], 2, FRAME, False)
    out = np.zeros(5, dtype=np.uint64)
    assert lib.emu_typed_open(d.ctypes.data, len(stream), out.ctypes.data) == 0 and out.tolist() == [0, 2, FRAME, 1, 0]


def test_element_size_1_is_the_plain_call(lib):
    src = _data(5 * 4096 + 17, 3)
    n = 6
    sizes = np.array([20 + i for i in range(n)], dtype=np.uint64); given = np.zeros(n, dtype=np.int32)
    outs = []
    for via in (0, 1):
        for checksum in (0, 1):
            d = np.full(4096, 0x5A, dtype=np.uint8); status = np.full(2, -1, dtype=np.int32)
            size = lib.emu_typed_plain(src.ctypes.data, src.size, 4096, checksum, sizes.ctypes.data, given.ctypes.data, via, d.ctypes.data, d.size, status.ctypes.data)
            assert status.tolist() == [0, 0]
            outs.append(d[:size].tobytes())
    assert outs[0] == outs[2] and outs[1] == outs[3] and len(sc.parse(outs[0])[0]) == n


def _open(lib, stream):
    buf = np.frombuffer(bytes(stream), dtype=np.uint8).copy()
    out = np.zeros(5, dtype=np.uint64)
    return lib.emu_typed_open(buf.ctypes.data, buf.size, out.ctypes.data), out.tolist()


def test_open_verdicts(lib):
    src, stream, frames, _, _ = _typed_stream(lib, 4, 1)
    assert _open(lib, stream) == (0, [0, 4, FRAME, 17, ELEMENTS * 4])
    contents = [b"a" * 100, b"b" * 100, b"c" * 100, b"d" * 40]
    fr = [b"\x01" * 9, b"\x02" * 8, b"\x03" * 7, b"\x04" * 6]
    assert _open(lib, sc.stream_of(fr, contents, False)) == (0, [0, 1, 0, 4, 340])
    # a foreign skippable frame of 24 bytes as the last entry: a plain stream
    foreign = struct.pack("<II", 0x184D2A50, 16) + b"q" * 16
    assert _open(lib, sc.stream_of(fr, contents, True, extra_entries=[(4, foreign)])) == (0, [0, 1, 0, 5, 340])
    # the marker's magic with other payload: plain too
    assert _open(lib, sc.stream_of(fr, contents, False, extra_entries=[(4, struct.pack("<II", pm.PLANES_MAGIC, 16) + b"q" * 16)]))[1][1] == 1
    # the tag over two groups of two planes: typed -- (100, 100), (40, 40) under frame_size 100
    good = [b"a" * 100, b"b" * 100, b"c" * 40, b"d" * 40]
    assert _open(lib, pm.stream_of(fr, good, 2, 100, False)) == (0, [0, 2, 100, 5, 280])
    # unequal planes: corrupt at that frame
    assert _open(lib, pm.stream_of(fr, [b"a" * 100, b"b" * 100, b"c" * 40, b"d" * 39], 2, 100, False)) == (20, [3, 0, 0, 0, 0])
    # a group that is not frame_size and not the last; a first group above frame_size; frames that are no whole groups; an empty last group
    assert _open(lib, pm.stream_of(fr, [b"a" * 40, b"b" * 40, b"c" * 100, b"d" * 100], 2, 100, False)) == (20, [0, 0, 0, 0, 0])
    assert _open(lib, pm.stream_of(fr, good, 2, 99, False)) == (20, [0, 0, 0, 0, 0])
    assert _open(lib, pm.stream_of(fr[:3], good[:3], 2, 100, False)) == (20, [3, 0, 0, 0, 0])
    assert _open(lib, pm.stream_of(fr, [b"a" * 100, b"b" * 100, b"", b""], 2, 100, False)) == (20, [2, 0, 0, 0, 0])
    # element sizes and versions this reader does not know: corrupt at the marker
    assert _open(lib, pm.stream_of(fr[:3], [b"a" * 10] * 3, 3, 100, False)) == (20, [3, 0, 0, 0, 0])
    v2 = bytearray(pm.stream_of(fr, good, 2, 100, False)); struct.pack_into("<I", v2, sum(len(f) for f in fr) + 12, 2)
    assert _open(lib, v2) == (20, [4, 0, 0, 0, 0])


def _plan(lib, stream, rg, limit=0):
    buf = np.frombuffer(bytes(stream), dtype=np.uint8).copy()
    table = np.array([(o, n, 0) for o, n in rg], dtype=np.uint64).reshape(-1, 3)
    cap = 64
    planar = np.zeros((cap, 3), dtype=np.uint64); jobs = np.zeros((cap, 6), dtype=np.uint64); passes = np.zeros((cap, 2), dtype=np.uint64)
    owner = np.zeros((len(rg), 2), dtype=np.uint64); counts = np.zeros(3, dtype=np.uint64)
    assert lib.emu_typed_plan(buf.ctypes.data, buf.size, table.ctypes.data, len(rg), limit, cap, planar.ctypes.data, jobs.ctypes.data, passes.ctypes.data, owner.ctypes.data, counts.ctypes.data) == 0
    q, j, p = (int(x) for x in counts)
    return planar[:q].tolist(), jobs[:j].tolist(), passes[:p].tolist(), owner.tolist()


RANGES_K4 = [(1, 2), (3, 6), (100, 999), (FRAME * 4 - 5, 11), (FRAME * 4 - 3, 2 * FRAME * 4 + 9), (50, 0), (100, 999), (500, 2000), (0, ELEMENTS * 4), (ELEMENTS * 4 - 3, 3),
             (FRAME * 4, FRAME * 4), (0, 1), (ELEMENTS * 4, 0), (2 * FRAME * 4 + 2, FRAME * 4 + 37 * 4 - 2)]


def test_plan_against_the_model(lib):
    """one range at a time: the planar ranges and the jobs are the model's; at most 2k + 1 planar ranges"""
    _, stream, _, _, _ = _typed_stream(lib, 4, 0)
    for off, n in RANGES_K4:
        planar, jobs, passes, owner = _plan(lib, stream, [(off, n)])
        want_ranges, want_jobs = pm.plan(ELEMENTS, 4, FRAME, off, n)
        assert [(a, b) for a, b, _ in planar] == want_ranges, (off, n)
        assert [(m, h, t) for _, _, m, _, h, t in jobs] == want_jobs, (off, n)
        assert len(planar) <= 2 * 4 + 1 and owner == [[0, len(planar)]]
        assert len(passes) == (1 if n else 0)
        at = 0
        for a, b, p in planar:                  # back to back in the planar buffer
            assert p == at
            at += b


def _read(lib, stream, planar_content, rg, limit=0, code_frame=-1, code=0):
    """-> (rc, destination bytes per range, status, stats); the destinations back to back at byte offset 1 of a guarded buffer"""
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


@pytest.mark.parametrize("k", [2, 4])
def test_typed_ranges(lib, k):
    src, stream, _, _, _ = _typed_stream(lib, k, 1)
    content = pm.split(src, k, FRAME)
    scale = lambda o, n: (o * k // 4, n * k // 4) if k != 4 else (o, n)
    rg_all = [scale(o, n) for o, n in RANGES_K4]
    rg_all = [(o, min(n, src.size - o)) for o, n in rg_all]
    for one in rg_all:                          # R = 1
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
    """the whole content under a limit of 20 000 bytes: groups of 16 384 planar bytes -> the range is cut at group boundaries into three passes, and the planar
    buffer stays below the limit; under a limit below one group the buffer is one group"""
    src, stream, _, _, _ = _typed_stream(lib, 4, 0)
    content = pm.split(src, 4, FRAME)
    rg = [(5, src.size - 7), (3 * FRAME * 4 - 2, 100), (7, 9)]
    rc, got, status, stats = _read(lib, stream, content, rg, limit=20000)
    assert rc == 0 and status == [0] * 8
    assert [g == src[o:o + n].tobytes() for (o, n), g in zip(rg, got)] == [True] * 3
    # range 0 is group 0 from element 1 (4 095 elements), then groups 1, 2, 3 whole; range 1 one element of group 2 and 25 of group 3; range 2 three elements
    last = FRAME * 4 + 37 * 4 + 4 + 100 + 12
    assert stats[4] == 3 and stats[5] == last <= 20000
    planar, jobs, passes, owner = _plan(lib, stream, rg, 20000)
    assert [int(b) for b, _ in passes] == [4095 * 4, FRAME * 4, last] and owner[0] == [0, 4 + 1 + 1]
    rc, got, status, stats = _read(lib, stream, content, rg, limit=1000)
    assert rc == 0 and status == [0] * 8 and stats[5] == FRAME * 4
    assert [g == src[o:o + n].tobytes() for (o, n), g in zip(rg, got)] == [True] * 3


def test_one_damaged_plane_frame(lib):
    """plane frame 6 (group 1, plane 2) fails with 20: exactly the ranges that touch group 1 report {20, 6}; the others are right, bytes included"""
    src, stream, _, _, _ = _typed_stream(lib, 4, 1)
    content = pm.split(src, 4, FRAME)
    g = FRAME * 4
    rg = [(10, 100), (g - 2, 4), (g, g), (2 * g + 1, 50), (0, src.size), (g + 77, 0), (2 * g - 1, 1), (2 * g, 1), (3 * g, 148)]
    touches = [o < 2 * g and o + n > g and n > 0 for o, n in rg]
    assert touches == [False, True, True, False, True, False, True, False, False]
    for limit in (0, 20000):
        rc, got, status, stats = _read(lib, stream, content, rg, limit=limit, code_frame=6, code=20)
        assert rc == 0
        assert status[:2] == [20, 1]
        for r, ((o, n), t) in enumerate(zip(rg, touches)):
            assert status[2 + 2 * r:4 + 2 * r] == ([20, 6] if t else [0, 0]), r
            if not t:
                assert got[r] == src[o:o + n].tobytes(), r


def test_refusals(lib):
    t = _text()
    check = lambda which, size, frame, k, flags=0: lib.emu_typed_check(which, size, frame, k, flags, t)
    assert check(0, 4096, 1024, 2) == 0 and check(0, 4096, 1024, 8, 1) == 0
    for k in (0, 3, 5, 16):
        assert check(0, 4096, 1024, k) == UNSUPPORTED and b"element size" in t.value
        assert check(1, 4096, 1024, k) == UNSUPPORTED
    assert check(0, 4097, 1024, 2) == UNSUPPORTED and b"multiple" in t.value
    assert check(0, 4100, 1024, 8) == UNSUPPORTED
    assert check(0, 4096, 0, 2) == UNSUPPORTED and b"frameSize" in t.value
    assert check(0, 4096, (1 << 30) + 1, 2) == UNSUPPORTED
    assert check(0, 4096, 1 << 30, 2) == 0
    assert check(0, 4096, 1024, 2, 2) == UNSUPPORTED
    most = ((1 << 27) - 1) // 2                  # groups of one element: two frames each
    assert check(0, most * 2, 1, 2) == 0
    assert check(0, (most + 1) * 2, 1, 2) == UNSUPPORTED and b"2^27 - 1" in t.value
    assert lib.emu_typed_bound((most + 1) * 2, 1, 2, 0) == 0 and lib.emu_typed_bound(4097, 1024, 2, 0) == 0 and lib.emu_typed_bound(4096, 1024, 3, 0) == 0
    for size, frame, k, ck in ((0, 4096, 2, 0), (ELEMENTS * 4, FRAME, 4, 1), (1 << 20, 131072, 8, 0)):
        n = -(-(size // k) // frame) * k
        assert lib.emu_typed_bound(size, frame, k, ck) == size + (size >> 8) + 64 * n + 8 + n * (12 if ck else 8) + 9 + 24 + (12 if ck else 8)
    # the typed read on a plain handle; a range beyond the content of a typed one
    contents = [b"a" * 100, b"b" * 40]
    plain = sc.stream_of([b"\x01" * 9, b"\x02" * 8], contents, False)
    rc, _, status, _ = _read(lib, plain, np.frombuffer(b"".join(contents), dtype=np.uint8).copy(), [(0, 10)])
    assert rc == UNSUPPORTED and status == [-1] * 4
    src, stream, _, _, _ = _typed_stream(lib, 4, 0)
    rc, _, status, stats = _read(lib, stream, pm.split(src, 4, FRAME), [(0, 4), (src.size - 1, 2)])
    assert rc == sc.SIZE_MISMATCH and status == [-1] * 6 and stats[6] == 1


def test_sanitizer_program(tmp_path):
    """tests/emu/typed_planes_main.cpp under AddressSanitizer and UBSan: the split, join and seal bodies over the shapes above, heap buffers sized exactly"""
    exe = os.path.join(str(tmp_path), "typed_planes_asan")
    subprocess.check_call(["sh", os.path.join(EMU, "build_asan_planes.sh"), "typed_planes_main.cpp", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert b"cases" in r.stdout
