"""The xor-with-base filter of typed seekable streams (python-zstandard_amd/csrc/zhip_seekable_typed.hpp and zhip_seekable_typed_calls.hpp) on the
host wave emulator, against the numpy model of tests/xor_model.py: the split-with-xor and join-with-xor bodies over the shapes at which they take another path
and over the three kinds of base, the compress call's stream, the marker's verdicts, typed ranges with a base over the range sets of
tests/seekable_range_cases.py, the read plan (unchanged without the filter), every refusal, the stand-alone sanitizer program, and the size the filter is
there for (libzstd alone). No GPU."""
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
from tests import seekable_range_cases as rc_cases
from tests import xor_model as xm
from tests.test_emu_seekable_typed import ELEMENTS, FRAME, RANGES_K4, UNSUPPORTED, _guarded, _intact

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
T_TYPED = 100                       # the trace's name of typed kernel k: 100 + k
K_SPLIT, K_JOIN, K_STATUS, K_SPLIT_DELTA, K_SPLIT_XOR, K_JOIN_XOR = 0, 1, 4, 5, 9, 10
T_KERNELS = set(range(T_TYPED, T_TYPED + 11))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("emu_seekable_xor_base")), "libzhip_emu_seekable_xor_base.so")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + EMU, "-w", "-o", out, os.path.join(EMU, "zhemu.cpp"), os.path.join(EMU, "emu_seekable_xor_base.cpp")])
    lib = C.CDLL(out)
    vp, u64, u32, i32, i64, ci = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_int64, C.c_int
    lib.emu_xor_split.restype = None; lib.emu_xor_split.argtypes = [vp, vp, u64, u32, u32, vp, u32, vp]
    lib.emu_xor_join.restype = None; lib.emu_xor_join.argtypes = [vp, vp, vp, vp, u32, u64, u32, u32, u32]
    lib.emu_xor_planes_call.restype = ci; lib.emu_xor_planes_call.argtypes = [ci, vp, u64, u32, u32, vp, vp, vp, u64, vp, vp, vp]
    lib.emu_xor_compress.restype = ci; lib.emu_xor_compress.argtypes = [vp, vp, u64, u32, u32, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp]
    lib.emu_xor_plan.restype = ci; lib.emu_xor_plan.argtypes = [vp, u64, vp, u64, u64, i64, u64, vp, vp, vp, vp, vp, vp, vp]
    lib.emu_xor_ranges.restype = ci; lib.emu_xor_ranges.argtypes = [vp, u64, vp, vp, u64, vp, u64, vp, u64, u64, i64, i32, vp, vp, vp, u64, vp, vp]
    lib.emu_xor_check.restype = ci; lib.emu_xor_check.argtypes = [ci, u64, u32, u32, ci, vp, vp]
    # the entries of before, in this library too
    lib.emu_delta_compress.restype = ci; lib.emu_delta_compress.argtypes = [ci, u32, vp, u64, u32, u32, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp]
    lib.emu_delta_open.restype = ci; lib.emu_delta_open.argtypes = [vp, u64, vp]
    lib.emu_delta_plan.restype = ci; lib.emu_delta_plan.argtypes = [vp, u64, vp, u64, u64, ci, u64, vp, vp, vp, vp, vp]
    lib.emu_delta_check.restype = ci; lib.emu_delta_check.argtypes = [ci, u64, u32, u32, u32, vp, vp]
    lib.emu_typed_grid.restype = u32; lib.emu_typed_grid.argtypes = [ci, u64, u32, u32]
    lib.emu_typed_bound.restype = u64; lib.emu_typed_bound.argtypes = [u64, u32, u32, ci]
    lib.emu_typed_plan.restype = ci; lib.emu_typed_plan.argtypes = [vp, u64, vp, u64, u64, u64, vp, vp, vp, vp, vp]
    lib.emu_typed_ranges.restype = ci; lib.emu_typed_ranges.argtypes = [vp, u64, vp, vp, u64, vp, u64, u64, i64, i32, vp, vp, vp]
    return lib


# ------------------------------------------------------------------------------------------------ the bodies
@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("m", xm.GROUP_SIZES)
def test_split_and_join_bodies(lib, k, m):
    """every kind of base on every shape: split-xor is the model's planar bytes (all zero where the base is the source), the record table the planes', join-xor
    of them the source; guard bytes around every buffer; byte offsets 0, 1 and 3"""
    for elements in xm.shapes(m):
        src = xm.source(k, elements, seed=100 * k + m)
        for n_kind, kind in enumerate(xm.BASES):
            base = xm.base_of(kind, src, k, seed=m)
            want = xm.split(src, base, k, m)
            assert xm.join(want, base, k, m).tobytes() == src.tobytes() and (kind != "same" or not want.any())
            off = (0, 1, 3)[(n_kind + elements) % 3]
            raw_s, s, at_s = _guarded(src.size, off); s[:] = src
            raw_b, b, at_b = _guarded(src.size, (off + 2) % 4); b[:] = base
            raw, d, at = _guarded(src.size, (off + 1) % 4 if off else 0)
            planes = xm.planes(src, base, k, m)
            records = np.zeros((len(planes), 2), dtype=np.uint64)
            grid = lib.emu_typed_grid(1, src.size, k, m)
            lib.emu_xor_split(s.ctypes.data, b.ctypes.data, src.size, k, m, d.ctypes.data, grid, records.ctypes.data)
            assert (d == want).all(), (k, m, elements, kind)
            assert _intact(raw, at, src.size) and (s == src).all() and (b == base).all() and _intact(raw_s, at_s, src.size) and _intact(raw_b, at_b, src.size)
            assert all(d[int(o):int(o + ln)].tobytes() == p for (o, ln), p in zip(records, planes))
            raw2, back, at2 = _guarded(src.size, off)
            lib.emu_xor_join(d.ctypes.data, b.ctypes.data, back.ctypes.data, None, 0, src.size, k, m, grid)
            assert (back == src).all(), (k, m, elements, kind)
            assert _intact(raw2, at2, src.size) and (b == base).all() and _intact(raw_b, at_b, src.size) and _intact(raw, at, src.size)


@pytest.mark.parametrize("k", [2, 4, 8])
def test_fewer_waves_than_tiles(lib, k):
    """the grid-stride loops' later trips: 3 groups of 2 500 elements are 9 tiles, on 1 and on 4 workgroups"""
    m, elements = 2500, 3 * 2500
    src = xm.source(k, elements, seed=7 + k); base = xm.base_of("low_bits", src, k)
    want = xm.split(src, base, k, m)
    for grid in (1, 4):
        raw, d, at = _guarded(src.size, 1)
        lib.emu_xor_split(src.ctypes.data, base.ctypes.data, src.size, k, m, d.ctypes.data, grid, None)
        assert (d == want).all() and _intact(raw, at, src.size)
        raw2, back, at2 = _guarded(src.size, 3)
        lib.emu_xor_join(d.ctypes.data, base.ctypes.data, back.ctypes.data, None, 0, src.size, k, m, grid)
        assert (back == src).all() and _intact(raw2, at2, src.size)


@pytest.mark.parametrize("k", [2, 4, 8])
def test_join_jobs_with_trims_and_content_offsets(lib, k):
    """jobs of 1 ... 2 100 elements that trim their first and last element, their base bytes anywhere in the base and their destinations in another order, all
    in ONE launch: every job's output is its slice of the joined planes XOR the base bytes at ITS content offset -- which neither dst nor planar gives"""
    rng = np.random.default_rng(43 + k)
    total = 9000 * k
    base = rng.integers(0, 256, total, dtype=np.uint8)
    jobs, pieces, planar, at_p = [], [], [], 0
    for m in (1, 15, 16, 17, 37, 1024, 1030, 2100):
        for h, t in ((0, 0), (1, 0), (0, 1), (k - 1, k - 1)):
            if h + t >= m * k:
                continue
            content = int(rng.integers(0, total // k - m + 1)) * k
            x = rng.integers(0, 256, m * k, dtype=np.uint8)              # the filtered elements
            planar.append(x.reshape(m, k).T.reshape(-1))
            pieces.append((x ^ base[content:content + m * k])[h:m * k - t])
            jobs.append([at_p, m, 0, h, t, content])
            at_p += m * k
    at_d = 0
    for j in rng.permutation(len(jobs)):                                 # the destinations: another order than the planar buffer's
        jobs[j][2] = at_d; at_d += pieces[j].size
    want = np.zeros(at_d, dtype=np.uint8)
    for job, piece in zip(jobs, pieces):
        want[job[2]:job[2] + piece.size] = piece
    planar = np.concatenate(planar)
    table = np.array(jobs, dtype=np.uint64)
    for off, grid in ((0, 8), (1, 3), (3, 1)):
        _, p, _ = _guarded(planar.size, off); p[:] = planar
        raw_b, b, at_b = _guarded(total, (off + 1) % 4); b[:] = base
        raw, d, at = _guarded(want.size, off)
        lib.emu_xor_join(p.ctypes.data, b.ctypes.data, d.ctypes.data, table.ctypes.data, len(jobs), 0, k, 1, grid)
        assert (d == want).all(), (k, off)
        assert _intact(raw, at, want.size) and (b == base).all() and _intact(raw_b, at_b, total)


# ------------------------------------------------------------------------------------------------ the stand-alone calls
def test_planes_calls(lib):
    """the calls with a base: one kernel each way on the plain kernels' grid, no tile-sums area"""
    k, m = 4, 1025
    src = xm.source(k, 3 * m + 17, seed=9); base = xm.base_of("low_bits", src, k)
    grid = lib.emu_typed_grid(1, src.size, k, m)

    def call(which, data):
        dst = np.full(src.size, 0x5A, dtype=np.uint8)
        trace = np.zeros(16, dtype=np.uint32); words = np.zeros(1, dtype=np.uint64); info = np.zeros(1, dtype=np.uint64)
        rc = lib.emu_xor_planes_call(which, data.ctypes.data, src.size, k, m, base.ctypes.data, dst.ctypes.data, trace.ctypes.data, 16, words.ctypes.data, info.ctypes.data, None)
        return rc, dst, trace[:int(words[0])].tolist(), int(info[0])

    rc, planar, trace, area = call(0, src)
    assert rc == 0 and (planar == xm.split(src, base, k, m)).all() and trace == [T_TYPED + K_SPLIT_XOR, grid] and area == 0
    rc, back, trace, area = call(1, planar)
    assert rc == 0 and (back == src).all() and trace == [T_TYPED + K_JOIN_XOR, grid] and area == 0


# ------------------------------------------------------------------------------------------------ the whole calls
_built = {}


def _pair(k, seed=5):
    """(source bytes, base bytes): random elements, and the same with only low bits of byte 0 flipped -- the high planes of the XOR are zeros, the low noise"""
    src = xm.source(k, ELEMENTS, seed=seed)
    return src, xm.base_of("low_bits", src, k, seed=seed)


def _stream(lib, k, checksum, seed=5):
    """(source, base, the stream the emulated call wrote, the filtered planes' libzstd frames, the kernel trace)"""
    key = (k, checksum, seed)
    if key in _built:
        return _built[key]
    src, base = _pair(k, seed)
    ref = reflib.checker()
    planes = xm.planes(src, base, k, FRAME)
    frames = [ref.compress(p, level=3) for p in planes]
    blob = np.frombuffer(b"".join(frames), dtype=np.uint8)
    offs = np.cumsum([0] + [len(f) for f in frames]).astype(np.uint64)
    bound = lib.emu_typed_bound(src.size, FRAME, k, checksum)
    raw, d, at = _guarded(bound, 0)
    status = np.full(2, -1, dtype=np.int32); info = np.zeros(4, dtype=np.uint64); staging = np.zeros(src.size, dtype=np.uint8)
    trace = np.zeros(64, dtype=np.uint32); words = np.zeros(1, dtype=np.uint64)
    rc = lib.emu_xor_compress(src.ctypes.data, base.ctypes.data, src.size, FRAME, k, checksum, blob.ctypes.data, offs.ctypes.data, d.ctypes.data, bound, status.ctypes.data,
                              staging.ctypes.data, info.ctypes.data, trace.ctypes.data, 64, words.ctypes.data, None)
    assert rc == 0 and status.tolist() == [0, 0] and int(info[1]) == 0 and _intact(raw, at, bound)
    assert (staging == xm.split(src, base, k, FRAME)).all()
    _built[key] = (src, base, d[:int(info[0])].tobytes(), frames, trace[:int(words[0])].tolist())
    return _built[key]


def _delta_stream(lib, k, filt):
    """a stream of the same source under filter 0 or 1, through the entry of before"""
    src, _ = _pair(k)
    ref = reflib.checker()
    planes = dm.planes(src, k, FRAME) if filt else pm.planes(src, k, FRAME)
    frames = [ref.compress(p, level=3) for p in planes]
    blob = np.frombuffer(b"".join(frames), dtype=np.uint8); offs = np.cumsum([0] + [len(f) for f in frames]).astype(np.uint64)
    bound = lib.emu_typed_bound(src.size, FRAME, k, 0)
    d = np.zeros(bound, dtype=np.uint8); status = np.full(2, -1, dtype=np.int32); info = np.zeros(4, dtype=np.uint64)
    trace = np.zeros(64, dtype=np.uint32); words = np.zeros(1, dtype=np.uint64)
    assert lib.emu_delta_compress(1, filt, src.ctypes.data, src.size, FRAME, k, 0, blob.ctypes.data, offs.ctypes.data, d.ctypes.data, bound, status.ctypes.data, None, info.ctypes.data,
                                  trace.ctypes.data, 64, words.ctypes.data, None) == 0
    return src, d[:int(info[0])].tobytes()


def _open(lib, stream):
    buf = np.frombuffer(bytes(stream), dtype=np.uint8).copy()
    out = np.zeros(6, dtype=np.uint64)
    return lib.emu_delta_open(buf.ctypes.data, buf.size, out.ctypes.data), out.tolist()


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("checksum", [0, 1])
def test_compress_and_marker(lib, k, checksum):
    """the stream is the model's: libzstd's frames of the XORed planes, the marker's word k | 0x400 under version 1, the table's checksums those of the filtered
    planar content; the split is the xor kernel and the only typed kernel in front of the seal; open reports filter 4"""
    src, base, stream, frames, trace = _stream(lib, k, checksum)
    planes = xm.planes(src, base, k, FRAME)
    assert stream == xm.stream_of(frames, planes, k, FRAME, bool(checksum))
    at = sum(len(f) for f in frames)
    assert struct.unpack_from("<I", stream, at + 16)[0] == k | 0x400 and struct.unpack_from("<I", stream, at + 12)[0] == 1
    entries, ck, _ = sc.parse(stream)
    assert ck == bool(checksum) and all(x is None or x == sc.xxh64(p) & 0xFFFFFFFF for (_, _, x), p in zip(entries, planes))
    assert trace[0] == T_TYPED + K_SPLIT_XOR and (T_TYPED + K_SPLIT) not in trace[::2] and (T_TYPED + K_SPLIT_DELTA) not in trace[::2]
    assert _open(lib, stream) == (0, [0, k, FRAME, 4 * k + 1, ELEMENTS * k, xm.XOR_BASE])
    assert any(not any(p) for p in planes) and any(len(f) > len(p) // 4 for f, p in zip(frames, planes))      # (zero planes and noisy planes in one stream)


def test_marker_verdicts(lib):
    """k | 0x400 opens with filter 4; filter 5, bits above the filter's byte, an element size of 3, and the values that never were filters: corrupt at the marker"""
    src, base, stream, frames, _ = _stream(lib, 4, 0)
    at = sum(len(f) for f in frames) + 16
    n = 4 * 4                                                     # the marker's frame index
    for word, verdict in ((4 | 0x400, 0), (4 | 0x100, 0), (4, 0), (4 | 0x500, 20), (4 | 0x400 | 1 << 16, 20), (3 | 0x400, 20), (4 | 0x200, 20), (4 | 0x300, 20), (1 | 0x400, 20)):
        s = bytearray(stream); struct.pack_into("<I", s, at, word)
        code, out = _open(lib, s)
        assert code == verdict, hex(word)
        assert out == ([0, 4, FRAME, n + 1, ELEMENTS * 4, word >> 8] if not verdict else [n, 0, 0, 0, 0, 0]), hex(word)


def _plan(lib, stream, rg, limit=0, filt=-1):
    buf = np.frombuffer(bytes(stream), dtype=np.uint8).copy()
    table = np.array([(o, n, 0) for o, n in rg], dtype=np.uint64).reshape(-1, 3)
    cap = 256
    planar = np.zeros((cap, 3), dtype=np.uint64); jobs = np.zeros((cap, 7), dtype=np.uint64); passes = np.zeros((cap, 2), dtype=np.uint64); content = np.zeros(cap, dtype=np.uint64)
    owner = np.zeros((len(rg), 2), dtype=np.uint64); counts = np.zeros(4, dtype=np.uint64); layout = np.zeros(5, dtype=np.uint64)
    assert lib.emu_xor_plan(buf.ctypes.data, buf.size, table.ctypes.data, len(rg), limit, filt, cap, planar.ctypes.data, jobs.ctypes.data, passes.ctypes.data, owner.ctypes.data,
                            content.ctypes.data, counts.ctypes.data, layout.ctypes.data) == 0
    q, j, p, c = (int(x) for x in counts)
    return planar[:q].tolist(), jobs[:j].tolist(), passes[:p].tolist(), owner.tolist(), content[:c].tolist(), layout.tolist()


def _old_plan(lib, stream, rg, limit, delta_entry):
    """the plan through an entry of before: emu_typed_plan (six words a job, no filter) or emu_delta_plan (seven, the stream's filter)"""
    buf = np.frombuffer(bytes(stream), dtype=np.uint8).copy()
    table = np.array([(o, n, 0) for o, n in rg], dtype=np.uint64).reshape(-1, 3)
    cap, w = 256, 7 if delta_entry else 6
    planar = np.zeros((cap, 3), dtype=np.uint64); jobs = np.zeros((cap, w), dtype=np.uint64); passes = np.zeros((cap, 2), dtype=np.uint64)
    owner = np.zeros((len(rg), 2), dtype=np.uint64); counts = np.zeros(3, dtype=np.uint64)
    if delta_entry:
        assert lib.emu_delta_plan(buf.ctypes.data, buf.size, table.ctypes.data, len(rg), limit, 0, cap, planar.ctypes.data, jobs.ctypes.data, passes.ctypes.data, owner.ctypes.data, counts.ctypes.data) == 0
    else:
        assert lib.emu_typed_plan(buf.ctypes.data, buf.size, table.ctypes.data, len(rg), limit, cap, planar.ctypes.data, jobs.ctypes.data, passes.ctypes.data, owner.ctypes.data, counts.ctypes.data) == 0
    q, j, p = (int(x) for x in counts)
    return planar[:q].tolist(), jobs[:j].tolist(), passes[:p].tolist(), owner.tolist()


def _up16(n):
    return (n + 15) // 16 * 16


def test_plan_and_its_content_offsets(lib):
    """the plan of a filter-4 stream is the unfiltered plan -- the model's planar ranges and jobs, skip 0 everywhere, the planar ranges of a partly covered
    group starting where the range starts -- plus one content offset per job: the model's, (g0 + lo) * k"""
    _, _, stream, _, _ = _stream(lib, 4, 0)
    for off, n in RANGES_K4:
        planar, jobs, passes, owner, content, layout = _plan(lib, stream, [(off, n)])
        want_ranges, want_jobs, want_content = xm.plan(ELEMENTS, 4, FRAME, off, n)
        assert [(a, b) for a, b, _ in planar] == want_ranges and [(m, h, t, skip) for _, _, m, _, h, t, skip in jobs] == [j + (0,) for j in want_jobs], (off, n)
        assert content == want_content and len(content) == len(jobs), (off, n)
        planar0, jobs0, passes0, owner0, content0, _ = _plan(lib, stream, [(off, n)], filt=xm.NONE)
        assert (planar0, jobs0, passes0, owner0, content0) == (planar, jobs, passes, owner, [])
    # under a small limit: passes, and the content offsets still one per job, in job order
    rg = [(o, n) for o, n in RANGES_K4]
    planar, jobs, passes, owner, content, layout = _plan(lib, stream, rg, limit=20000)
    assert len(passes) > 1 and len(content) == len(jobs)
    flat = [c for o, n in rg for c in xm.plan(ELEMENTS, 4, FRAME, o, n)[2]]
    assert content == flat
    assert layout == [0, _up16(len(jobs) * 48), _up16(len(jobs) * 48) + _up16(len(rg) * 8), _up16(len(jobs) * 48) + _up16(len(rg) * 8) + _up16(len(planar) * 4),
                      _up16(len(jobs) * 48) + _up16(len(rg) * 8) + _up16(len(planar) * 4) + _up16(len(jobs) * 8)]


@pytest.mark.parametrize("filt", [xm.NONE, xm.DELTA])
def test_no_plan_change_without_the_filter(lib, filt):
    """filter 0 and filter 1 streams: the plan is field for field what the entries of before compute -- emu_typed_plan's six words a job (filter 0),
    emu_delta_plan's seven (the stream's filter) -- under the default limit and under small ones; no content offsets, and the upload is as long as it was"""
    src, stream = _delta_stream(lib, 4, filt)
    rg = [(o, n) for o, n in RANGES_K4]
    for limit in (0, 20000, 1000):
        planar, jobs, passes, owner, content, layout = _plan(lib, stream, rg, limit=limit)
        old = _old_plan(lib, stream, rg, limit, True)
        assert (planar, jobs, passes, owner) == old and content == []
        if filt == xm.NONE:
            planar6, jobs6, passes6, owner6 = _old_plan(lib, stream, rg, limit, False)
            assert planar6 == planar and jobs6 == [j[:6] for j in jobs] and all(j[6] == 0 for j in jobs) and passes6 == passes and owner6 == owner
        else:
            assert any(j[6] for j in jobs)                                  # (the delta plan does skip)
        end = _up16(len(jobs) * 48) + _up16(len(rg) * 8) + _up16(len(planar) * 4)
        assert layout == [0, _up16(len(jobs) * 48), _up16(len(jobs) * 48) + _up16(len(rg) * 8), end, end]
    for off, n in RANGES_K4:                                                # and one range at a time against the models
        planar, jobs, _, _, content, _ = _plan(lib, stream, [(off, n)])
        want_ranges, want_jobs = dm.plan(ELEMENTS, 4, FRAME, off, n) if filt else pm.plan(ELEMENTS, 4, FRAME, off, n)
        assert [(a, b) for a, b, _ in planar] == want_ranges and [(m, h, t, skip) for _, _, m, _, h, t, skip in jobs] == [j if filt else j + (0,) for j in want_jobs]
        assert content == []


def _read(lib, stream, planar_content, base, table, capacity, limit=0, code_frame=-1, code=0, base_size=None, base_ptr=None):
    """the emulated typed read with a base into a guarded destination of `capacity` bytes; table: [(offset, length, dstOffset)] -> (rc, the destination, status, stats, trace, text)"""
    buf = np.frombuffer(bytes(stream), dtype=np.uint8).copy()
    rg = rc_cases.ranges_array(table)
    raw, d, dat = _guarded(capacity, 1)
    raw_b, b, at_b = _guarded(base.size, 3); b[:] = base
    status = np.full(2 + 2 * len(table), -1, dtype=np.int32); stats = np.zeros(7, dtype=np.uint64)
    trace = np.zeros(1 << 16, dtype=np.uint32); words = np.zeros(1, dtype=np.uint64); text = C.create_string_buffer(256)
    ptr = {None: b.ctypes.data, "null": None, "dst": d.ctypes.data + max(capacity - 1, 0)}[base_ptr]
    rc = lib.emu_xor_ranges(buf.ctypes.data, buf.size, planar_content.ctypes.data, ptr, base.size if base_size is None else base_size, rg.ctypes.data, len(table), d.ctypes.data, capacity,
                            limit, code_frame, code, status.ctypes.data, stats.ctypes.data, trace.ctypes.data, trace.size, words.ctypes.data, text)
    assert _intact(raw, dat, capacity) and (b == base).all() and _intact(raw_b, at_b, base.size)
    return rc, d.copy(), status.tolist(), [int(x) for x in stats], trace[:min(int(words[0]), trace.size)].tolist(), text.value


def _range_sets(k):
    """the range lists of tests/seekable_range_cases.py over the stream's groups in ELEMENT order: zero-length, the whole content, duplicates, nested, group
    boundary to group boundary, ending on one, inside one group, anywhere (so starts and ends inside elements and inside groups), each with a destination of its own"""
    d_off = np.array([min(g * FRAME * k, ELEMENTS * k) for g in range(5)], dtype=np.int64)
    out = []
    for seed, count in ((1, 0), (2, 3), (3, 9), (4, 40), (5, 64), (6, 130)):
        rng = np.random.default_rng(7100 + seed + k)
        out.append(rc_cases.place_destinations(rng, rc_cases.random_ranges(rng, d_off, count)))
    return out


@pytest.mark.parametrize("k", [2, 4, 8])
def test_typed_ranges_with_a_base(lib, k):
    """the elements read back through zsk_typed_ranges_base equal the source's slices, under the default scratch limit and under small ones (several
    passes); nothing outside the ranges' destinations is written; one xor join per pass and no other join"""
    src, base, stream, _, _ = _stream(lib, k, 1)
    content = xm.split(src, base, k, FRAME)
    for table, capacity in _range_sets(k):
        for limit in rc_cases.LIMITS:
            rc, d, status, stats, trace, _ = _read(lib, stream, content, base, table, capacity, limit=limit)
            assert rc == 0 and status == [0] * (2 + 2 * len(table)), (k, len(table), limit)
            for o, n, to in table:
                assert d[to:to + n].tobytes() == src[o:o + n].tobytes(), (o, n, limit)
            assert (d[rc_cases.untouched_mask(table, capacity)] == 0x5A).all()
            kernels = [t for t in trace[::2] if t in T_KERNELS]
            if any(n for _, n, _ in table):
                assert kernels == [T_TYPED + K_JOIN_XOR] * stats[4] + [T_TYPED + K_STATUS] and stats[4] >= 1
                if limit == 4096 and sum(n for _, n, _ in table) > 3 * 4096:
                    assert stats[4] > 1
    for off, n in [(o * k // 4, min(n * k // 4, ELEMENTS * k - o * k // 4)) for o, n in RANGES_K4]:      # and the fixed ranges of the typed tests, singly
        rc, d, status, _, _, _ = _read(lib, stream, content, base, [(off, n, 0)], n)
        assert rc == 0 and status == [0, 0, 0, 0] and d.tobytes() == src[off:off + n].tobytes(), (off, n)


def test_another_base_gives_wrong_elements_and_status_0(lib):
    """the stream does not name its base: a base of the right size that is not the one it was written against reads back as source ^ base ^ other, status 0"""
    src, base, stream, _, _ = _stream(lib, 4, 0)
    content = xm.split(src, base, 4, FRAME)
    other = xm.base_of("random", src, 4, seed=77)
    rc, d, status, _, _, _ = _read(lib, stream, content, other, [(5, 3000, 0)], 3000)
    assert rc == 0 and status == [0, 0, 0, 0] and d.tobytes() == (src ^ base ^ other)[5:3005].tobytes() != src[5:3005].tobytes()


def test_one_damaged_plane_frame(lib):
    """plane frame 6 (group 1, plane 2) fails with 20: exactly the ranges that need group 1 report {20, 6}; the others are right, bytes included"""
    src, base, stream, _, _ = _stream(lib, 4, 1)
    content = xm.split(src, base, 4, FRAME)
    g = FRAME * 4
    rg = [(10, 100), (g - 2, 4), (g, g), (2 * g + 1, 50), (0, src.size), (g + 77, 0), (2 * g - 1, 1), (2 * g, 1), (3 * g, 148)]
    touches = [o < 2 * g and o + n > g and n > 0 for o, n in rg]
    table, at = [], 0
    for o, n in rg:
        table.append((o, n, at)); at += n
    for limit in (0, 20000):
        rc, d, status, stats, _, _ = _read(lib, stream, content, base, table, at, limit=limit, code_frame=6, code=20)
        assert rc == 0 and status[:2] == [20, 1]
        for r, ((o, n, to), t) in enumerate(zip(table, touches)):
            assert status[2 + 2 * r:4 + 2 * r] == ([20, 6] if t else [0, 0]), r
            if not t:
                assert d[to:to + n].tobytes() == src[o:o + n].tobytes(), r


def test_refusals(lib):
    """every refusal of the calls with a base, and of the calls of before on filter 4: UNSUPPORTED, nothing launched, nothing written"""
    t = C.create_string_buffer(256); words = np.zeros(1, dtype=np.uint64)
    check = lambda which, size, frame, k, mode: (lib.emu_xor_check(which, size, frame, k, mode, words.ctypes.data, t), int(words[0]))
    for which in (0, 1, 2):
        assert check(which, 4096, 1024, 4, 0) == (UNSUPPORTED, 0) and b"base" in t.value and b"NULL" in t.value          # a null base
        assert check(which, 4096, 1024, 1, 1) == (UNSUPPORTED, 0) and b"element size" in t.value                          # element size 1
        assert check(which, 4096, 1024, 4, 2) == (UNSUPPORTED, 0) and b"overlaps" in t.value                              # a base that shares a byte with the output
        assert check(which, 4096, 1024, 3, 1) == (UNSUPPORTED, 0) and check(which, 4097, 1024, 2, 1) == (UNSUPPORTED, 0) and check(which, 4096, 0, 2, 1) == (UNSUPPORTED, 0)      # the plain calls' own
    for which in (3, 4, 5):                                                 # the *_filter_ calls have no base to take: filter 4 as filter 2
        for k in (1, 2, 4, 8):
            assert check(which, 4096, 1024, k, 0) == (UNSUPPORTED, 0) and b"filter" in t.value, (which, k)
    for filt in (2, 3, 5):                                                  # and what never was a filter stays refused (the entry of before)
        for k in (1, 2, 4, 8):
            assert (lib.emu_delta_check(0, 4096, 1024, k, filt, words.ctypes.data, t), int(words[0])) == (UNSUPPORTED, 0) and b"filter" in t.value
        assert (lib.emu_delta_check(1, 4096, 1024, 4, filt, words.ctypes.data, t), int(words[0])) == (UNSUPPORTED, 0) and b"filter" in t.value

    # the read: a null base, a base of another size, a base over the output, a stream whose filter is not 4; the read without a base on a filter-4 stream
    src, base, stream, _, _ = _stream(lib, 4, 0)
    content = xm.split(src, base, 4, FRAME)
    table = [(8, 4000, 0)]
    for kw, word in ((dict(base_ptr="null"), b"NULL"), (dict(base_size=base.size - 4), b"size"), (dict(base_size=base.size + 4), b"size"), (dict(base_size=0), b"size"),
                     (dict(base_ptr="dst"), b"overlaps")):
        rc, d, status, stats, trace, text = _read(lib, stream, content, base, table, 4000, **kw)
        assert rc == UNSUPPORTED and trace == [] and (d == 0x5A).all() and status == [-1] * 4 and word in text and b"base" in text, kw
    for filt in (xm.NONE, xm.DELTA):
        _, other = _delta_stream(lib, 4, filt)
        rc, d, status, stats, trace, text = _read(lib, other, content, base, table, 4000)
        assert rc == UNSUPPORTED and trace == [] and (d == 0x5A).all() and status == [-1] * 4 and b"filter" in text
    buf = np.frombuffer(stream, dtype=np.uint8).copy()
    rg = rc_cases.ranges_array(table)
    raw, d, at = _guarded(4000, 1)
    status = np.full(4, -1, dtype=np.int32); stats = np.zeros(7, dtype=np.uint64); text = C.create_string_buffer(256)
    rc = lib.emu_typed_ranges(buf.ctypes.data, buf.size, content.ctypes.data, rg.ctypes.data, 1, d.ctypes.data, 4000, 0, -1, 0, status.ctypes.data, stats.ctypes.data, text)
    assert rc == UNSUPPORTED and b"base" in text.value and (d == 0x5A).all() and _intact(raw, at, 4000) and status.tolist() == [-1] * 4 and stats[5] == 0


# ------------------------------------------------------------------------------------------------ what the filter is for
def test_size_claim_with_libzstd_alone():
    """bf16, four groups of 131 072, default_rng(7): w0 = N(0, 1) * 0.02 in fp32, w1 = w0 + N(0, 1) * 0.02 * 1e-3, both rounded to bf16 with torch on the CPU.
    libzstd's level-3 frames of every plane of every group of w1 ^ w0 sum to at most 0.35 of those of w1's planes (libzstd alone, with seed 1, gives 0.247). The
    package's host model is what is measured; it is also checked against tests/xor_model.py"""
    import zstandard_amd.seekable as zs
    G = 131072
    w0, w1 = xm.checkpoint_pair("bf16", 4 * G, 1e-3, 7)
    ref = reflib.checker()
    plain = zs.elements_to_planes(w1, 2, G)
    filtered = zs.elements_to_planes(w1, 2, G, base=w0)
    assert filtered == zs.elements_to_planes(w1, 2, G, filter="xor_base", base=w0) == xm.split(w1, w0, 2, G).tobytes() and plain == pm.split(np.frombuffer(w1, dtype=np.uint8), 2, G).tobytes()
    assert zs.planes_to_elements(filtered, 2, G, base=w0) == w1 and zs.planes_to_elements(filtered, 2, G, base=w1) == w0
    total = {name: sum(len(ref.compress(planar[at:at + G], level=3)) for at in range(0, len(planar), G)) for name, planar in (("planes", plain), ("xor", filtered))}
    print("planes %d bytes (%.3f of raw), xor with base + planes %d bytes (%.3f of raw): ratio %.3f" % (total["planes"], total["planes"] / len(w1), total["xor"], total["xor"] / len(w1),
                                                                                                      total["xor"] / total["planes"]))
    assert total["xor"] <= 0.35 * total["planes"]
    for bad in (dict(filter="xor_base"), dict(filter="delta", base=w0), dict(filter="xor", base=w0), dict(base=w0[:-2])):
        with pytest.raises(ValueError):
            zs.elements_to_planes(w1, 2, G, **bad)
    with pytest.raises(ValueError):
        zs.elements_to_planes(w1, 2, G, filter="xor")


def test_sanitizer_program(tmp_path):
    """tests/emu/xor_planes_main.cpp under AddressSanitizer and UBSan: the split and join bodies over the shapes above, every buffer -- the base too -- a heap
    allocation sized exactly. A program of its own, run as a subprocess"""
    exe = os.path.join(str(tmp_path), "xor_planes_asan")
    subprocess.check_call(["sh", os.path.join(EMU, "build_asan_planes.sh"), "xor_planes_main.cpp", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert b"cases" in r.stdout
