"""The host side of the seekable calls (python-zstandard_amd/csrc/zhip_seekable_calls.hpp), which the library and the emulator harness both compile: every meta
layout (alignment, no two arrays overlapping, everything inside what is reserved, the reserved totals as they were before the expressions moved:
tests/golden/seekable_layouts.json), the launch sequence of one small case per call against the order DESIGN.md section 9 states, at one CU with the lanes
running and at 256 CUs recording only, and the host checks' codes and texts. No GPU."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import seekable_cases as sc
from tests import seekable_edit_cases as ec
from tests import seekable_range_cases as rc_
from tests import seekable_record_cases as rec

HERE = os.path.dirname(os.path.abspath(__file__))
UNSUPPORTED, SIZE_MISMATCH = 6, 3            # ZHIP_ERR_UNSUPPORTED, ZHIP_ERR_SIZE_MISMATCH (include/zstd_hip.h)
SCAN_TILE, SCAN_GRID, COPY_TILE = 256, 1024, 4096
COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 262143, 262144, 262145, 1 << 27]
# ZskKernel's order, then what the backend calls the compaction and the batch calls
(SCAN_REDUCE, SCAN_WRITE, CHUNK_SEGS, VERDICT, TABLE, RECORDS_VERDICT, RECORDS_SEGS, RECORDS_TABLE, RANGE_SEGS, RANGE_VERIFY, RANGE_FINISH, GATHER_SEGS, GATHER_VERIFY,
 GATHER_FINISH, EDIT_SIZES, EDIT_VERDICT, EDIT_COPY, EDIT_TABLE, COMPACT, COMPRESS, DECOMPRESS) = range(21)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = os.path.join(HERE, "emu")
    out = os.path.join(str(tmp_path_factory.mktemp("emu_seekable_calls")), "libzhip_emu_seekable_calls.so")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + d, "-w", "-o", out, os.path.join(d, "zhemu.cpp"), os.path.join(d, "emu_seekable_calls.cpp")])
    lib = C.CDLL(out)
    vp, u64, u32, i32, i64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_int64
    lib.emu_calls_mode.restype = None; lib.emu_calls_mode.argtypes = [C.c_int, C.c_int]
    lib.emu_calls_trace.restype = u64; lib.emu_calls_trace.argtypes = [vp, u64]
    lib.emu_calls_ids.restype = None; lib.emu_calls_ids.argtypes = [vp]
    lib.emu_calls_layout.restype = u64; lib.emu_calls_layout.argtypes = [u32, vp, vp]
    lib.emu_check_compress.restype = C.c_int; lib.emu_check_compress.argtypes = [C.c_int, u64, u32, C.c_int, vp]
    lib.emu_check_records.restype = C.c_int; lib.emu_check_records.argtypes = [C.c_int, vp, u64, u64, C.c_int, vp]
    lib.emu_check_range.restype = C.c_int; lib.emu_check_range.argtypes = [u64, u64, u64, vp]
    lib.emu_check_ranges.restype = C.c_int; lib.emu_check_ranges.argtypes = [C.c_int, vp, u64, u64, vp, u64, vp]
    lib.emu_check_edit.restype = C.c_int; lib.emu_check_edit.argtypes = [C.c_int, vp, u64, vp, u64, vp, u64, u64, C.c_int, vp, u64, vp, vp]
    lib.emu_calls_edit.restype = C.c_int; lib.emu_calls_edit.argtypes = [vp, u64, vp, u64, vp, u64, vp, u64, u64, u64, u32, vp, vp, vp, u64, vp, vp]
    # the calls themselves, as tests/seekable_*cases.py declare them
    lib.emu_seekable_table.restype = u64; lib.emu_seekable_table.argtypes = [vp, u64, u32, u32, vp, vp, vp, u64, vp, vp, vp]
    lib.emu_seekable_range.restype = C.c_int; lib.emu_seekable_range.argtypes = [vp, u64, vp, u64, u64, vp, i64, vp, vp, vp]
    lib.emu_seekable_xxh64.restype = u64; lib.emu_seekable_xxh64.argtypes = [vp, u32]
    lib.emu_records_compress.restype = u64; lib.emu_records_compress.argtypes = [vp, u64, vp, u32, u64, u64, u32, vp, vp, vp, u64, vp, vp, vp, vp]
    lib.emu_gather_plan.restype = C.c_int; lib.emu_gather_plan.argtypes = [vp, u64, vp, u64, u64, u64, vp, vp, u64, vp, u64, vp, u64, vp]
    lib.emu_gather_run.restype = C.c_int; lib.emu_gather_run.argtypes = [vp, u64, vp, vp, u64, vp, u64, u64, i64, i64, i32, vp, vp, vp, u64]
    lib.emu_edit_run.restype = C.c_int
    lib.emu_edit_run.argtypes = [vp, u64, vp, u32, vp, vp, u32, vp, vp, vp, vp, i32, vp, u32, vp, u64, u32, vp, vp, vp, vp]
    ids = np.zeros(4, dtype=np.uint32)
    lib.emu_calls_ids(ids.ctypes.data)
    assert ids.tolist() == [18, COMPACT, COMPRESS, DECOMPRESS]
    yield lib
    lib.emu_calls_mode(1, 0)


# ------------------------------------------------------------------------------------------------ layouts
GOLDEN = json.load(open(os.path.join(HERE, "golden", "seekable_layouts.json")))


def _layout(lib, kind, *params):
    """-> ({area: [(offset, bytes)]}, {area: reserved bytes})"""
    p = np.array(list(params) + [0], dtype=np.uint64)
    out = np.zeros((40, 3), dtype=np.uint64)
    rows = int(lib.emu_calls_layout(kind, p.ctypes.data, out.ctypes.data))
    assert 0 < rows <= 40
    arrays, total = {}, {}
    for area, off, size in out[:rows].tolist():
        if size == (1 << 64) - 1:
            total[area] = off
        else:
            arrays.setdefault(area, []).append((off, size))
    assert set(arrays) == set(total)
    return arrays, total


def _check_layout(arrays, total, what):
    for area, rows in arrays.items():
        end = 0
        for off, size in sorted(rows):
            assert off % 16 == 0, (what, area, off)                 # every array starts 16-aligned today (so 8-aligned too)
            assert off >= end, "%s: two arrays of area %d overlap at %d" % (what, area, off)
            end = off + size
        assert end <= total[area], "%s: area %d ends at %d, %d are reserved" % (what, area, end, total[area])


@pytest.mark.parametrize("n", COUNTS)
def test_layouts_of_one_count(lib, n):
    for kind, name in ((0, "compress"), (1, "records"), (2, "range")):
        arrays, total = _layout(lib, kind, n)
        _check_layout(arrays, total, (name, n))
        assert total[0] == GOLDEN[name][str(n)], (name, n)
    arrays, total = _layout(lib, 5, n)
    _check_layout(arrays, total, ("open", n))
    assert [total[0], total[1]] == GOLDEN["open"][str(n)]
    assert len(arrays[0]) == 3 and len(arrays[1]) == 6


@pytest.mark.parametrize("count", COUNTS)
def test_layouts_of_many_ranges(lib, count):
    for R, S, J in ((count, count, count), (1, count, 0), (count, 1, 3)):
        arrays, total = _layout(lib, 3, R, S, J, count)
        _check_layout(arrays, total, ("ranges", R, S, J, count))
        assert [total[0], total[1]] == GOLDEN["ranges"]["%d,%d,%d,%d" % (R, S, J, count)]
        assert sorted(o for o, _ in arrays[0]) == [0, 32 * R, 32 * (R + S)], "the tables are uploaded back to back"


@pytest.mark.parametrize("in_place", [0, 1])
@pytest.mark.parametrize("n_records", [0, 1, 65])
@pytest.mark.parametrize("n", COUNTS)
def test_layouts_of_edit(lib, n, n_records, in_place):
    for entry in (8, 12):
        arrays, total = _layout(lib, 4, n, n_records, n, in_place, entry)
        _check_layout(arrays, total, ("edit", n, n_records, in_place, entry))
        assert total[0] == GOLDEN["edit"]["%d,%d,%d,%d" % (n, n_records, in_place, entry)]
        first = min(off for off, _ in arrays[0][-10:])
        assert first == (GOLDEN["records"][str(n_records)] if n_records else 0), "the edit's arrays lie behind the records layout only when there are records"


# ------------------------------------------------------------------------------------------------ launch traces
def _lane_grid(cu, lanes):
    return min(max((lanes + 63) // 64, 1), cu * 8)


def _scan(n):
    g = min(max((n + SCAN_TILE - 1) // SCAN_TILE, 1), SCAN_GRID)          # zsk_scan_shape
    return [(SCAN_REDUCE, g), (SCAN_WRITE, g)]


def _tail(cu, n, table_kernel):
    return _scan(n) + [(VERDICT, 1), (table_kernel, _lane_grid(cu, n))] + ([(COMPACT, min(n, cu * 16))] if n else [])


def _want_compress(cu, n):
    return ([(CHUNK_SEGS, _lane_grid(cu, n)), (COMPRESS, n)] if n else []) + _tail(cu, n, TABLE)


def _want_records_front(cu, n):
    return _scan(n) + _scan(n) + [(RECORDS_VERDICT, 1)] + ([(RECORDS_SEGS, _lane_grid(cu, n)), (COMPRESS, n)] if n else [])


def _want_records(cu, n):
    return _want_records_front(cu, n) + _tail(cu, n, RECORDS_TABLE)


def _want_picks(cu, n, capacity):
    return [(EDIT_SIZES, _lane_grid(cu, n))] + _scan(n) + _scan(n) + [(EDIT_VERDICT, 1), (EDIT_COPY, min(capacity // COPY_TILE + n + 1, cu * 32)), (EDIT_TABLE, _lane_grid(cu, n))]


def _trace(lib):
    out = np.zeros((4096, 2), dtype=np.uint32)
    n = int(lib.emu_calls_trace(out.ctypes.data, 4096))
    return [tuple(r) for r in out[:n].tolist()]


MODES = [(1, 0), (256, 1)]           # one CU with the lanes running; 256 CUs, the launches recorded only


@pytest.fixture(params=MODES, ids=["1cu", "256cu-trace"])
def mode(lib, request):
    lib.emu_calls_mode(*request.param)
    yield request.param
    lib.emu_calls_mode(1, 0)


@pytest.mark.parametrize("n", [0, 3])
def test_trace_compress(lib, mode, n):
    cu, trace_only = mode
    frame_size = 1000
    src = sc.source((n - 1) * frame_size + 137) if n else b""
    s = np.frombuffer(src, dtype=np.uint8).copy() if src else np.zeros(1, dtype=np.uint8)
    sizes = np.array([50 + i for i in range(n)] or [0], dtype=np.uint64); st = np.zeros(max(n, 1), dtype=np.int32)
    cap = int(sizes[:n].sum()) + rec.table_size(n, False)
    dst = np.zeros(cap + 64, dtype=np.uint8); ssegs = np.zeros((max(n, 1), 2), dtype=np.uint64); dsegs = np.zeros((max(n, 1), 2), dtype=np.uint64); out = np.full(2, -1, dtype=np.int32)
    size = lib.emu_seekable_table(s.ctypes.data, len(src), frame_size, 0, sizes.ctypes.data, st.ctypes.data, dst.ctypes.data, cap, ssegs.ctypes.data, dsegs.ctypes.data, out.ctypes.data)
    assert _trace(lib) == _want_compress(cu, n)
    if not trace_only:
        assert size == cap and out.tolist() == [0, 0]


@pytest.mark.parametrize("n", [0, 5])
def test_trace_records(lib, mode, n):
    cu, trace_only = mode
    lengths = [100, 0, 4096, 1, 700][:n]
    records, src_size = rec.layout(lengths, np.random.default_rng(2))
    sizes = [min(40 + i, rec.compress_bound(l)) for i, l in enumerate(lengths)]
    r = rec.run_compress(lib, sc.source(src_size), records, sum(lengths), max(lengths + [0]), False, sizes)
    assert _trace(lib) == _want_records(cu, n)
    if not trace_only:
        assert r["status"] == [0, 0] and r["refused"] is None and r["copied"] == n and r["size"] == sum(sizes) + rec.table_size(n, False)


def _five_frames(lib):
    sizes = [(30, 4096)] * 5
    content = sc.source(5 * 4096)
    frames = [bytes([i]) * c for i, (c, _) in enumerate(sizes)]
    return sc.stream_of(frames, sc.chunks(content, 4096), False), content


@pytest.mark.parametrize("offset,length,frames,count,edge", [(4100, 50, 1, 1, 4096), (4000, 8000, 3, 3, 8192)], ids=["inside-one-frame", "across-three"])
def test_trace_range(lib, mode, offset, length, frames, count, edge):
    cu, trace_only = mode
    stream, content = _five_frames(lib)
    buf = np.frombuffer(stream, dtype=np.uint8).copy(); c = np.frombuffer(content, dtype=np.uint8).copy()
    dst = np.zeros(length, dtype=np.uint8); out = np.full(2, -1, dtype=np.int32); cnt = C.c_uint32(0)
    assert lib.emu_seekable_range(buf.ctypes.data, len(stream), c.ctypes.data, offset, length, dst.ctypes.data, -1, out.ctypes.data, None, C.byref(cnt)) == 0
    assert _trace(lib) == [(RANGE_SEGS, _lane_grid(cu, frames)), (DECOMPRESS, count), (RANGE_VERIFY, _lane_grid(cu, count)), (RANGE_FINISH, _lane_grid(cu, edge // 16 + 1))]
    if not trace_only:
        assert out.tolist() == [0, 0] and dst.tobytes() == content[offset:offset + length]


def test_trace_ranges_in_two_passes(lib, mode):
    cu, trace_only = mode
    stream, content = _five_frames(lib)
    # frames 0 and 3 are cut: 8 192 bytes of scratch frames under a limit of 4 096 -- a pass each; frame 2 lies wholly inside its range and decodes in place
    ranges = [(100, 300, 0), (8192, 4096, 6000), (13000, 100, 11000)]
    cap = 12000
    stats, segs, jobs, passes, _ = _plan(lib, stream, ranges, cap, 4096)
    assert len(passes) == 2 and stats[1] == 1
    rc, status, dst, _, _ = rc_.run(lib, stream, content, ranges, cap, 4096)
    assert rc == 0
    R, want = len(ranges), []
    for p, (scratch, item0, item1, tiles) in enumerate(passes):
        frames = sum(s[1] for s in segs if s[5] == p)
        last = p + 1 == len(passes)
        want.append((GATHER_SEGS, _lane_grid(cu, frames)))
        if item1 > item0:
            want += [(DECOMPRESS, item1 - item0), (GATHER_VERIFY, _lane_grid(cu, item1 - item0))]
        if tiles or last:
            want.append((GATHER_FINISH, _lane_grid(cu, tiles * 64 if tiles * 64 > (R if last else 0) else R)))
    assert _trace(lib) == want
    if not trace_only:
        assert status == [0] * (2 + 2 * R)
        for off, ln, at in ranges:
            assert dst[at:at + ln].tobytes() == content[off:off + ln]


def _plan(lib, stream, ranges, capacity, limit):
    """emu_gather_plan -> (stats, segments [first, frames, item, home, inPlace, pass], jobs, passes [scratch, item0, item1, tiles], ranges' frames)"""
    buf = np.frombuffer(stream, dtype=np.uint8).copy(); rg = rc_.ranges_array(ranges)
    stats = np.zeros(8, dtype=np.uint64); segs = np.zeros((64, 6), dtype=np.uint64); jobs = np.zeros((64, 4), dtype=np.uint64); passes = np.zeros((64, 4), dtype=np.uint64)
    fr = np.zeros((len(ranges), 2), dtype=np.uint64)
    assert lib.emu_gather_plan(buf.ctypes.data, len(stream), rg.ctypes.data, len(ranges), capacity, limit, stats.ctypes.data, segs.ctypes.data, 64, jobs.ctypes.data, 64,
                               passes.ctypes.data, 64, fr.ctypes.data) == 0
    return stats.tolist(), segs[:int(stats[5])].tolist(), jobs[:int(stats[3])].tolist(), passes[:int(stats[4])].tolist(), fr.tolist()


@pytest.mark.parametrize("in_place", [False, True], ids=["out-of-place", "in-place"])
def test_trace_edit_without_records(lib, mode, in_place):
    cu, trace_only = mode
    rng = np.random.default_rng(5)
    old = ec.random_stream(rng, [40, 5000, 0, 17], False)
    picks = ec.identity_picks(4) if in_place else [(ec.FRAME, 3), (ec.FRAME, 1)]
    c = ec.new_case(old=old, picks=picks, capacity=len(old) + 64, in_place=in_place)
    r = ec.run(lib, c)
    assert r["rc"] == 0 and _trace(lib) == _want_picks(cu, len(picks), c["capacity"])
    if not trace_only:
        assert r["in_place"] == in_place and r["status"] == [0, 0] and r["dst"][:r["size"]].tobytes() == ec.expected_stream(c)


@pytest.mark.parametrize("in_place", [False, True], ids=["out-of-place", "in-place"])
def test_trace_edit_with_records(lib, mode, in_place):
    """the whole call: the records' front half, then the per-pick half -- its arrays behind the records layout in the same area"""
    cu, trace_only = mode
    rng = np.random.default_rng(6)
    frame_sizes = [40, 5000, 17]
    old = ec.random_stream(rng, frame_sizes, True)
    lengths = [300, 0, 4500]
    records, src_size = rec.layout(lengths, rng, shuffle=False)
    src = sc.source(src_size)
    given = [25, 9, 4200]
    picks = ec.identity_picks(3) + [(ec.RECORD, 2), (ec.RECORD, 0)] if in_place else [(ec.RECORD, 1), (ec.FRAME, 2), (ec.RECORD, 2), (ec.FRAME, 0)]
    cap = len(old) + sum(given) + 200
    dst = np.full(cap + 64, 0x5A, dtype=np.uint8)
    if in_place:
        dst[:len(old)] = np.frombuffer(old, dtype=np.uint8); old_ptr = dst.ctypes.data
    else:
        old_buf = np.frombuffer(old, dtype=np.uint8).copy(); old_ptr = old_buf.ctypes.data
    pk = np.array(picks, dtype=np.uint32); s8 = np.frombuffer(src, dtype=np.uint8).copy(); r64 = rec.records_array(records)
    sz = np.array(given, dtype=np.uint64); st = np.zeros(3, dtype=np.int32); out = np.full(2, -1, dtype=np.int32); info = np.zeros(4, dtype=np.uint64)
    rc = lib.emu_calls_edit(old_ptr, len(old), pk.ctypes.data, len(picks), s8.ctypes.data, len(src), r64.ctypes.data, 3, sum(lengths), max(lengths), 1, sz.ctypes.data, st.ctypes.data,
                            dst.ctypes.data, cap, out.ctypes.data, info.ctypes.data)
    assert rc == 0 and _trace(lib) == _want_records_front(cu, 3) + _want_picks(cu, len(picks), cap)
    if trace_only:
        return
    assert out.tolist() == [0, 0] and int(info[1]) == 1 and int(info[2]) == 0 and (dst[cap:] == 0x5A).all()
    entries, ck, at = sc.parse(dst[:int(info[0])].tobytes())
    old_entries, _, _ = sc.parse(old)
    old_at = np.cumsum([0] + [e[0] for e in old_entries])
    assert ck and len(entries) == len(picks)
    pos = 0
    for (kind, i), e in zip(picks, entries):
        if kind == ec.FRAME:
            assert e == old_entries[i] and dst[pos:pos + e[0]].tobytes() == old[old_at[i]:old_at[i] + e[0]]
        else:
            off, ln = records[i]
            assert e == (given[i], ln, sc.xxh64(src[off:off + ln]) & 0xFFFFFFFF) and dst[pos:pos + e[0]].tobytes() == rec.stand_in_frame(i, given[i])
        pos += e[0]
    assert pos == at


# ------------------------------------------------------------------------------------------------ the host checks: the library's codes and texts
def _text(buf):
    return buf.value.decode()


def test_refusals_of_the_compress_calls(lib):
    t = C.create_string_buffer(256)
    assert lib.emu_check_compress(1, 1000, 100, 0, t) == 0 and lib.emu_check_compress(1, 0, 4096, 1, t) == 0
    for args in ((0, 1000, 100, 0), (1, 1000, 100, 2)):
        assert lib.emu_check_compress(*args, t) == UNSUPPORTED and _text(t) == "seekable compress: bad arguments"
    for args in ((1, 1000, 0, 0), (1, 1000, (1 << 30) + 1, 0), (1, (1 << 27) + 1, 1, 0)):
        assert lib.emu_check_compress(*args, t) == UNSUPPORTED and _text(t) == "seekable compress: frameSize must be 1 ... 2^30 and the frame count at most 2^27"
    r = np.zeros(2, dtype=np.uint64)
    assert lib.emu_check_records(1, r.ctypes.data, 1, 1 << 30, 1, t) == 0 and lib.emu_check_records(1, None, 0, 0, 0, t) == 0
    for args in ((0, r.ctypes.data, 1, 10, 0), (1, None, 1, 10, 0), (1, r.ctypes.data, 1, 10, 4)):
        assert lib.emu_check_records(*args, t) == UNSUPPORTED and _text(t) == "seekable compress: bad arguments"
    for args in ((1, r.ctypes.data, (1 << 27) + 1, 10, 0), (1, r.ctypes.data, 1, (1 << 30) + 1, 0)):
        assert lib.emu_check_records(*args, t) == UNSUPPORTED and _text(t) == "seekable compress: at most 2^27 records of at most 2^30 bytes"


def test_refusals_of_the_readers(lib):
    t = C.create_string_buffer(256)
    assert lib.emu_check_range(0, 100, 100, t) == 0 and lib.emu_check_range(100, 0, 100, t) == 0
    assert lib.emu_check_range(1, 100, 100, t) == SIZE_MISMATCH and _text(t) == "seekable decompress: the range ends at 101, the content at 100"
    assert lib.emu_check_range(1 << 63, 1 << 63, 100, t) == SIZE_MISMATCH and _text(t) == "seekable decompress: the range ends at 0, the content at 100"
    good = [(0, 10, 0), (50, 20, 10)]
    dst = np.zeros(8, dtype=np.uint8)

    def ranges(rg, pointers=1, d=dst.ctypes.data, cap=1000, content=100):
        a = rc_.ranges_array(rg)
        return lib.emu_check_ranges(pointers, a.ctypes.data if rg is not None else None, len(rg or ()), content, d, cap, t)

    assert ranges(good) == 0 and ranges([]) == 0 and ranges([(5, 0, 3)], d=None) == 0
    assert ranges(good, pointers=0) == UNSUPPORTED and _text(t) == "seekable ranges: bad arguments (NULL, or more than 2^27 ranges)"
    assert lib.emu_check_ranges(1, None, 2, 100, dst.ctypes.data, 1000, t) == UNSUPPORTED and _text(t) == "seekable ranges: bad arguments (NULL, or more than 2^27 ranges)"
    assert lib.emu_check_ranges(1, dst.ctypes.data, (1 << 27) + 1, 100, dst.ctypes.data, 1000, t) == UNSUPPORTED
    assert ranges(good + [(95, 6, 400)]) == SIZE_MISMATCH and _text(t) == "seekable ranges: range 2 ends at 95 + 6, the content at 100"
    assert ranges(good + [(0, 6, 995)]) == SIZE_MISMATCH and _text(t) == "seekable ranges: range 2 goes to 995 + 6, the capacity is 1000"
    assert ranges(good + [(0, 6, 29)]) == UNSUPPORTED and _text(t) == "seekable ranges: the destinations of ranges 1 and 2 overlap"
    assert ranges(good, d=None) == UNSUPPORTED and _text(t) == "seekable ranges: bad arguments (no destination)"


def test_refusals_of_edit(lib):
    t = C.create_string_buffer(256)
    rng = np.random.default_rng(9)
    old = ec.random_stream(rng, [40, 500, 17], True)
    room = np.zeros(len(old) + 4096, dtype=np.uint8)
    room[:len(old)] = np.frombuffer(old, dtype=np.uint8)
    elsewhere = np.zeros(4096, dtype=np.uint8)
    r = np.zeros(4, dtype=np.uint64)
    F, R = ec.FRAME, ec.RECORD

    def edit(picks, pointers=1, use_old=True, n_records=2, records=r.ctypes.data, max_record=100, flags=1, dst=elsewhere.ctypes.data, cap=4096):
        pk = np.array(picks or [(0, 0)], dtype=np.uint32)
        ip = C.c_uint32(7)
        rc = lib.emu_check_edit(pointers, room.ctypes.data if use_old else None, len(old) if use_old else 0, pk.ctypes.data, len(picks), records, n_records, max_record, flags, dst, cap,
                                C.byref(ip), t)
        return rc, ip.value, _text(t)

    assert edit([(F, 2), (R, 1)])[:2] == (0, 0)
    assert edit(ec.identity_picks(3) + [(R, 0)], dst=room.ctypes.data, cap=len(room))[:2] == (0, 1), "append in place"
    for kw in (dict(pointers=0), dict(dst=None), dict(records=None), dict(flags=3)):
        assert edit([(F, 0)], **kw)[::2] == (UNSUPPORTED, "seekable edit: bad arguments")
    assert edit([(R, 0)], n_records=(1 << 27) + 1)[::2] == (UNSUPPORTED, "seekable edit: at most 2^27 records of at most 2^30 bytes")
    assert edit([(R, 0)], max_record=(1 << 30) + 1)[::2] == (UNSUPPORTED, "seekable edit: at most 2^27 records of at most 2^30 bytes")
    assert edit([(F, 0)], flags=0)[::2] == (UNSUPPORTED, "seekable edit: ZHIP_SEEKABLE_CHECKSUM must be set exactly when the opened stream's table has checksums")
    assert edit([(F, 0), (2, 0)])[::2] == (UNSUPPORTED, "seekable edit: position 1 is neither a frame nor a record pick")
    assert edit([(R, 0), (F, 0)], use_old=False)[::2] == (UNSUPPORTED, "seekable edit: position 1 is a frame pick, and no stream is opened")
    assert edit([(F, 3)])[::2] == (SIZE_MISMATCH, "seekable edit: position 0 names frame 3, there are 3")
    assert edit([(F, 0), (R, 2)])[::2] == (SIZE_MISMATCH, "seekable edit: position 1 names record 2, there are 2")
    overlap = "seekable edit: the destination overlaps the opened stream (allowed only at its base, with picks that begin with every frame in order)"
    assert edit([(F, 1), (F, 0), (F, 2)], dst=room.ctypes.data, cap=len(room))[::2] == (UNSUPPORTED, overlap), "at the base, but not an append"
    assert edit(ec.identity_picks(3), dst=room.ctypes.data + 8, cap=len(room) - 8)[::2] == (UNSUPPORTED, overlap), "an append, but not at the base"


def test_the_emulated_calls_return_the_librarys_codes(lib):
    """the entries of tests/emu/emu_seekable*.cpp no longer map refusals by hand: what they return is what the shared checks return"""
    stream, content = _five_frames(lib)
    buf = np.frombuffer(stream, dtype=np.uint8).copy(); c = np.frombuffer(content, dtype=np.uint8).copy()
    dst = np.zeros(64, dtype=np.uint8); out = np.full(2, -1, dtype=np.int32)
    assert lib.emu_seekable_range(buf.ctypes.data, len(stream), c.ctypes.data, len(content) - 1, 2, dst.ctypes.data, -1, out.ctypes.data, None, None) == SIZE_MISMATCH
    assert rc_.run(lib, stream, content, [(0, 10, 0), (20, 10, 5)], 100)[0] == UNSUPPORTED
    assert rc_.run(lib, stream, content, [(len(content), 1, 0)], 100)[0] == SIZE_MISMATCH
    old = ec.random_stream(np.random.default_rng(3), [40, 500], False)
    assert ec.run(lib, ec.new_case(old=old, picks=[(ec.FRAME, 2)], capacity=4096))["rc"] == SIZE_MISMATCH
    assert ec.run(lib, ec.new_case(old=old, picks=[(2, 0)], capacity=4096))["rc"] == UNSUPPORTED
