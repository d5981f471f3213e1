"""Chains of xor-with-base links (python-zstandard_amd/csrc/zhip_seekable_typed.hpp and zhip_seekable_typed_calls.hpp) on the host wave
emulator, against the numpy model of tests/chain_model.py: the chain join body over the shapes at which it takes another path, with 1, 2, 3 and 16 links, with
and without a base; its properties; the whole call over one emulator backend per link, on chains written with the emulated compress calls, over the range sets
of tests/seekable_range_cases.py; damaged frames in one and in two links; every refusal; the stand-alone sanitizer program; and the sizes the feature is there
for (libzstd alone). No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import chain_model as cm
from tests import delta_model as dm
from tests import planes_model as pm
from tests import reflib
from tests import seekable_range_cases as rc_cases
from tests import xor_model as xm

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
UNSUPPORTED = 6
GUARD = 64
FRAME = 4096
ELEMENTS = 3 * FRAME + 37
T_TYPED = 100                       # the trace's name of typed kernel k: 100 + k
K_JOIN_CHAIN, K_STATUS_CHAIN = 11, 12
T_KERNELS = set(range(T_TYPED, T_TYPED + 13))
LIMITS = (0, 4096)                  # the default scratch limit, and one that forces several passes


def _guarded(n, offset, fill=0x5A):
    """(the whole buffer, the view of n bytes at `offset` bytes behind a 64-byte aligned guard)"""
    raw = np.full(n + 2 * GUARD + 64 + offset, fill, dtype=np.uint8)
    skew = (-raw.ctypes.data) % 64
    at = skew + GUARD + offset
    return raw, raw[at:at + n], at


def _intact(raw, at, n, fill=0x5A):
    return (raw[:at] == fill).all() and (raw[at + n:] == fill).all()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("emu_seekable_chain")), "libzhip_emu_seekable_chain.so")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + EMU, "-w", "-o", out, os.path.join(EMU, "zhemu.cpp"), os.path.join(EMU, "emu_seekable_chain.cpp")])
    lib = C.CDLL(out)
    vp, u64, u32, i32, i64, ci = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_int64, C.c_int
    lib.emu_chain_join.restype = None; lib.emu_chain_join.argtypes = [vp, u32, vp, vp, vp, u32, u64, u32, u32, u32]
    lib.emu_chain_planes_call.restype = ci; lib.emu_chain_planes_call.argtypes = [vp, u64, u64, u32, u32, vp, ci, vp, vp, u64, vp, vp]
    lib.emu_chain_open.restype = vp; lib.emu_chain_open.argtypes = [vp, vp, u64, vp]
    lib.emu_chain_close.restype = None; lib.emu_chain_close.argtypes = [vp]
    lib.emu_chain_link_info.restype = None; lib.emu_chain_link_info.argtypes = [vp, u64, vp]
    lib.emu_chain_ranges.restype = ci; lib.emu_chain_ranges.argtypes = [vp, vp, u64, vp, vp, i32, vp, u64, vp, u64, vp, u64, u64, vp, vp, vp, vp, u64, vp, vp]
    lib.emu_chain_single.restype = ci; lib.emu_chain_single.argtypes = [vp, u64, vp, vp, u64, vp, u64, vp, u64, u64, vp, vp, vp, u64, vp]
    # the entries of before, in this library too
    lib.emu_xor_join.restype = None; lib.emu_xor_join.argtypes = [vp, vp, vp, vp, u32, u64, u32, u32, u32]
    lib.emu_planes_join.restype = None; lib.emu_planes_join.argtypes = [vp, vp, vp, u32, u64, u32, u32, u32]
    lib.emu_xor_compress.restype = ci; lib.emu_xor_compress.argtypes = [vp, vp, u64, u32, u32, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp]
    lib.emu_delta_compress.restype = ci; lib.emu_delta_compress.argtypes = [ci, u32, vp, u64, u32, u32, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp]
    lib.emu_typed_plain.restype = u64; lib.emu_typed_plain.argtypes = [vp, u64, u32, u32, vp, vp, ci, vp, u64, vp]
    lib.emu_typed_grid.restype = u32; lib.emu_typed_grid.argtypes = [ci, u64, u32, u32]
    lib.emu_typed_bound.restype = u64; lib.emu_typed_bound.argtypes = [u64, u32, u32, ci]
    return lib


def _pointers(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def _chain_join(lib, planars, base, dst, jobs, size, k, group, grid):
    table = None if jobs is None else np.array(jobs, dtype=np.uint64)
    lib.emu_chain_join(_pointers(planars), len(planars), None if base is None else base.ctypes.data, dst.ctypes.data, None if jobs is None else table.ctypes.data,
                       0 if jobs is None else len(jobs), size, k, group, grid)


# ------------------------------------------------------------------------------------------------ the body
@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("m", xm.GROUP_SIZES)
def test_chain_join_body(lib, k, m):
    """1, 2, 3 and 16 planar buffers of one layout, with and without a base, on every shape: the output is the model's; guard bytes around every buffer; byte
    offsets 0, 1 and 3; no input changes"""
    turn = 0
    for elements in xm.shapes(m):
        size = elements * k
        grid = lib.emu_typed_grid(1, size, k, m)
        for n_links in cm.LINK_COUNTS:
            data = cm.random_planars(k, elements, n_links, seed=100 * k + m + n_links)
            for with_base in (False, True):
                off = (0, 1, 3)[turn % 3]; turn += 1
                held = [_guarded(size, (off + i) % 4 if i % 2 else off) for i in range(n_links)]
                for (_, view, _), d in zip(held, data):
                    view[:] = d
                base = xm.source(k, elements, seed=7 + turn) if with_base else None
                raw_b, b, at_b = _guarded(size, (off + 2) % 4)
                if with_base:
                    b[:] = base
                raw, out, at = _guarded(size, (off + 1) % 4 if off else 0)
                _chain_join(lib, [v for _, v, _ in held], b if with_base else None, out, None, size, k, m, grid)
                assert (out == cm.join_chain(data, base, k, m)).all(), (k, m, elements, n_links, with_base)
                assert _intact(raw, at, size) and _intact(raw_b, at_b, size) and (not with_base or (b == base).all())
                assert all(_intact(r, a, size) and (v == d).all() for (r, v, a), d in zip(held, data))


@pytest.mark.parametrize("k", [2, 4, 8])
def test_fewer_waves_than_tiles(lib, k):
    """the grid-stride loop's later trips: 3 groups of 2 500 elements are 9 tiles, on 1 and on 4 workgroups"""
    m, elements = 2500, 3 * 2500
    size = elements * k
    for n_links in (2, 3):
        data = cm.random_planars(k, elements, n_links, seed=k)
        base = xm.source(k, elements, seed=70 + k)
        for grid in (1, 4):
            for b in (None, base):
                raw, out, at = _guarded(size, 3)
                _chain_join(lib, data, b, out, None, size, k, m, grid)
                assert (out == cm.join_chain(data, b, k, m)).all() and _intact(raw, at, size)


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("n_links", cm.LINK_COUNTS)
def test_join_jobs_with_trims_and_content_offsets(lib, k, n_links):
    """jobs of 1 ... 2 100 elements that trim their first and last element, their base bytes anywhere in the base and their destinations in another order, all
    in ONE launch over n_links planar buffers of the same layout: every job's output is its slice of the joined XOR of the links, XOR the base bytes at ITS
    content offset; without a base the content offsets are not read (the emulator entry hands the kernel none)"""
    rng = np.random.default_rng(43 + k + 10 * n_links)
    total = 9000 * k
    base = rng.integers(0, 256, total, dtype=np.uint8)
    jobs, pieces, pieces0, planar, at_p = [], [], [], [[] for _ in range(n_links)], 0
    for m in (1, 15, 16, 17, 37, 1024, 1030, 2100):
        for h, t in ((0, 0), (1, 0), (0, 1), (k - 1, k - 1)):
            if h + t >= m * k:
                continue
            content = int(rng.integers(0, total // k - m + 1)) * k
            xs = [rng.integers(0, 256, m * k, dtype=np.uint8) for _ in range(n_links)]      # every link's filtered elements
            acc = np.zeros(m * k, dtype=np.uint8)
            for i, x in enumerate(xs):
                planar[i].append(x.reshape(m, k).T.reshape(-1)); acc ^= x
            pieces.append((acc ^ base[content:content + m * k])[h:m * k - t]); pieces0.append(acc[h:m * k - t])
            jobs.append([at_p, m, 0, h, t, content])
            at_p += m * k
    at_d = 0
    for j in rng.permutation(len(jobs)):                                 # the destinations: another order than the planar buffers'
        jobs[j][2] = at_d; at_d += pieces[j].size
    planar = [np.concatenate(p) for p in planar]
    for with_base, parts in ((True, pieces), (False, pieces0)):
        want = np.zeros(at_d, dtype=np.uint8)
        for job, piece in zip(jobs, parts):
            want[job[2]:job[2] + piece.size] = piece
        for off, grid in ((0, 8), (1, 3), (3, 1)):
            held = [_guarded(p.size, (off + i) % 4) for i, p in enumerate(planar)]
            for (_, v, _), p in zip(held, planar):
                v[:] = p
            raw_b, b, at_b = _guarded(total, (off + 1) % 4); b[:] = base
            raw, d, at = _guarded(want.size, off)
            _chain_join(lib, [v for _, v, _ in held], b if with_base else None, d, jobs, 0, k, 1, grid)
            assert (d == want).all(), (k, off, with_base)
            assert _intact(raw, at, want.size) and (b == base).all() and _intact(raw_b, at_b, total)


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("k", [2, 4, 8])
def test_one_link_is_the_join_of_before(lib, k):
    """nLinks = 1 with a base is planes_join_xor byte for byte; without a base it is planes_join"""
    m, elements = 1025, 2 * 1025 + 17
    size = elements * k
    planar = cm.random_planars(k, elements, 1, seed=k)[0]; base = xm.source(k, elements, seed=3)
    grid = lib.emu_typed_grid(1, size, k, m)
    got = np.zeros(size, dtype=np.uint8); old = np.zeros(size, dtype=np.uint8)
    _chain_join(lib, [planar], base, got, None, size, k, m, grid)
    lib.emu_xor_join(planar.ctypes.data, base.ctypes.data, old.ctypes.data, None, 0, size, k, m, grid)
    assert got.tobytes() == old.tobytes() == xm.join(planar, base, k, m).tobytes()
    _chain_join(lib, [planar], None, got, None, size, k, m, grid)
    lib.emu_planes_join(planar.ctypes.data, old.ctypes.data, None, 0, size, k, m, grid)
    assert got.tobytes() == old.tobytes() == pm.join(planar, k, m).tobytes()


@pytest.mark.parametrize("k", [2, 4, 8])
def test_equal_links_cancel_and_order_does_not_matter(lib, k):
    """two equal planar buffers in the chain give the base back; the result does not depend on the order of the links"""
    m, elements = 1024, 2 * 1024 + 15
    size = elements * k
    a, b2, c = cm.random_planars(k, elements, 3, seed=20 + k); base = xm.source(k, elements, seed=4)
    grid = lib.emu_typed_grid(1, size, k, m)
    out = np.zeros(size, dtype=np.uint8)
    _chain_join(lib, [a, a.copy()], base, out, None, size, k, m, grid)
    assert (out == base).all()
    _chain_join(lib, [a, b2, a.copy(), b2.copy()], None, out, None, size, k, m, grid)
    assert not out.any()
    results = []
    for order in ([a, b2, c], [c, a, b2], [b2, c, a], [c, b2, a]):
        _chain_join(lib, order, base, out, None, size, k, m, grid)
        results.append(out.tobytes())
    assert len(set(results)) == 1 and results[0] == cm.join_chain([a, b2, c], base, k, m).tobytes()


def test_planes_join_chain_call(lib):
    """the stand-alone call: one chain join on the plain join's grid; its refusals launch and write nothing"""
    k, m = 4, 1025
    elements = 3 * m + 17; size = elements * k
    data = cm.random_planars(k, elements, 3, seed=1); base = xm.source(k, elements, seed=2)
    grid = lib.emu_typed_grid(1, size, k, m)

    def call(planars, n, size_, k_, m_, mode):
        dst = np.full(size, 0x5A, dtype=np.uint8)
        trace = np.zeros(16, dtype=np.uint32); words = np.zeros(1, dtype=np.uint64); text = C.create_string_buffer(256)
        ptrs = (C.c_void_p * max(len(planars), 1))(*[None if p is None else p.ctypes.data for p in planars])
        rc = lib.emu_chain_planes_call(ptrs, n, size_, k_, m_, base.ctypes.data, mode, dst.ctypes.data, trace.ctypes.data, 16, words.ctypes.data, text)
        return rc, dst, trace[:int(words[0])].tolist(), text.value

    for mode, b in ((0, None), (1, base)):
        rc, out, trace, _ = call(data, 3, size, k, m, mode)
        assert rc == 0 and (out == cm.join_chain(data, b, k, m)).all() and trace == [T_TYPED + K_JOIN_CHAIN, grid]
    many = [data[0]] * 17
    for args, word in (((data, 0, size, k, m, 1), b"links"), ((many, 17, size, k, m, 1), b"links"), (([data[0], None, data[2]], 3, size, k, m, 1), b"link 1"),
                       ((data, 3, size, 3, m, 1), b"element size"), ((data, 3, size - 1, k, m, 1), b"multiple"), ((data, 3, size, k, 0, 1), b"frameSize"),
                       ((data, 3, size, k, m, 2), b"overlaps")):
        rc, out, trace, text = call(*args)
        assert rc == UNSUPPORTED and trace == [] and (out == 0x5A).all() and word in text, (args[1:], text)


# ------------------------------------------------------------------------------------------------ the whole call
_built = {}


def _frames_of(planes):
    ref = reflib.checker()
    frames = [ref.compress(p, level=3) for p in planes]
    return np.frombuffer(b"".join(frames), dtype=np.uint8), np.cumsum([0] + [len(f) for f in frames]).astype(np.uint64)


def _write_link(lib, data, base, k, frame=FRAME, checksum=1):
    """a link's stream through the emulated compress calls: emu_delta_compress under filter 0 (no base), emu_xor_compress (a base)"""
    planes = pm.planes(data, k, frame) if base is None else xm.planes(data, base, k, frame)
    blob, offs = _frames_of(planes)
    bound = lib.emu_typed_bound(data.size, frame, k, checksum)
    d = np.zeros(bound, dtype=np.uint8); status = np.full(2, -1, dtype=np.int32); info = np.zeros(4, dtype=np.uint64)
    trace = np.zeros(64, dtype=np.uint32); words = np.zeros(1, dtype=np.uint64)
    if base is None:
        rc = lib.emu_delta_compress(1, 0, data.ctypes.data, data.size, frame, k, checksum, blob.ctypes.data, offs.ctypes.data, d.ctypes.data, bound, status.ctypes.data, None, info.ctypes.data,
                                    trace.ctypes.data, 64, words.ctypes.data, None)
    else:
        rc = lib.emu_xor_compress(data.ctypes.data, base.ctypes.data, data.size, frame, k, checksum, blob.ctypes.data, offs.ctypes.data, d.ctypes.data, bound, status.ctypes.data, None,
                                  info.ctypes.data, trace.ctypes.data, 64, words.ctypes.data, None)
    assert rc == 0 and status.tolist() == [0, 0]
    return d[:int(info[0])].copy()


class Chain:
    """the opened handles of a chain's links on the emulator, their planar contents, and the reader's base"""

    def __init__(self, lib, streams, contents, base):
        self.lib, self.streams, self.contents, self.base = lib, streams, contents, base
        bad = np.zeros(1, dtype=np.uint64)
        sizes = np.array([s.size for s in streams], dtype=np.uint64)
        self.handle = lib.emu_chain_open(_pointers(streams), sizes.ctypes.data, len(streams), bad.ctypes.data)
        assert self.handle, "link %d did not open" % int(bad[0])

    def read(self, table, capacity, limit=0, pick=None, damage=None, code=20, base="own", base_size=None, want_link=True):
        """table: [(offset, length, dstOffset)] -> (rc, the destination, status, link, stats, traces per link, text); damage: {handle index: frame}"""
        lib = self.lib
        pick = list(range(len(self.streams))) if pick is None else pick
        rg = rc_cases.ranges_array(table)
        raw, d, dat = _guarded(capacity, 1)
        b = self.base if isinstance(base, str) and base == "own" else base
        raw_b = at_b = None
        if isinstance(b, np.ndarray):
            raw_b, held, at_b = _guarded(b.size, 3); held[:] = b
            ptr, size = held.ctypes.data, b.size
        elif b == "dst":
            ptr, size = d.ctypes.data + max(capacity - 1, 0), self.contents[0].size
        else:
            ptr, size = None, 0
        status = np.full(2 + 2 * len(table), -1, dtype=np.int32); link = np.full(1 + len(table), -7, dtype=np.int32); stats = np.zeros(8, dtype=np.uint64)
        cap = 1 << 14
        traces = np.zeros((max(len(pick), 1), cap), dtype=np.uint32); words = np.zeros(max(len(pick), 1), dtype=np.uint64); text = C.create_string_buffer(256)
        frames = np.array([(damage or {}).get(i, -1) for i in range(len(self.streams))], dtype=np.int64)
        picks = np.array(pick if pick else [0], dtype=np.int64)
        rc = lib.emu_chain_ranges(self.handle, picks.ctypes.data, len(pick), _pointers(self.contents), frames.ctypes.data, code, ptr, size if base_size is None else base_size,
                                  rg.ctypes.data, len(table), d.ctypes.data, capacity, limit, status.ctypes.data, link.ctypes.data if want_link else None, stats.ctypes.data,
                                  traces.ctypes.data, cap, words.ctypes.data, text)
        assert _intact(raw, dat, capacity) and (raw_b is None or ((held == b).all() and _intact(raw_b, at_b, b.size)))
        assert all(int(w) <= cap for w in words)
        return rc, d.copy(), status.tolist(), link.tolist(), [int(x) for x in stats], [traces[i, :int(words[i])].tolist() for i in range(len(pick))], text.value

    def single(self, i, base, table, capacity, limit=0):
        """the single-stream typed read on handle i -> (rc, destination bytes, status, stats, trace)"""
        rg = rc_cases.ranges_array(table)
        d = np.full(capacity, 0x5A, dtype=np.uint8); status = np.full(2 + 2 * len(table), -1, dtype=np.int32); stats = np.zeros(7, dtype=np.uint64)
        trace = np.zeros(1 << 14, dtype=np.uint32); words = np.zeros(1, dtype=np.uint64)
        rc = self.lib.emu_chain_single(self.handle, i, self.contents[i].ctypes.data, None if base is None else base.ctypes.data, 0 if base is None else base.size, rg.ctypes.data, len(table),
                                       d.ctypes.data, capacity, limit, status.ctypes.data, stats.ctypes.data, trace.ctypes.data, trace.size, words.ctypes.data)
        return rc, d.tobytes(), status.tolist(), [int(x) for x in stats], trace[:int(words[0])].tolist()

    def close(self):
        self.lib.emu_chain_close(self.handle); self.handle = None


def _chain(lib, k, n_links, full):
    """(the versions, the chain of n_links links that reads the last one): full -- [full stream of v0, d1, ..., d(n-1)]; else [d1, ..., dn] and the base v0"""
    key = (k, n_links, full)
    if key not in _built:
        vs = cm.versions(k, ELEMENTS, n_links - 1 if full else n_links, seed=5 + k)
        sources, base = cm.link_sources(vs, full)
        streams = [_write_link(lib, data, b, k) for data, b in sources]
        contents = [cm.planar_of(data, b, k, FRAME) for data, b in sources]
        _built[key] = (vs, Chain(lib, streams, contents, base))
    return _built[key]


def _range_sets(k):
    """the range lists of tests/seekable_range_cases.py over the stream's groups in ELEMENT order (as tests/test_emu_seekable_xor_base.py takes them)"""
    d_off = np.array([min(g * FRAME * k, ELEMENTS * k) for g in range(5)], dtype=np.int64)
    out = []
    for seed, count in ((1, 0), (2, 3), (3, 9), (4, 40), (5, 64), (6, 130)):
        rng = np.random.default_rng(7100 + seed + k)
        out.append(rc_cases.place_destinations(rng, rc_cases.random_ranges(rng, d_off, count)))
    return out


def _typed(trace):
    return [t for t in trace[::2] if t in T_KERNELS]


def _plain(trace):
    return [(t, g) for t, g in zip(trace[::2], trace[1::2]) if t not in T_KERNELS]


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("n_links", [1, 2, 5])
@pytest.mark.parametrize("full", [True, False])
def test_chain_ranges(lib, k, n_links, full):
    """every range's bytes equal the slice of the LAST version, under the default scratch limit and under one that forces several passes; nothing outside the
    ranges' destinations is written; per pass every link runs exactly the many-ranges call a single-stream read of its handle runs, the first link's backend
    launches one chain join per pass and the reducer, and no kernel of the single-stream reads is launched"""
    vs, chain = _chain(lib, k, n_links, full)
    last = vs[-1]
    for table, capacity in _range_sets(k):
        for limit in LIMITS:
            rc, d, status, link, stats, traces, text = chain.read(table, capacity, limit=limit)
            assert rc == 0 and status == [0] * (2 + 2 * len(table)) and link == [-1] * (1 + len(table)), (k, n_links, full, len(table), limit, text)
            for o, n, to in table:
                assert d[to:to + n].tobytes() == last[o:o + n].tobytes(), (o, n, limit)
            assert (d[rc_cases.untouched_mask(table, capacity)] == 0x5A).all()
            if not any(n for _, n, _ in table):
                assert [_typed(t) for t in traces] == [[T_TYPED + K_STATUS_CHAIN]] + [[]] * (n_links - 1) and all(_plain(t) == [] for t in traces)
                continue
            passes = stats[4]
            assert _typed(traces[0]) == [T_TYPED + K_JOIN_CHAIN] * passes + [T_TYPED + K_STATUS_CHAIN] and passes >= 1
            assert all(_typed(t) == [] for t in traces[1:])
            if limit == 4096 and sum(n for _, n, _ in table) > 3 * 4096:
                assert passes > 1
            # the same ranges through the single-stream read of every handle: its many-ranges calls are the link's, launch for launch
            items = 0
            for i in range(n_links):
                b = cm.link_sources(vs, full)[0][i][1]                        # the link's own base: its predecessor (none: the full stream)
                rc1, _, status1, stats1, trace1 = chain.single(i, b, table, capacity, limit=limit)
                assert rc1 == 0 and not any(status1) and _plain(trace1) == _plain(traces[i]) and stats1[4] == passes, (i, limit)
                items += stats1[0]
            assert stats[0] == items and stats[7] == n_links * stats[5] and (limit == 0 or stats[5] <= max(limit, FRAME * k))


@pytest.mark.parametrize("k", [2, 4, 8])
def test_one_link_chain_is_the_single_stream_read(lib, k):
    """nLinks = 1: the destination, the status and the stats are the single-stream typed read's, byte for byte, with a base and without"""
    for full in (True, False):
        vs, chain = _chain(lib, k, 1, full)
        for table, capacity in _range_sets(k):
            for limit in LIMITS:
                rc, d, status, link, stats, traces, _ = chain.read(table, capacity, limit=limit)
                rc1, d1, status1, stats1, trace1 = chain.single(0, chain.base, table, capacity, limit=limit)
                assert (rc, status, stats[:5]) == (rc1, status1, stats1[:5]) and d.tobytes() == d1 and _plain(traces[0]) == _plain(trace1)


def test_single_stream_reads_around_a_chain_read(lib):
    """a single-stream typed read on one of the chain's handles before and after a chain read returns what it did"""
    vs, chain = _chain(lib, 4, 5, True)
    table, capacity = _range_sets(4)[3]
    before = [chain.single(i, vs[i - 1] if i else None, table, capacity, limit=4096) for i in (0, 2, 4)]
    rc, d, status, _, _, _, _ = chain.read(table, capacity, limit=4096)
    assert rc == 0 and not any(status)
    after = [chain.single(i, vs[i - 1] if i else None, table, capacity, limit=4096) for i in (0, 2, 4)]
    assert before == after and all(r[0] == 0 and not any(r[2]) for r in before)
    for (i, r) in zip((0, 2, 4), before):                                    # (and each of them reads ITS version)
        for o, n, to in table:
            assert r[1][to:to + n] == vs[i][o:o + n].tobytes()


# ------------------------------------------------------------------------------------------------ damage
def _damage_table(k):
    g = FRAME * k
    rg = [(10, 100), (g - 2, 4), (g, g), (2 * g + 1, 50), (0, ELEMENTS * k), (g + 77, 0), (2 * g - 1, 1), (2 * g, 1), (3 * g, 37 * k)]
    touches = [o < 2 * g and o + n > g and n > 0 for o, n in rg]
    table, at = [], 0
    for o, n in rg:
        table.append((o, n, at)); at += n
    return table, at, touches


@pytest.mark.parametrize("full", [True, False])
def test_one_damaged_plane_frame(lib, full):
    """plane frame 6 (group 1, plane 2) of link j fails with 20, for j the first, a middle and the last link: exactly the ranges over group 1 report {20, 6}
    and link j; the others are right, bytes included"""
    vs, chain = _chain(lib, 4, 5, full)
    table, capacity, touches = _damage_table(4)
    for j in (0, 2, 4):
        for limit in (0, 20000):
            rc, d, status, link, _, _, _ = chain.read(table, capacity, limit=limit, damage={j: 6})
            assert rc == 0 and status[:2] == [20, 1] and link[0] == j
            for r, ((o, n, to), t) in enumerate(zip(table, touches)):
                assert status[2 + 2 * r:4 + 2 * r] == ([20, 6] if t else [0, 0]) and link[1 + r] == (j if t else -1), (j, r)
                if not t:
                    assert d[to:to + n].tobytes() == vs[-1][o:o + n].tobytes(), (j, r)
            rc2, d2, status2, link2, _, _, _ = chain.read(table, capacity, limit=limit, damage={j: 6}, want_link=False)      # d_link NULL: the same status
            assert rc2 == 0 and status2 == status and link2 == [-7] * len(link)


def test_two_damaged_links_report_the_earlier(lib):
    """frames under one range damaged in links 3 and 1: link 1 is reported, with ITS frame; a range only link 3's frame lies under reports link 3"""
    vs, chain = _chain(lib, 4, 5, True)
    g = FRAME * 4
    table = [(g + 8, 100, 0), (2 * g + 8, 100, 100), (g - 50, 2 * g + 100, 200), (5, 20, 300 + 2 * g)]
    capacity = 320 + 2 * g
    rc, d, status, link, _, _, _ = chain.read(table, capacity, damage={3: 9, 1: 6}, code=20)      # link 3: group 2, plane 1; link 1: group 1, plane 2
    assert rc == 0 and status == [20, 0, 20, 6, 20, 9, 20, 6, 0, 0] and link == [1, 1, 3, 1, -1]
    assert d[300 + 2 * g:320 + 2 * g].tobytes() == vs[-1][5:25].tobytes()
    rc, d, status, link, _, _, _ = chain.read(table, capacity, damage={3: 6, 1: 6}, code=20)      # the same frame index in both
    assert rc == 0 and status == [20, 0, 20, 6, 0, 0, 20, 6, 0, 0] and link == [1, 1, -1, 1, -1]
    assert d[100:200].tobytes() == vs[-1][2 * g + 8:2 * g + 108].tobytes()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(lib):
    """every refusal of the chain read: UNSUPPORTED, the message names the link, no backend launched anything, and the output, the status and d_link are untouched"""
    k = 4
    vs = cm.versions(k, ELEMENTS, 3, seed=9)
    full = _write_link(lib, vs[0], None, k); d1 = _write_link(lib, vs[1], vs[0], k); d2 = _write_link(lib, vs[2], vs[1], k)
    blob, offs = _frames_of(dm.planes(vs[0], k, FRAME))
    bound = lib.emu_typed_bound(vs[0].size, FRAME, k, 1)
    dl = np.zeros(bound, dtype=np.uint8); status = np.full(2, -1, dtype=np.int32); info = np.zeros(4, dtype=np.uint64); trace = np.zeros(64, dtype=np.uint32); words = np.zeros(1, dtype=np.uint64)
    assert lib.emu_delta_compress(1, 1, vs[0].ctypes.data, vs[0].size, FRAME, k, 1, blob.ctypes.data, offs.ctypes.data, dl.ctypes.data, bound, status.ctypes.data, None, info.ctypes.data,
                                  trace.ctypes.data, 64, words.ctypes.data, None) == 0
    delta = dl[:int(info[0])].copy()
    sizes = np.array([20 + i for i in range(4)], dtype=np.uint64); given = np.zeros(4, dtype=np.int32)
    pl = np.full(4096, 0x5A, dtype=np.uint8)
    plain = pl[:lib.emu_typed_plain(vs[0].ctypes.data, vs[0].size, FRAME * k, 0, sizes.ctypes.data, given.ctypes.data, 0, pl.ctypes.data, pl.size, status.ctypes.data)].copy()
    v2 = cm.versions(2, ELEMENTS * 2, 1, seed=1)                          # the same content size, another element size
    k2 = _write_link(lib, v2[1], v2[0], 2)
    other_group = _write_link(lib, vs[1], vs[0], k, frame=FRAME // 2)
    short = _write_link(lib, vs[1][:-k], vs[0][:-k], k)
    streams = [full, d1, d2, delta, plain, k2, other_group, short]
    FULL, D1, D2, DELTA, PLAIN, K2, GROUP, SHORT = range(8)
    zeros = np.zeros(ELEMENTS * k, dtype=np.uint8)
    chain = Chain(lib, streams, [zeros] * len(streams), vs[0])
    table = [(8, 4000, 0)]
    cases = [
        (dict(pick=[]), b"links"), (dict(pick=[FULL] * 17), b"links"), (dict(pick=[FULL, -1, D2]), b"link 1 is NULL"), (dict(pick=[FULL, D1, D1]), b"link 2"),
        (dict(pick=[FULL, PLAIN]), b"link 1 is a plain"), (dict(pick=[PLAIN], base=None), b"link 0 is a plain"),
        (dict(pick=[FULL, D1, K2]), b"link 2 differs"), (dict(pick=[FULL, GROUP]), b"link 1 differs"), (dict(pick=[FULL, D1, SHORT]), b"link 2 differs"),
        (dict(pick=[DELTA, D1]), b"link 0 has the delta"), (dict(pick=[FULL, D1, DELTA]), b"link 2 is not"), (dict(pick=[D1, FULL]), b"link 1 is not"),
        (dict(pick=[D1, D2], base=None), b"link 0 is an xor-with-base stream"), (dict(pick=[FULL, D1]), b"link 0 is an unfiltered"),
        (dict(pick=[D1, D2], base_size=ELEMENTS * k - k), b"link 0 has another content size"), (dict(pick=[D1, D2], base_size=0), b"content size"),
        (dict(pick=[D1, D2], base="dst"), b"overlaps"),
    ]
    for kw, word in cases:
        kw.setdefault("base", None if kw["pick"] and kw["pick"][0] == FULL and word != b"link 0 is an unfiltered" else "own")
        rc, d, status, link, stats, traces, text = chain.read(table, 4000, **kw)
        assert rc == UNSUPPORTED and word in text and b"chain" in text, (kw, text)
        assert all(t == [] for t in traces) and (d == 0x5A).all() and status == [-1] * 4 and link == [-7] * 2, (kw, text)
    # the ranges' own refusals, as before: beyond the content, a destination beyond the capacity
    for bad_table, cap in (([(8, ELEMENTS * k, 0)], ELEMENTS * k), ([(8, 4000, 1)], 4000)):
        for pick, base in (([FULL, D1], None), ([D1, D2], "own")):
            rc, d, status, link, stats, traces, text = chain.read(bad_table, cap, pick=pick, base=base)
            assert rc != 0 and all(t == [] for t in traces) and (d == 0x5A).all() and status == [-1] * 4 and link == [-7] * 2 and b"range" in text, text
    chain.close()


# ------------------------------------------------------------------------------------------------ the sanitizer program
def test_sanitizer_program(tmp_path):
    """tests/emu/chain_planes_main.cpp under AddressSanitizer and UBSan: the chain join body over the shapes above, every buffer -- every link's planar buffer
    and the base -- a heap allocation sized exactly. A program of its own, run as a subprocess"""
    exe = os.path.join(str(tmp_path), "chain_planes_asan")
    subprocess.check_call(["sh", os.path.join(EMU, "build_asan_planes.sh"), "chain_planes_main.cpp", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert b"cases" in r.stdout


# ------------------------------------------------------------------------------------------------ what the feature is for
@pytest.mark.parametrize("dtype,k", [("bf16", 2), ("fp32", 4)])
def test_predecessor_deltas_are_smaller_with_libzstd_alone(dtype, k):
    """4 groups of 131 072 elements, default_rng(7): w0 = N(0, 1) * 0.02 in fp32, w(i) = w(i-1) + N(0, 1) * 0.02 * 1e-3, every version rounded to the storage
    type. libzstd's level-3 frames of every plane of every group: size(v8 ^ v7) < size(v8 ^ v4) < size(v8 ^ v0) -- the predecessor layout is the small one,
    and it is the one only a chain read serves. (libzstd 1.5.7 gives, as fractions of raw -- bf16: 0.175 < 0.226 < 0.254 against 0.708 for v8's own planes; fp32: 0.588 <
    0.613 < 0.627 against 0.854)"""
    G = 131072
    vs = cm.drifting_versions(dtype, 4 * G, 8, 1e-3, 7)
    ref = reflib.checker()

    def size(data, base):
        planar = pm.split(np.frombuffer(data, dtype=np.uint8), k, G) if base is None else xm.split(data, base, k, G)
        return sum(len(ref.compress(planar[at:at + G].tobytes(), level=3)) for at in range(0, planar.size, G))

    raw = len(vs[8])
    own, d7, d4, d0 = size(vs[8], None), size(vs[8], vs[7]), size(vs[8], vs[4]), size(vs[8], vs[0])
    print("%s: planes of v8 %.3f, v8 ^ v7 %.3f, v8 ^ v4 %.3f, v8 ^ v0 %.3f of raw" % (dtype, own / raw, d7 / raw, d4 / raw, d0 / raw))
    assert d7 < d4 < d0
