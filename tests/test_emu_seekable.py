"""The seekable-stream kernels (python-zstandard_amd/csrc/zhip_seekable.hpp) on the host wave emulator: the multi-workgroup scan against numpy.cumsum, the
table writer against a table written here from the layout, the open call's checks against single changes to a good stream, the range pieces with the decoder
replaced by a copy -- and zhip_seekable_bound against the sizes libzstd gives the streams of the GPU suite."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import seekable_cases as sc


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return sc.emu(tmp_path_factory.mktemp("emu_seekable"))


def _tiles(lib):
    t = np.zeros(3, dtype=np.uint32)
    lib.emu_seekable_tiles(t.ctypes.data)
    return [int(x) for x in t]


def _scan_sizes():
    # the tile sizes are the kernel's own: asked of the build under test when the cases are collected would need the build, so the constants are
    # asserted equal to these in test_scan_tiles
    lanes, tile, grid_pass = 64, 256, 1024 * 256
    ns = [0, 1, 2, 63, 64, 65]
    for t in (lanes, tile, grid_pass):
        ns += [t - 1, t, t + 1]
    return sorted(set(ns + [70001]))


def test_scan_tiles(lib):
    assert _tiles(lib) == [64, 256, 1024 * 256], "the scan's tile sizes changed: _scan_sizes has to follow them"


@pytest.mark.parametrize("n", _scan_sizes())
def test_scan_matches_cumsum(lib, n):
    rng = np.random.default_rng(1000 + n)
    sizes = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    if n:
        sizes[rng.integers(0, n, size=max(1, n // 7))] = 0
        sizes[rng.integers(0, n, size=max(1, n // 7))] = (1 << 32) - 1
    for failing in ([], [n // 2] if n else [], [n - 1, n // 3] if n > 2 else []):
        status = np.zeros(max(n, 1), dtype=np.int32)
        for i in failing:
            status[i] = 40
        offs = np.full(n + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        bad = lib.emu_seekable_scan(sizes.ctypes.data if n else None, status.ctypes.data, n, offs.ctypes.data)
        counted = np.where(status[:n] != 0, np.uint64(0), sizes)
        want = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(counted, dtype=np.uint64)])
        assert np.array_equal(offs, want), "n = %d, failing %r" % (n, failing)
        assert bad == (min(failing) if failing else (1 << 64) - 1)


def _run_table(lib, src, frame_size, checksum, out_sizes, status, capacity):
    n = len(out_sizes)
    s = np.frombuffer(src, dtype=np.uint8).copy() if src else np.zeros(1, dtype=np.uint8)
    sizes = np.array(out_sizes, dtype=np.uint64) if n else np.zeros(1, dtype=np.uint64)
    st = np.array(status, dtype=np.int32) if n else np.zeros(1, dtype=np.int32)
    dst = np.full(capacity + 64, 0xCD, dtype=np.uint8)
    ssegs = np.zeros((max(n, 1), 2), dtype=np.uint64); dsegs = np.zeros((max(n, 1), 2), dtype=np.uint64)
    out = np.full(2, -1, dtype=np.int32)
    size = lib.emu_seekable_table(s.ctypes.data, len(src), frame_size, int(checksum), sizes.ctypes.data, st.ctypes.data, dst.ctypes.data, capacity,
                                  ssegs.ctypes.data, dsegs.ctypes.data, out.ctypes.data)
    return int(size), out.tolist(), dst, ssegs[:n], dsegs[:n], st[:n]


@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("n", [0, 1, 65])
def test_table_writer(lib, n, checksum):
    frame_size = 1000
    src = sc.source((n - 1) * frame_size + 137) if n else b""
    parts = sc.chunks(src, frame_size)
    assert len(parts) == n
    rng = np.random.default_rng(7 + n)
    out_sizes = [int(x) for x in rng.integers(9, 1200, size=n)]
    want = sc.table([(c, len(p), sc.xxh64(p) & 0xFFFFFFFF) for c, p in zip(out_sizes, parts)], checksum)
    total = sum(out_sizes)
    size, status, dst, ssegs, dsegs, st = _run_table(lib, src, frame_size, checksum, out_sizes, [0] * n, total + len(want))
    assert status == [0, 0] and size == total + len(want)
    assert dst[total:size].tobytes() == want
    assert (dst[:total] == 0xCD).all() and (dst[size:] == 0xCD).all(), "only the table is this kernel's to write"
    bound = lambda v: v + (v >> 8) + (((128 << 10) - v) >> 11 if v < (128 << 10) else 0)
    for i, p in enumerate(parts):
        assert tuple(ssegs[i]) == (i * frame_size, len(p))
        assert dsegs[i][1] == bound(len(p)) and dsegs[i][0] >= (dsegs[i - 1][0] + dsegs[i - 1][1] if i else 0)
    # one byte short: status 70, size 0, nothing written, and every frame's status set so that the compaction copies nothing
    size, status, dst, _, _, st = _run_table(lib, src, frame_size, checksum, out_sizes, [0] * n, total + len(want) - 1)
    assert size == 0 and status[0] == 70 and (dst == 0xCD).all() and (st != 0).all()
    if n == 65:
        # a frame the encoder refused: its code and index, whatever its size cell holds
        size, status, dst, _, _, st = _run_table(lib, src, frame_size, checksum, out_sizes, [0] * 40 + [40] + [0] * 23 + [70], total + len(want))
        assert size == 0 and status == [40, 40] and (dst == 0xCD).all() and (st != 0).all()
        # the capacity cuts frame 3: that is the index
        size, status, dst, _, _, st = _run_table(lib, src, frame_size, checksum, out_sizes, [0] * n, sum(out_sizes[:4]) - 1)
        assert size == 0 and status == [70, 3] and (dst == 0xCD).all()


def test_xxh64_agrees(lib):
    for n in (0, 1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 1000, 4096):
        p = sc.source(n)
        b = np.frombuffer(p, dtype=np.uint8).copy() if n else np.zeros(1, dtype=np.uint8)
        assert lib.emu_seekable_xxh64(b.ctypes.data, n) == sc.xxh64(p), n


def _good5(checksum):
    rng = np.random.default_rng(5)
    contents = [sc.source(20497)[i * 4096:(i + 1) * 4096] for i in range(6)][:5]
    frames = [bytes(rng.integers(0, 256, size=k, dtype=np.uint8)) for k in (100, 37, 4000, 1, 513)]      # the validator does not look into frames
    return sc.stream_of(frames, contents, checksum), contents


@pytest.mark.parametrize("checksum", [False, True])
def test_validator(lib, checksum):
    good, contents = _good5(checksum)
    code, info = sc.emu_validate(lib, good)
    assert code == 0 and info == [5, 12 if checksum else 8, int(checksum), 100 + 37 + 4000 + 1 + 513, sum(len(c) for c in contents)]
    for name, stream, want in sc.validator_damage(good, 5, checksum):
        code, _ = sc.emu_validate(lib, stream)
        assert code == want, name
    for bits in (1, 2, 3):                                        # the unused bits are ignored
        b = bytearray(good); b[len(b) - 5] |= bits
        assert sc.emu_validate(lib, bytes(b))[0] == 0
    e = 12 if checksum else 8
    at = len(good) - (8 + 5 * e + 9)
    b = bytearray(good); struct.pack_into("<I", b, at + 8 + 3 * e + 4, sc.MAX_CONTENT)        # exactly 2^30 is allowed
    assert sc.emu_validate(lib, bytes(b))[0] == 0
    assert sc.emu_validate(lib, sc.table([], checksum))[0] == 0, "the stream of zero frames"
    for k in range(17):
        assert sc.emu_validate(lib, good[:k])[0] in (10, 20), "shorter than a table"


def test_accepted_tables_stay_inside_the_stream(lib):
    """whatever the entries say, a stream the checks accept yields no offset outside it: random tables, some consistent, most not"""
    rng = np.random.default_rng(99)
    accepted = 0
    for trial in range(300):
        n = int(rng.integers(0, 40))
        csz = [int(x) for x in rng.integers(0, 300, size=n)]
        dsz = [int(x) for x in rng.integers(0, 3, size=n) * rng.integers(0, 5000, size=n)]
        ck = bool(trial & 1)
        body = bytes(rng.integers(0, 256, size=sum(csz), dtype=np.uint8))
        if trial % 3 == 0 and n:
            csz[int(rng.integers(0, n))] += int(rng.integers(1, 1 << 31))          # a size that points far outside
        if trial % 5 == 0 and n:
            csz[int(rng.integers(0, n))] = 0xFFFFFFFF
        stream = body + sc.table([(c, d, 0) for c, d in zip(csz, dsz)], ck)
        buf = np.frombuffer(stream, dtype=np.uint8).copy()
        info = np.zeros(5, dtype=np.uint64)
        c_off = np.zeros(n + 1, dtype=np.uint64); d_off = np.zeros(n + 1, dtype=np.uint64); place = np.zeros(n + 1, dtype=np.uint64)
        code = lib.emu_seekable_validate(buf.ctypes.data, len(stream), info.ctypes.data, c_off.ctypes.data, d_off.ctypes.data, place.ctypes.data)
        if code:
            assert code == 20
            continue
        accepted += 1
        assert int(c_off[n]) == int(info[3]) <= len(stream) and (np.diff(c_off.astype(np.int64)) >= 0).all()
        assert [int(x) for x in np.diff(c_off.astype(np.int64))] == csz and [int(x) for x in np.diff(d_off.astype(np.int64))] == dsz
        assert [int(x) for x in np.diff(place.astype(np.int64))] == [int(d != 0) for d in dsz]
    assert 50 < accepted < 250


def _range(lib, stream, content, offset, length, short_frame=-1):
    buf = np.frombuffer(stream, dtype=np.uint8).copy()
    c = np.frombuffer(content, dtype=np.uint8).copy()
    dst = np.full(64 + length + 64, 0x5A, dtype=np.uint8)
    out = np.full(2, -1, dtype=np.int32)
    segs = np.zeros((64, 4), dtype=np.uint64); cnt = C.c_uint32(0)
    rc = lib.emu_seekable_range(buf.ctypes.data, len(stream), c.ctypes.data, offset, length, dst[64:].ctypes.data, short_frame, out.ctypes.data, segs.ctypes.data, C.byref(cnt))
    assert (dst[:64] == 0x5A).all() and (dst[64 + length:] == 0x5A).all(), "bytes outside [0, length) are untouched"
    return rc, out.tolist(), dst[64:64 + length].tobytes(), segs[:cnt.value]


@pytest.mark.parametrize("checksum", [False, True])
def test_range_pieces(lib, checksum):
    total, fs = sc.RANGE_CASE
    content = sc.source(total)
    parts = sc.chunks(content, fs)
    rng = np.random.default_rng(3)
    frames = [bytes(rng.integers(0, 256, size=int(k), dtype=np.uint8)) for k in rng.integers(20, 900, size=len(parts))]
    # a skippable frame and an empty frame listed with Decompressed_Size 0: never the decoder's
    stream = sc.stream_of(frames, parts, checksum, extra_entries=[(2, b"\x50\x2a\x4d\x18\x03\x00\x00\x00abc"), (0, b"\x28\xb5\x2f\xfd\x20\x00\x01\x00\x00")])
    for off, ln in sc.ranges_of(total) + [(4096, 8192), (100, 20000), (3 * 4096, 4096 + 17)]:
        rc, status, got, segs = _range(lib, stream, content, off, ln)
        assert rc == 0 and status == [0, 0], (off, ln)
        assert got == content[off:off + ln], (off, ln)
        assert all(int(s[3]) > 0 for s in segs)
        if ln:
            inside = [int(s[2]) for s in segs if int(s[2]) < (1 << 63)]
            assert len(segs) == (off + ln - 1) // fs - off // fs + 1 and len(segs) - len(inside) <= 2
            assert len(inside) == sum(1 for k in range(len(parts)) if off <= k * fs and k * fs + len(parts[k]) <= off + ln)
    for off, ln in ((total, 1), (0, total + 1), (total + 1, 0), ((1 << 64) - 1, 2)):
        assert _range(lib, stream, content, off, ln)[0] == sc.SIZE_MISMATCH
    # a frame that comes out short: 20 and its index in the TABLE (two entries of no content lie in front of frame 3's)
    rc, status, _, _ = _range(lib, stream, content, 4096, 3 * 4096, short_frame=5)
    assert rc == 0 and status == [20, 5]
    rc, status, _, _ = _range(lib, stream, content, 0, 4096, short_frame=5)
    assert rc == 0 and status == [0, 0]
    if checksum:
        wrong = bytearray(content); wrong[2 * 4096 + 5] ^= 1; wrong[4 * 4096 + 1] ^= 0x80        # what frames 2 and 4 "decode" to differs from what the entries were made of
        rc, status, _, _ = _range(lib, stream, bytes(wrong), 0, total)
        assert rc == 0 and status == [22, 4], "the lowest failing frame: content frame 2 is entry 4"
        rc, status, got, _ = _range(lib, stream, bytes(wrong), 0, 2 * 4096)
        assert rc == 0 and status == [0, 0] and got == content[:2 * 4096]


def test_bound_covers_libzstd(lib, ref):
    from tests import reflib
    import zstandard_amd as zstd
    L = zstd._lib.lib()
    assert L.zhip_seekable_bound(10, 0, 0) == 0 and L.zhip_seekable_bound(10, (1 << 30) + 1, 0) == 0 and L.zhip_seekable_bound(1 << 28, 1, 0) == 0
    assert L.zhip_seekable_bound(10, 4, 2) == 0, "unknown flag"
    assert L.zhip_seekable_bound((1 << 27), 1, 1) > 0 and L.zhip_seekable_bound(0, 4096, 0) == 17
    for src_size, fs in sc.CASES:
        data = sc.source(src_size)
        parts = sc.chunks(data, fs)
        assert L.zhip_seekable_frame_count(src_size, fs) == len(parts)
        levels = (3, 1, 5) if (src_size, fs) == sc.CASES[-1] else (3, 1)
        for level in levels:
            for flags in (reflib.DEFAULT_FLAGS, reflib.DEFAULT_FLAGS | reflib.F_CHECKSUM):
                frames = sum(len(ref.compress(p, level, flags)) for p in parts)
                for ck in (0, 1):
                    actual = frames + 8 + len(parts) * (12 if ck else 8) + 9
                    assert L.zhip_seekable_bound(src_size, fs, ck) >= actual, (src_size, fs, level, flags, ck)
                    assert lib.emu_seekable_bound(src_size, fs, ck) == L.zhip_seekable_bound(src_size, fs, ck)
