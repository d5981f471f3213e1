"""One frame per record and reads by frame index (zhip_seekable_compress_records_device, zhip_seekable_frame_offsets, zhip_seekable_decompress_frames_device)
without a GPU: the scan's two record modes against numpy.cumsum, the segment writer's slots against the host's reservation, the pre-check's failures, the table
writer against a table written here from the layout, zhip_seekable_records_bound against libzstd's frames, the index -> range mapping against a Python model
through the library's own plan and gather kernels -- on the host wave emulator, and the same as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import subprocess

import numpy as np
import pytest

from tests import seekable_cases as sc
from tests import seekable_range_cases as rc_
from tests import seekable_record_cases as rec


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return rec.emu(tmp_path_factory.mktemp("emu_seekable_records"))


# ---------------------------------------------------------------------------------------------------- 1. both scan modes
TILE, GRID_PASS = 256, 1024 * 256


def test_scan_tiles(lib):
    t = np.zeros(3, dtype=np.uint32)
    lib.emu_seekable_tiles(t.ctypes.data)
    assert [int(x) for x in t] == [64, TILE, GRID_PASS], "the scan's tile sizes changed: the sizes below have to follow them"


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, GRID_PASS - 1, GRID_PASS, GRID_PASS + 1])
def test_scan_modes_match_cumsum(lib, n):
    rng = np.random.default_rng(3000 + n)
    lengths = rng.integers(0, 5000, size=n, dtype=np.uint64)
    if n:
        lengths[rng.integers(0, n, size=max(1, n // 9))] = 0
        lengths[rng.integers(0, n, size=max(1, n // 50))] = rng.choice(np.array(rec.EDGE_LENGTHS, dtype=np.uint64), size=max(1, n // 50))
    limit = 400000
    offsets = rng.integers(0, 1 << 20, size=n, dtype=np.uint64)
    src_size = (1 << 20) + limit
    records = np.stack([offsets, lengths], axis=1) if n else np.zeros((0, 2), dtype=np.uint64)
    strides = ((lengths + (lengths >> np.uint64(8)) + np.where(lengths < 131072, (np.uint64(131072) - np.minimum(lengths, np.uint64(131072))) >> np.uint64(11), np.uint64(0))
                + np.uint64(15)) & ~np.uint64(15))
    zero = np.zeros(1, dtype=np.uint64)
    a = np.ascontiguousarray(records) if n else np.zeros((1, 2), dtype=np.uint64)
    for mode, counted in ((3, lengths), (4, strides)):
        offs = np.full(n + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        bad = lib.emu_records_scan(a.ctypes.data, n, mode, limit, src_size, offs.ctypes.data)
        assert np.array_equal(offs, np.concatenate([zero, np.cumsum(counted, dtype=np.uint64)])), "mode %d, n = %d" % (mode, n)
        assert bad == rec.NONE
    if n >= 255:
        # the scalar model agrees with numpy where both are cheap
        small = [(int(o), int(l)) for o, l in records[:300]]
        assert np.array_equal(rec.scan_model(small, 4)[0][1:], np.cumsum(strides[:300], dtype=np.uint64))
    # the lowest bad record: first, last, on a tile's edge, on a span's edge -- each kind of bad, alone and with a later one
    # (where spans are several tiles the emulator takes seconds per scan: the first record of the second workgroup's span, and the last record)
    spots = [2 * TILE if n > GRID_PASS else TILE, n - 1] if n >= GRID_PASS - 1 else sorted(set(i for i in (0, n - 1, TILE - 1, TILE, n // 2) if 0 <= i < n))
    kinds = [lambda o, l: (o, limit + 1), lambda o, l: (src_size - l + 1, l) if l else (src_size + 1, 0), lambda o, l: (rec.NONE - 3, max(l, 4))]
    for k, i in enumerate(spots):
        for later in ((n - 1,) if n >= GRID_PASS - 1 else (None, n - 1)):
            damaged = a.copy()
            damaged[i] = kinds[k % 3](int(a[i][0]), int(a[i][1]))
            if later is not None and later > i:
                damaged[later] = (0, limit + 7)
            offs = np.full(n + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
            bad = lib.emu_records_scan(damaged.ctypes.data, n, 3, limit, src_size, offs.ctypes.data)
            assert bad == i, (n, i, k, later)
            assert np.array_equal(offs, np.concatenate([zero, np.cumsum(damaged[:n, 1], dtype=np.uint64)])), "a bad record still counts its length: the verdict never reads the sums then"
            if n <= 300:
                assert rec.scan_model([(int(o), int(l)) for o, l in damaged[:n]], 3, limit, src_size)[1] == i


# ---------------------------------------------------------------------------------------------------- 2. the segment writer
def _edge_records(seed, extra=40, share=6):
    rng = np.random.default_rng(seed)
    lengths = rec.EDGE_LENGTHS + [int(x) for x in rng.integers(0, 9000, size=extra)] + rec.EDGE_LENGTHS[:4]
    order = rng.permutation(len(lengths))
    lengths = [lengths[i] for i in order]
    records, src_size = rec.layout(lengths, rng, shuffle=True, share=share)
    return lengths, records, src_size


@pytest.mark.parametrize("seed", [1, 2])
def test_segment_writer(lib, seed):
    lengths, records, src_size = _edge_records(seed)
    n, total, longest = len(records), sum(lengths), max(lengths)
    assert len(set(o for o, _ in records)) < n, "at least two records share bytes"
    src = sc.source(src_size)
    for max_content in (total, total + 12345):
        got = rec.run_compress(lib, src, records, max_content, longest, False, sizes=[1] * n)
        assert got["status"] == [0, 0] and got["pre"] == 1 and got["refused"] is None
        assert got["slot_bytes"] == rec.slot_bytes(max_content, n)
        assert got["src_segs"] == records
        spans = []
        for i, (at, cap) in enumerate(got["slot_segs"]):
            assert at % 16 == 0, "slot %d is not 16-aligned" % i
            assert cap >= rec.compress_bound(lengths[i]), "slot %d is shorter than zhip_compress_bound" % i
            assert at + cap <= got["slot_bytes"], "slot %d leaves the reserved area" % i
            spans.append((at, at + max(cap, 1)))
        spans.sort()
        assert all(b0 <= a1 for (_, b0), (a1, _) in zip(spans, spans[1:])), "slots overlap"
    # a generous maxContentBytes does not size the slots beyond n records of maxRecordBytes
    got = rec.run_compress(lib, src, records, 1 << 50, longest, False, sizes=[1] * n)
    assert got["status"] == [0, 0] and got["slot_bytes"] == rec.slot_bytes(n * longest, n)


def test_slot_reservation_is_enough():
    """the derivation next to zsk_records_slot_bytes, checked where it is tight: every length's stride against len + (len >> 8) + 79"""
    for l in list(range(0, 70000)) + list(range(131072 - 3000, 131072 + 3000)) + [400000, (1 << 30) - 1, 1 << 30]:
        assert rec.slot_stride(l) <= l + (l >> 8) + 79
        assert rec.slot_stride(l) >= rec.compress_bound(l)
    assert rec.compress_bound(0) == 64, "the harmless form's slots are zhip_compress_bound(0)"


# ---------------------------------------------------------------------------------------------------- 3. pre-check failures
@pytest.mark.parametrize("case", rec.precheck_failures(), ids=[c[0] for c in rec.precheck_failures()])
def test_precheck_failures(lib, case):
    name, records, src_size, max_content, max_record, want = case
    n = len(records)
    src = sc.source(src_size)
    for checksum in (False, True):
        got = rec.run_compress(lib, src, records, max_content, max_record, checksum, sizes=[9] * n, capacity=n * 9 + rec.table_size(n, checksum))
        assert got["status"] == want and got["pre"] == 0, name
        assert got["size"] == 0 and (got["dst"] == rec.GUARD_BYTE).all() and got["copied"] == 0, "a failed pre-check writes nothing (%s)" % name
        assert got["refused"] is None, "the batch was handed a segment outside its buffer (%s)" % name
        assert all(s == (0, 0) for s in got["src_segs"]), "the segments handed on are empty"
        assert got["slot_segs"] == [(64 * i, 64) for i in range(n)] and 64 * n <= got["slot_bytes"]


def test_precheck_passes_at_the_bounds(lib):
    """exactly maxRecordBytes, exactly srcSize, exactly maxContentBytes: all allowed"""
    records = [(0, 100), (100, 3000), (3100 - 50, 50), (3100, 0)]
    got = rec.run_compress(lib, sc.source(3100), records, 3150, 3000, True, sizes=[20, 30, 40, 9])
    assert got["status"] == [0, 0] and got["pre"] == 1 and got["size"] == 99 + rec.table_size(4, True)


# ---------------------------------------------------------------------------------------------------- 4. the table writer
@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("n", [0, 1, 65])
def test_table_writer(lib, n, checksum):
    rng = np.random.default_rng(70 + n)
    lengths = [int(x) for x in rng.integers(1, 2500, size=n)]
    for i in range(0, n, 7):
        lengths[i] = 0                                                      # empty records among them
    records, src_size = rec.layout(lengths, rng, shuffle=True, share=3 if n > 3 else 0)
    src = sc.source(max(src_size, 1))[:src_size]
    out_sizes = [min(int(x), rec.compress_bound(l)) for x, l in zip(rng.integers(9, 1200, size=n), lengths)]      # (no frame is larger than its slot)
    want = sc.table([(c, l, sc.xxh64(src[o:o + l]) & 0xFFFFFFFF) for c, (o, l) in zip(out_sizes, records)], checksum)
    if n and checksum:
        assert want[8 + 8:8 + 12] == (sc.xxh64(b"") & 0xFFFFFFFF).to_bytes(4, "little"), "the checksum of an empty record is XXH64's of b''"
    total = sum(out_sizes)
    got = rec.run_compress(lib, src, records, sum(lengths), max(lengths + [0]), checksum, sizes=out_sizes)
    assert got["status"] == [0, 0] and got["size"] == total + len(want)
    assert got["dst"][total:].tobytes() == want
    assert got["dst"][:total].tobytes() == b"".join(rec.stand_in_frame(i, c) for i, c in enumerate(out_sizes)), "frames back to back in index order"
    # one byte short: 70, size 0, nothing written
    got = rec.run_compress(lib, src, records, sum(lengths), max(lengths + [0]), checksum, sizes=out_sizes, capacity=total + len(want) - 1)
    assert got["size"] == 0 and got["status"][0] == 70 and (got["dst"] == rec.GUARD_BYTE).all() and got["copied"] == 0
    if n == 65:
        assert got["status"] == [70, 64], "only the table does not fit: the last frame"
        got = rec.run_compress(lib, src, records, sum(lengths), max(lengths), checksum, sizes=out_sizes, status=[0] * 40 + [40] + [0] * 23 + [70])
        assert got["size"] == 0 and got["status"] == [40, 40] and (got["dst"] == rec.GUARD_BYTE).all() and got["copied"] == 0
        got = rec.run_compress(lib, src, records, sum(lengths), max(lengths), checksum, sizes=out_sizes, capacity=sum(out_sizes[:3]) - 1)
        assert got["size"] == 0 and got["status"] == [70, 2] and (got["dst"] == rec.GUARD_BYTE).all()


# ---------------------------------------------------------------------------------------------------- 5. the bound
def test_records_bound_arguments(lib):
    import zstandard_amd as zstd
    L = zstd._lib.lib()
    assert L.zhip_seekable_records_bound(0, 0, 0) == 17 and L.zhip_seekable_records_bound(0, 0, 1) == 17
    assert L.zhip_seekable_records_bound(1000, (1 << 27) + 1, 0) == 0, "more than 2^27 records"
    assert L.zhip_seekable_records_bound(1000, 1 << 27, 1) > 0
    assert L.zhip_seekable_records_bound(1000, 3, 2) == 0, "unknown flag"
    assert L.zhip_seekable_records_bound((1 << 57) + 1, 3, 0) == 0
    for content, n in ((0, 5), (1000, 3), (1 << 20, 300), (1 << 40, 1 << 20)):
        for ck in (0, 1):
            assert L.zhip_seekable_records_bound(content, n, ck) == lib.emu_records_bound(content, n, ck) == content + (content >> 8) + 64 * n + rec.table_size(n, ck)


@pytest.mark.parametrize("level", [1, 3, -5])
def test_records_bound_covers_libzstd(level):
    from tests import reflib
    if not reflib.have_ref():
        pytest.skip("no libzstd 1.5.7 available")
    import zstandard_amd as zstd
    ref = reflib.RefZstd()
    L = zstd._lib.lib()
    for seed in (1, 2):
        lengths, records, src_size = _edge_records(seed)
        src = sc.source(src_size)
        for flags in (reflib.DEFAULT_FLAGS, reflib.DEFAULT_FLAGS | reflib.F_CHECKSUM):
            frames = sum(len(ref.compress(src[o:o + l], level, flags)) for o, l in records)
            for ck in (0, 1):
                assert L.zhip_seekable_records_bound(sum(lengths), len(records), ck) >= frames + rec.table_size(len(records), ck), (seed, level, flags, ck)


# ---------------------------------------------------------------------------------------------------- 6. frame offsets and reads by index
def _stream(lib, n, seed, checksum):
    rng = np.random.default_rng(9000 + seed)
    sizes = rc_.random_sizes(rng, n)
    if n > 2:
        sizes[1] = 0
    content = bytes(rng.integers(0, 256, size=sum(sizes), dtype=np.uint8))
    return sizes, content, rc_.stream_for(lib, sizes, content, checksum, rng), rng


@pytest.mark.parametrize("n", [0, 1, 7, 130])
def test_frame_offsets(lib, n):
    sizes, content, stream, rng = _stream(lib, n, n, False)
    d = [0]
    for s in sizes:
        d.append(d[-1] + s)
    for first, count in [(0, n), (0, 0), (n, 0), (n // 2, n - n // 2), (n // 3, 1 if n else 0)]:
        rc, got = rec.frame_offsets(lib, stream, first, count)
        assert rc == 0 and got == d[first:first + count + 1], (first, count)
    for first, count in [(0, n + 1), (n + 1, 0), (n, 1), (1, n), ((1 << 32) - 1, 2)]:
        if first + count > n:
            assert rec.frame_offsets(lib, stream, first, count)[0] == sc.SIZE_MISMATCH, (first, count)


@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("n", [1, 7, 130])
def test_reads_by_index(lib, n, checksum):
    sizes, content, stream, rng = _stream(lib, n, 50 + n, checksum)
    d = [0]
    for s in sizes:
        d.append(d[-1] + s)
    for frames in rec.index_lists(rng, n):
        for limit in (0, 4096):
            rc, status, dst, stats, rg = rec.frames_run(lib, stream, content, frames, capacity=sum(sizes[f] for f in frames) + 16, limit=limit)
            assert rc == 0 and status == [0] * (2 + 2 * len(frames)), frames
            at = 0
            for k, f in enumerate(frames):                                   # order kept, back to back
                assert rg[k] == (d[f], sizes[f], at), (k, f)
                assert dst[at:at + sizes[f]].tobytes() == content[d[f]:d[f + 1]]
                at += sizes[f]
            assert (dst[at:] == rec.GUARD_BYTE).all()
            named = [f for f in frames if sizes[f]]
            once = [f for f in set(named) if named.count(f) == 1]
            assert stats[0] == len(set(named)), "every distinct frame with content is one item; an empty frame is none"
            assert stats[1] == len(once), "a frame named once decodes in place, a repeated one through the scratch"
            if len(set(frames)) == len(frames):
                assert stats[1] == stats[0]
    # destinations of the caller's: reversed order with gaps
    frames = list(range(n))
    offs, at = [0] * n, 5
    for f in reversed(frames):
        offs[f] = at; at += sizes[f] + 3
    rc, status, dst, stats, rg = rec.frames_run(lib, stream, content, frames, dst_offsets=offs, capacity=at)
    assert rc == 0 and status == [0] * (2 + 2 * n)
    mask = np.ones(at, dtype=bool)
    for f in frames:
        assert dst[offs[f]:offs[f] + sizes[f]].tobytes() == content[d[f]:d[f + 1]]
        mask[offs[f]:offs[f] + sizes[f]] = False
    assert (dst[mask] == rec.GUARD_BYTE).all()
    # an index equal to nFrames: refused with its position, nothing written
    for frames, pos in (([n], 0), ([0, n], 1), (list(range(n)) + [n + 5], n)):
        rc, status, dst, stats, _ = rec.frames_run(lib, stream, content, frames)
        assert rc == sc.SIZE_MISMATCH and stats[7] == pos and (dst == rec.GUARD_BYTE).all() and status == [-1] * (2 + 2 * len(frames))
    # overlapping destinations are the many-ranges call's refusal
    if n >= 7 and sizes[0] and sizes[2]:
        rc, _, dst, stats, _ = rec.frames_run(lib, stream, content, [0, 2], dst_offsets=[0, sizes[0] - 1], capacity=sizes[0] + sizes[2])
        assert rc == sc.UNSUPPORTED and stats[7] == 1 and (dst == rec.GUARD_BYTE).all()


# ---------------------------------------------------------------------------------------------------- 7. the sanitizer run
def test_sanitizer_run(lib, tmp_path):
    """tests 2 to 4 and 6 as a stand-alone program built with -fsanitize=address,undefined, in a child process: every buffer has exactly the size the call is given"""
    prog = rec.sanitizer_program(tmp_path)
    path = os.path.join(str(tmp_path), "cases.bin")
    cases = 0
    with open(path, "wb") as f:
        lengths, records, src_size = _edge_records(1, extra=20)
        n = len(records)
        src = sc.source(src_size)
        rng = np.random.default_rng(4)
        sizes = [min(int(x), rec.compress_bound(l)) for x, l in zip(rng.integers(9, 300, size=n), lengths)]
        for checksum in (False, True):
            cap = sum(sizes) + rec.table_size(n, checksum)
            rec.write_compress_case(f, src, records, sum(lengths), max(lengths), checksum, sizes, cap, [0, 0]); cases += 1
            rec.write_compress_case(f, src, records, sum(lengths), max(lengths), checksum, sizes, cap - 1, [70, n - 1]); cases += 1
            rec.write_compress_case(f, b"", [], 0, 0, checksum, [], rec.table_size(0, checksum), [0, 0]); cases += 1
        for name, records, src_size, max_content, max_record, want in rec.precheck_failures():
            n = len(records)
            rec.write_compress_case(f, sc.source(src_size), records, max_content, max_record, True, [9] * n, 9 * n + rec.table_size(n, True), want); cases += 1
        for n in (1, 7, 130):
            sizes, content, stream, rng = _stream(lib, n, 50 + n, True)
            for frames in rec.index_lists(rng, n):
                for limit in (0, 4096):
                    rec.write_frames_case(f, stream, content, frames, limit); cases += 1
    done = subprocess.run([prog, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode(errors="replace")[-4000:]
    assert done.stdout.decode().strip().endswith("%d cases" % cases)
