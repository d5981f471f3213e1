"""Many ranges of a seekable stream in one decode batch on the GPU (zhip_seekable_decompress_ranges_device, SeekableStream.read_ranges): every byte of every
range against a Python slice of the source, guards between and around the destinations, the per-range and overall status pairs against the single-range call's,
the counts of the plan (items, inPlace, copyJobs, passes), rejected calls, stream order with recycled table slots, dictionaries and the Python layer.
Streams that reach the GPU damaged pass the host emulator's run of the open call's checks first, as in tests/test_gpu_seekable.py."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from tests import seekable_cases as sc
from tests import test_gpu_seekable as base

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = base.GUARD, base.GUARD_BYTE
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def zstd():
    import torch
    import zstandard_amd as z
    import zstandard_amd.device  # noqa: F401
    assert torch.cuda.is_available()
    return z


@pytest.fixture(scope="module")
def contexts(zstd):
    made = {}

    def get(level=3, write_checksum=False, dict_data=None):
        key = (level, write_checksum, dict_data)
        if key not in made:
            made[key] = zstd.device.DeviceBatchContext(level=level, write_checksum=write_checksum, dict_data=dict_data)
        return made[key]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return sc.emu(tmp_path_factory.mktemp("emu_seekable_ranges_gpu"))


@pytest.fixture(scope="module")
def s1(contexts):
    """S1: the 6-frame stream, without and with table checksums -> (content, {checksum: stream bytes})"""
    src_size, fs = sc.RANGE_CASE
    data = sc.source(src_size)
    out = {}
    for checksum in (False, True):
        stream, st, _ = base._compress(contexts(3, checksum), base._dev(data), fs, checksum)
        assert st == [0, 0]
        out[checksum] = stream
    return data, out


class Opened:
    """a stream on the device and its handle"""

    def __init__(self, ctx, stream_bytes):
        self.ctx, self.tensor = ctx, base._dev(stream_bytes)
        rc, _, self.h, self.info = base._open(ctx, self.tensor)
        assert rc == 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.L.zhip_seekable_close(self.h)


def _table(ranges):
    from zstandard_amd import _lib
    arr = (_lib.SeekableRange * max(len(ranges), 1))()
    for k, (o, l, d) in enumerate(ranges):
        arr[k].offset, arr[k].length, arr[k].dstOffset = o, l, d
    return arr


def _queue(ctx, h, ranges, buf, cap, status, stream):
    """the C call alone -> (rc, stats)"""
    from zstandard_amd import _lib
    stats = _lib.SeekableGatherStats()
    rc = ctx.L.zhip_seekable_decompress_ranges_device(ctx.ctx, h, _table(ranges), len(ranges), buf.data_ptr() + GUARD, cap, status.data_ptr(), C.byref(stats), stream.cuda_stream)
    return rc, {k: int(getattr(stats, k)) for k, _ in stats._fields_}


def _gather(ctx, h, ranges, cap):
    """ranges [(offset, length, dstOffset)] into a buffer of cap bytes with guards on both sides -> (rc, status [2 + 2R], the cap bytes, stats);
    asserts that nothing outside the ranges' destinations was written"""
    import torch
    buf = torch.full((GUARD + cap + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    status = torch.full((2 + 2 * len(ranges),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    rc, stats = _queue(ctx, h, ranges, buf, cap, status, s)
    s.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == GUARD_BYTE).all() and (host[GUARD + cap:] == GUARD_BYTE).all(), "bytes outside [d_dst, d_dst + dstCapacity) were written"
    body = host[GUARD:GUARD + cap]
    if rc == 0:
        assert (body[_untouched(ranges, cap)] == GUARD_BYTE).all(), "bytes of d_dst outside the ranges' destinations were written"
    return rc, status.cpu().tolist(), body, stats


def _untouched(ranges, cap):
    m = np.ones(cap, dtype=bool)
    for _, l, d in ranges:
        m[d:d + l] = False
    return m


def _place(ranges, rng=None, gap=64, reverse=False):
    """(offset, length) -> [(offset, length, dstOffset)], capacity: back to back with `gap` bytes between, in call order, reversed, or in rng's order"""
    order = list(range(len(ranges)))
    if reverse:
        order.reverse()
    if rng is not None:
        order = [int(x) for x in rng.permutation(len(ranges))]
    at, dst = gap, [0] * len(ranges)
    for r in order:
        dst[r] = at
        at += ranges[r][1] + (gap if rng is None else int(rng.integers(0, gap + 1)))
    return [(o, l, d) for (o, l), d in zip(ranges, dst)], at


def _check_bytes(body, ranges, data, only=None):
    for r, (o, l, d) in enumerate(ranges):
        if only is None or only[r]:
            assert body[d:d + l].tobytes() == data[o:o + l], (r, o, l)


# ---------------------------------------------------------------------------------------------------- 1. one-range lists are the single-range call
@pytest.mark.parametrize("checksum", [False, True])
def test_one_range_lists(contexts, s1, checksum):
    data, streams = s1
    ctx = contexts(3, False)
    with Opened(ctx, streams[checksum]) as o:
        for off, ln in sc.ranges_of(len(data)):
            rc1, status1, got1, _ = base._read(ctx, o.h, off, ln)
            rc, status, body, stats = _gather(ctx, o.h, [(off, ln, 0)], ln)
            assert rc == rc1 == 0 and status[2:4] == status1 == [0, 0] and status[:2] == [0, 0], (off, ln)
            assert body.tobytes() == got1 == data[off:off + ln], (off, ln)
            assert stats["items"] == ((off + ln - 1) // 4096 - off // 4096 + 1 if ln else 0)


# ---------------------------------------------------------------------------------------------------- 2. the whole list in one call
@pytest.mark.parametrize("checksum", [False, True])
def test_all_ranges_in_one_call(contexts, s1, checksum):
    data, streams = s1
    ctx = contexts(3, False)
    with Opened(ctx, streams[checksum]) as o:
        ranges, cap = _place(sc.ranges_of(len(data)))
        rc, status, body, stats = _gather(ctx, o.h, ranges, cap)
        assert rc == 0 and status == [0] * (2 + 2 * len(ranges))
        _check_bytes(body, ranges, data)
        assert stats["items"] == 6 and stats["passes"] == 1


# ---------------------------------------------------------------------------------------------------- 3. sharing
def test_sharing(contexts, s1):
    data, streams = s1
    total = len(data)
    ctx = contexts(3, False)
    with Opened(ctx, streams[True]) as o:
        def go(listed):
            ranges, cap = _place(listed)
            rc, status, body, stats = _gather(ctx, o.h, ranges, cap)
            assert rc == 0 and status == [0] * (2 + 2 * len(ranges))
            _check_bytes(body, ranges, data)
            return stats

        assert go([(0, 100), (100, 4096), (4196, 8000)])["items"] == 3
        st = go([(3 * 4096 + 100 * k, 100) for k in range(31)] + [(3 * 4096 + 700, 100)])
        assert (st["items"], st["inPlace"], st["copyJobs"]) == (1, 0, 32)
        st = go([(0, total), (0, total)])
        assert (st["items"], st["inPlace"]) == (6, 0)
        st = go([(0, total)])
        assert (st["items"], st["inPlace"], st["copyJobs"], st["scratchBytes"]) == (6, 6, 0, 0)


# ---------------------------------------------------------------------------------------------------- 4. a stream this backend did not write
@pytest.mark.parametrize("checksum", [False, True])
def test_foreign_stream(contexts, ref, emu, checksum):
    sizes = [1, 70000, 0, 300000, 4096]
    big = sc.source(sum(sizes))
    contents, at = [], 0
    for s in sizes:
        contents.append(big[at:at + s]); at += s
    frames = [ref.compress(c, 19) for c in contents]
    skippable = struct.pack("<II", 0x184D2A53, 11) + b"hello world"
    stream = sc.stream_of(frames, contents, checksum, extra_entries=[(4, skippable)])
    assert sc.emu_validate(emu, stream)[0] == 0
    ctx = contexts(3, False)
    with Opened(ctx, stream) as o:
        assert o.info.maxFrameContent == 300000
        listed = [(0, len(big))]
        edge = 0
        for s in sizes[:-1]:
            edge += s
            listed += [(edge - 1, 2), (max(edge - 3000, 0), 6000), (edge, 1), (edge - 1, 1)]
        ranges, cap = _place(listed, reverse=True)
        rc, status, body, stats = _gather(ctx, o.h, ranges, cap)
        assert rc == 0 and status == [0] * (2 + 2 * len(ranges)), status
        _check_bytes(body, ranges, big)
        assert stats["items"] == 4 and stats["inPlace"] == 0 and stats["scratchBytes"] == len(big), "the empty and the skippable entry are never the decoder's"


# ---------------------------------------------------------------------------------------------------- 5. many ranges, and the same list in several passes
def test_many_ranges_and_passes(contexts):
    src_size, fs = 300 * 4096 + 9, 4096
    data = sc.source(src_size)
    ctx = contexts(3, False)
    stream, st, _ = base._compress(ctx, base._dev(data), fs, True)
    assert st == [0, 0]
    rng = np.random.default_rng(505)
    listed = []
    for _ in range(1000):
        ln = int(rng.integers(1, 3 * 4096 + 1))
        listed.append((int(rng.integers(0, src_size - ln + 1)), ln))
    ranges, cap = _place(listed, rng=rng)
    with Opened(ctx, stream) as o:
        rc, status, body, stats = _gather(ctx, o.h, ranges, cap)
        assert rc == 0 and not any(status)
        _check_bytes(body, ranges, data)
        touched = set()
        for off, ln in listed:
            touched.update(range(off // fs, (off + ln - 1) // fs + 1))
        assert stats["items"] == len(touched) and stats["passes"] == 1
        ctx.L.zhip_seekable_set_scratch_limit(o.h, 16384)
        rc, status, again, limited = _gather(ctx, o.h, ranges, cap)
        assert rc == 0 and not any(status)
        assert limited["passes"] > 1 and limited["items"] == stats["items"] and limited["scratchBytes"] == stats["scratchBytes"]
        assert (again == body).all()
        ctx.L.zhip_seekable_set_scratch_limit(o.h, 0)
        rc, status, again, back = _gather(ctx, o.h, ranges, cap)
        assert rc == 0 and back["passes"] == 1 and (again == body).all()


# ---------------------------------------------------------------------------------------------------- 6. damage
def test_damage(contexts, s1, emu):
    data, streams = s1
    good = streams[True]
    entries, _, at = sc.parse(good)
    total = len(data)
    ctx = contexts(3, False)
    listed = [(100, 2 * 4096 - 100), (2 * 4096 - 5, 4096), (0, 0), (4 * 4096, 4096), (0, total), (3 * 4096 + 9, 1), (2 * 4096, 4096), (5 * 4096, 17)]
    ranges, cap = _place(listed, rng=np.random.default_rng(6))
    needs = lambda f: [bool(l) and o < (f + 1) * 4096 and o + l > f * 4096 for o, l, _ in ranges]

    def check(stream, frame, code):
        assert sc.emu_validate(emu, bytes(stream))[0] == 0
        with Opened(ctx, stream) as o:
            rc, status, body, _ = _gather(ctx, o.h, ranges, cap)
        assert rc == 0
        hit = needs(frame)
        for r, h in enumerate(hit):
            pair = status[2 + 2 * r:4 + 2 * r]
            if h:
                assert pair[1] == frame and (pair[0] == code if code else pair[0] != 0), (r, pair)
            else:
                assert pair == [0, 0], (r, pair)
        first = hit.index(True)
        assert status[:2] == [status[2 + 2 * first], first], "the lowest range that failed"
        _check_bytes(body, ranges, data, only=[not h for h in hit])

    bad = bytearray(good); bad[at + 8 + 2 * 12 + 8] ^= 0x10                 # a bit of entry 2's checksum
    check(bad, 2, 22)
    start3 = sum(e[0] for e in entries[:3])
    bad = bytearray(good); bad[start3 + entries[3][0] // 2] ^= 0x55         # a payload byte of frame 3
    check(bad, 3, None)


# ---------------------------------------------------------------------------------------------------- 7. rejected calls
def test_rejected_calls(contexts, s1):
    data, streams = s1
    total = len(data)
    ctx = contexts(3, False)
    good = [(0, 100, 0), (4000, 200, 100), (total - 1, 1, 300)]
    cap = 301
    with Opened(ctx, streams[False]) as o:
        for bad, want, named, numbers in [
                (good + [(total, 1, 400)], 3, "range 3 ends", (total, 1)),
                (good + [(1 << 63, 1 << 63, 400)], 3, "range 3 ends", (1 << 63,)),
                ([(0, 0, 0), (0, total + 1, 0)], 3, "range 1 ends", (total + 1, total)),
                ([(0, 100, 0), (0, 100, cap - 99)], 3, "range 1 goes", (cap - 99, 100, cap)),
                ([(0, 100, (1 << 64) - 50)], 3, "range 0 goes", ((1 << 64) - 50,)),
                ([(0, 100, 0), (200, 50, 150), (4000, 100, 99)], 6, "ranges 0 and 2 overlap", ()),
                ([(0, 100, 20), (0, 100, 20)], 6, "ranges 0 and 1 overlap", ())]:
            rc, status, body, _ = _gather(ctx, o.h, bad, cap)
            assert rc == want, bad
            assert (body == GUARD_BYTE).all() and status == [-1] * (2 + 2 * len(bad)), "a rejected call writes nothing, d_status included"
            text = base.zstandard_last_error(ctx)
            assert named in text and all(str(n) in text for n in numbers), text
        from zstandard_amd import _lib
        L = ctx.L
        import torch
        status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        buf = torch.full((64,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        one = _table([(0, 1, 0)])
        assert L.zhip_seekable_decompress_ranges_device(ctx.ctx, o.h, None, 1, buf.data_ptr(), 64, status.data_ptr(), None, s) == 6
        assert L.zhip_seekable_decompress_ranges_device(ctx.ctx, o.h, one, 1, buf.data_ptr(), 64, None, None, s) == 6
        assert L.zhip_seekable_decompress_ranges_device(ctx.ctx, o.h, one, 1, None, 64, status.data_ptr(), None, s) == 6
        assert L.zhip_seekable_decompress_ranges_device(ctx.ctx, None, one, 1, buf.data_ptr(), 64, status.data_ptr(), None, s) == 6
        assert L.zhip_seekable_decompress_ranges_device(ctx.ctx, o.h, one, (1 << 27) + 1, buf.data_ptr(), 64, status.data_ptr(), None, s) == 6
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [-1] * 4 and (buf.cpu().numpy() == GUARD_BYTE).all()
        # no ranges, and only empty ones: the status is set, nothing else happens (stats may be NULL)
        rc, status, body, stats = _gather(ctx, o.h, [], cap)
        assert rc == 0 and status == [0, 0] and (body == GUARD_BYTE).all() and stats["items"] == 0
        rc, status, body, stats = _gather(ctx, o.h, [(5, 0, 3), (total, 0, cap)], cap)
        assert rc == 0 and status == [0] * 6 and (body == GUARD_BYTE).all() and stats["passes"] == 0


# ---------------------------------------------------------------------------------------------------- 8. stream order, and the table slots
def test_stream_order(contexts, s1):
    import torch
    data, streams = s1
    total = len(data)
    ctx = contexts(3, False)
    L = ctx.L
    list_a, cap_a = _place([(0, total), (4095, 2), (3 * 4096 + 5, 100)])
    list_b, cap_b = _place([(2 * 4096 - 1, 4098), (0, 0), (total - 20, 20), (100, 4096), (100, 4096)], reverse=True)
    with Opened(ctx, streams[True]) as o:
        staged = o.tensor.clone()
        s = torch.cuda.Stream()                    # non-blocking: not ordered against the null stream
        for round_ in range(2):
            buf_a = torch.full((GUARD + cap_a + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
            buf_b = torch.full((GUARD + cap_b + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
            st_a = torch.full((2 + 2 * len(list_a),), -1, dtype=torch.int32, device="cuda")
            st_b = torch.full((2 + 2 * len(list_b),), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                o.tensor.fill_(0x3C)                           # the stream's bytes are not there yet ...
                o.tensor.copy_(staged, non_blocking=True)      # ... a device copy brings them, and nothing waits for it
            rc_a, stats_a = _queue(ctx, o.h, list_a, buf_a, cap_a, st_a, s)
            rc_b, stats_b = _queue(ctx, o.h, list_b, buf_b, cap_b, st_b, s)
            assert rc_a == 0 and rc_b == 0
            err = base.zstd_error()
            assert L.zhip_ctx_sync(ctx.ctx, s.cuda_stream, st_b.data_ptr(), 1, C.byref(err)) == 0
            assert st_a.cpu().tolist() == [0] * (2 + 2 * len(list_a)) and st_b.cpu().tolist() == [0] * (2 + 2 * len(list_b)), round_
            for buf, ranges, cap in ((buf_a, list_a, cap_a), (buf_b, list_b, cap_b)):
                host = buf.cpu().numpy()
                body = host[GUARD:GUARD + cap]
                _check_bytes(body, ranges, data)
                assert (host[:GUARD] == GUARD_BYTE).all() and (host[GUARD + cap:] == GUARD_BYTE).all() and (body[_untouched(ranges, cap)] == GUARD_BYTE).all()
            assert stats_a["items"] == 6 and stats_b["items"] == 6 and stats_b["inPlace"] == 2, "list b: frame 2 lies inside its first range alone, frame 5 inside its third"


# ---------------------------------------------------------------------------------------------------- 9. dictionary
def test_dictionary(contexts):
    from tests.corpus import Corpus
    blob = open(os.path.join(HERE, "golden", "dict_json4k_16k.bin"), "rb").read()
    data = Corpus(frame_size=4096).json_docs(0, 40).numpy().tobytes()
    assert len(data) == 40 * 4096
    ctx = contexts(3, False, blob)
    stream, st, _ = base._compress(ctx, base._dev(data), 4096, True)
    assert st == [0, 0]
    rng = np.random.default_rng(909)
    listed = []
    for _ in range(64):
        ln = int(rng.integers(1, 3 * 4096))
        listed.append((int(rng.integers(0, len(data) - ln + 1)), ln))
    ranges, cap = _place(listed, rng=rng)
    with Opened(ctx, stream) as o:
        rc, status, body, stats = _gather(ctx, o.h, ranges, cap)
        assert rc == 0 and not any(status), status[:2]
        _check_bytes(body, ranges, data)
        assert 0 < stats["items"] <= 40


# ---------------------------------------------------------------------------------------------------- 10. the Python layer
def test_python_layer(zstd, s1):
    import torch
    import zstandard_amd.seekable as seekable
    data, streams = s1
    total = len(data)
    listed = [(0, 100), (4095, 2), (0, 0), (3 * 4096, 4096 + 17 + 4096), (0, total)]
    ctx = zstd.device.DeviceBatchContext()
    try:
        with zstd.device.SeekableStream(ctx, base._dev(streams[True])) as st:
            views = st.read_ranges(listed)
            assert [v.numel() for v in views] == [l for _, l in listed]
            assert all(v.cpu().numpy().tobytes() == data[o:o + l] for v, (o, l) in zip(views, listed))
            at = 0
            for v in views:                                                # views of ONE tensor, back to back in call order
                assert v.storage_offset() == at and v.untyped_storage().data_ptr() == views[0].untyped_storage().data_ptr(); at += v.numel()
            assert st.last_gather_stats["items"] == 6
            arr = np.array(listed, dtype=np.int64)
            views = st.read_ranges(arr)
            assert all(v.cpu().numpy().tobytes() == data[o:o + l] for v, (o, l) in zip(views, listed))
            assert st.read_ranges([]) == []
            out = torch.full((total + 9000,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
            offs = [total + 8300, 7, 0, 20]
            views = st.read_ranges(listed[:4], out=out, out_offsets=offs[:4])
            host = out.cpu().numpy()
            for (o, l), d, v in zip(listed[:4], offs, views):
                assert host[d:d + l].tobytes() == data[o:o + l] and v.storage_offset() == d and v.numel() == l
            assert (host[_untouched([(o, l, d) for (o, l), d in zip(listed[:4], offs)], out.numel())] == GUARD_BYTE).all()
            with pytest.raises(zstd.ZstdError, match="overlap"):
                st.read_ranges([(0, 10), (0, 10)], out=out, out_offsets=[0, 5])
            with pytest.raises(zstd.ZstdError, match="range 1"):
                st.read_ranges([(0, 10), (total, 1)])
            with pytest.raises(zstd.ZstdError):
                st.read_ranges([(0, 10, 3)])
        with zstd.device.SeekableStream(ctx, base._dev(streams[True]), scratch_limit=4096) as st:
            views = st.read_ranges([(o, l) for o, l in listed if l] * 2)
            assert st.last_gather_stats["passes"] > 1 and st.last_gather_stats["items"] == 6
            assert all(v.cpu().numpy().tobytes() == data[o:o + l] for v, (o, l) in zip(views, [(o, l) for o, l in listed if l] * 2))
            st.set_scratch_limit(0)
            st.read_ranges([(0, total), (0, total)])
            assert st.last_gather_stats["passes"] == 1
        # a frame that fails: the range and the frame are named
        entries, _, at = sc.parse(streams[True])
        bad = bytearray(streams[True]); bad[at + 8 + 2 * 12 + 8] ^= 0x10
        with zstd.device.SeekableStream(ctx, base._dev(bad)) as st:
            with pytest.raises(zstd.ZstdError, match=r"range 2: frame 2: .*[Cc]hecksum"):
                st.read_ranges([(0, 100), (4096, 4096), (3 * 4096 - 1, 1), (0, total)])
            assert [v.cpu().numpy().tobytes() for v in st.read_ranges([(0, 100), (3 * 4096, 5)])] == [data[:100], data[3 * 4096:3 * 4096 + 5]]
    finally:
        ctx.close()
    got = seekable.decompress_ranges(streams[False], listed)
    assert got == [data[o:o + l] for o, l in listed]
    assert seekable.decompress_ranges(streams[False], []) == []
    with pytest.raises(zstd.ZstdError):
        seekable.decompress_ranges(streams[False], [(total, 1)])
    with pytest.raises(zstd.ZstdError):
        seekable.decompress_ranges(b"", [(0, 0)])
