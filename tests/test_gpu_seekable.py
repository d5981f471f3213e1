"""Seekable streams on the GPU (include/zstd_hip.h, "seekable streams"): one HBM buffer compressed as a batch into frames + seek table, any byte range read
back. Every frame is compared with libzstd 1.5.7's for the same chunk (tests/reflib.checker()), every table field with what the layout says, every byte of
every range with the source; nothing is sampled. Streams that reach the GPU damaged pass the host emulator's run of the open call's checks first
(tests/seekable_cases.emu_validate), so no case relies on a read outside the stream."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from tests import reflib
from tests import seekable_cases as sc

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 64, 0xC7
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
    """DeviceBatchContext per (level, write_checksum[, dictionary]), made once"""
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
    return sc.emu(tmp_path_factory.mktemp("emu_seekable_gpu"))


def _dev(data):
    import torch
    if not len(data):
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def _flags(write_checksum):
    return reflib.DEFAULT_FLAGS | (reflib.F_CHECKSUM if write_checksum else 0)


def _compress(ctx, src_t, frame_size, checksum, capacity=None, stream=None):
    """the C call with a guard behind dstCapacity -> (stream bytes, [code, index], stream size)"""
    import torch
    ctx._ensure_cparams()
    L = ctx.L
    flags = 1 if checksum else 0
    cap = L.zhip_seekable_bound(src_t.numel(), frame_size, flags) if capacity is None else capacity
    dst = torch.full((cap + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    size = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = L.zhip_seekable_compress_device(ctx.ctx, src_t.data_ptr(), src_t.numel(), frame_size, flags, dst.data_ptr(), cap, size.data_ptr(), status.data_ptr(), s.cuda_stream)
    assert rc == 0, zstandard_last_error(ctx)
    err = zstd_error()
    rc = L.zhip_ctx_sync(ctx.ctx, s.cuda_stream, status.data_ptr(), 1, C.byref(err))
    st = status.cpu().tolist()
    assert (rc == 0) == (st[0] == 0) and (rc == 0 or (rc == 1 and err.zstdErr == st[0]))
    host = dst.cpu().numpy()
    assert (host[cap:] == GUARD_BYTE).all(), "bytes at or beyond d_dst + dstCapacity were written"
    n = int(size[0])
    if st[0]:
        assert n == 0 and (host == GUARD_BYTE).all(), "a failed stream writes nothing"
    return host[:n].tobytes(), st, n


def zstd_error():
    from zstandard_amd import _lib
    return _lib.Error()


def zstandard_last_error(ctx):
    return ctx.L.zhip_last_error().decode()


def _open(ctx, stream_t):
    """-> (rc, zstd error code, handle, info)"""
    from zstandard_amd import _lib
    import torch
    h, info, err = C.c_void_p(), _lib.SeekableInfo(), _lib.Error()
    rc = ctx.L.zhip_seekable_open_device(ctx.ctx, stream_t.data_ptr(), stream_t.numel(), torch.cuda.current_stream().cuda_stream, C.byref(h), C.byref(info), C.byref(err))
    return rc, err.zstdErr, (h if rc == 0 else None), info


def _read(ctx, handle, offset, length):
    """the C call into a buffer with guards on both sides -> (rc, [code, index], bytes, whole guarded buffer)"""
    import torch
    buf = torch.full((GUARD + length + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    rc = ctx.L.zhip_seekable_decompress_device(ctx.ctx, handle, offset, length, buf.data_ptr() + GUARD, status.data_ptr(), s.cuda_stream)
    s.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == GUARD_BYTE).all() and (host[GUARD + length:] == GUARD_BYTE).all(), "bytes of d_dst outside [0, length) were written"
    return rc, status.cpu().tolist(), host[GUARD:GUARD + length].tobytes(), host


def _libzstd_decompress(ref, stream, size, dict_data=None):
    """ZSTD_decompress: every frame of the stream, the skippable table frame passed over"""
    L = ref.lib
    L.ZSTD_decompress.restype = C.c_size_t
    L.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    dst = C.create_string_buffer(max(size, 1))
    r = L.ZSTD_decompress(dst, size, stream, len(stream))
    assert not L.ZSTD_isError(r), L.ZSTD_getErrorName(r)
    return dst.raw[:r]


def _check_stream(stream, data, frame_size, checksum, ref, oracle, level, flags, dict_data=None):
    parts = sc.chunks(data, frame_size)
    entries, ck, at = sc.parse(stream)
    assert ck == checksum and len(entries) == len(parts)
    pos = 0
    for i, (p, e) in enumerate(zip(parts, entries)):
        want = ref.compress(p, level, flags, dict_data) if dict_data else ref.compress(p, level, flags)
        assert e[0] == len(want) and e[1] == len(p), "entry %d" % i
        assert stream[pos:pos + e[0]] == want, "frame %d is not libzstd's" % i
        if checksum:
            assert e[2] == oracle.xxh64(p) & 0xFFFFFFFF, "checksum %d" % i
        pos += e[0]
    assert pos == at


# ---------------------------------------------------------------------------------------------------- 1. streams are libzstd's frames plus the table
@pytest.mark.parametrize("case", sc.CASES, ids=["%dx%d" % c for c in sc.CASES])
def test_streams_are_libzstd_frames_plus_table(contexts, ref, oracle, case):
    src_size, fs = case
    data = sc.source(src_size)
    src_t = _dev(data)
    levels = (3, 1, 5) if case == sc.CASES[-1] else (3, 1)
    for level in levels:
        for wc in (False, True):
            ctx = contexts(level, wc)
            for checksum in (False, True):
                stream, st, n = _compress(ctx, src_t, fs, checksum)
                assert st == [0, 0], (level, wc, checksum, st)
                assert n <= ctx.L.zhip_seekable_bound(src_size, fs, int(checksum))
                _check_stream(stream, data, fs, checksum, ref, oracle, level, _flags(wc))
                assert _libzstd_decompress(ref, stream, src_size) == data


# ---------------------------------------------------------------------------------------------------- 2. a refused chunk fails the stream
def test_refused_chunk_fails_the_stream(contexts):
    src_size, fs = 3 * 131072 + 1, 131072
    stream, st, n = _compress(contexts(5, False), _dev(sc.source(src_size)), fs, True)
    assert st == [40, 3] and n == 0 and stream == b""


# ---------------------------------------------------------------------------------------------------- 3. capacity
@pytest.mark.parametrize("checksum", [False, True])
def test_capacity(contexts, checksum):
    src_size, fs = sc.RANGE_CASE
    ctx = contexts(3, False)
    src_t = _dev(sc.source(src_size))
    whole, st, n = _compress(ctx, src_t, fs, checksum)
    assert st == [0, 0]
    exact, st, n2 = _compress(ctx, src_t, fs, checksum, capacity=n)
    assert st == [0, 0] and n2 == n and exact == whole
    _, st, n3 = _compress(ctx, src_t, fs, checksum, capacity=n - 1)
    assert st[0] == 70 and n3 == 0
    entries, _, at = sc.parse(whole)
    _, st, _ = _compress(ctx, src_t, fs, checksum, capacity=entries[0][0] + entries[1][0] + 5)
    assert st == [70, 2], "the first frame that ends beyond the capacity"
    _, st, _ = _compress(ctx, _dev(b""), fs, checksum, capacity=16)
    assert st[0] == 70
    empty, st, n0 = _compress(ctx, _dev(b""), fs, checksum, capacity=17)
    assert st == [0, 0] and empty == sc.table([], checksum)


# ---------------------------------------------------------------------------------------------------- 4. ranges
@pytest.fixture(scope="module")
def range_streams(contexts):
    src_size, fs = sc.RANGE_CASE
    data = sc.source(src_size)
    out = {}
    for checksum in (False, True):
        stream, st, _ = _compress(contexts(3, checksum), _dev(data), fs, checksum)
        assert st == [0, 0]
        out[checksum] = stream
    return data, out


@pytest.mark.parametrize("checksum", [False, True])
def test_ranges(contexts, range_streams, emu, checksum):
    data, streams = range_streams
    stream = streams[checksum]
    assert sc.emu_validate(emu, stream)[0] == 0
    ctx = contexts(3, False)
    st_t = _dev(stream)
    rc, _, h, info = _open(ctx, st_t)
    assert rc == 0
    try:
        total = len(data)
        assert (info.streamSize, info.contentSize, info.nFrames, info.maxFrameContent, info.checksumFlag) == (len(stream), total, 6, 4096, int(checksum))
        for off, ln in sc.ranges_of(total):
            rc, status, got, _ = _read(ctx, h, off, ln)
            assert rc == 0 and status == [0, 0], (off, ln, status)
            assert got == data[off:off + ln], (off, ln)
        for off, ln in ((total, 1), (0, total + 1)):
            rc, status, _, host = _read(ctx, h, off, ln)
            assert rc == 3 and (host == GUARD_BYTE).all() and status == [-1, -1], "a range outside the content: size mismatch, nothing written"
            text = zstandard_last_error(ctx)
            assert str(off + ln) in text and str(total) in text
    finally:
        ctx.L.zhip_seekable_close(h)


# ---------------------------------------------------------------------------------------------------- 5. a stream this backend did not write
@pytest.mark.parametrize("checksum", [False, True])
def test_foreign_stream(contexts, ref, emu, checksum):
    sizes = [1, 70000, 0, 300000, 4096]
    big = sc.source(sum(sizes))
    contents, at = [], 0
    for s in sizes:
        contents.append(big[at:at + s]); at += s
    frames = [ref.compress(c, 19) for c in contents]
    skippable = struct.pack("<II", 0x184D2A53, 11) + b"hello world"
    stream = sc.stream_of(frames, contents, checksum, extra_entries=[(4, skippable)])      # ... 300 000, the skippable frame, 4 096
    assert sc.emu_validate(emu, stream)[0] == 0
    assert _libzstd_decompress(ref, stream, len(big)) == big
    ctx = contexts(3, False)
    st_t = _dev(stream)
    rc, _, h, info = _open(ctx, st_t)
    assert rc == 0
    try:
        assert (info.contentSize, info.nFrames, info.maxFrameContent, info.checksumFlag) == (len(big), 6, 300000, int(checksum))
        ranges = [(0, len(big))]
        edge = 0
        for s in sizes[:-1]:
            edge += s
            ranges += [(edge - 1, 2), (max(edge - 3000, 0), 6000), (edge, 1), (edge - 1, 1)]
        for off, ln in ranges:
            rc, status, got, _ = _read(ctx, h, off, ln)
            assert rc == 0 and status == [0, 0], (off, ln, status)
            assert got == big[off:off + ln], (off, ln)
    finally:
        ctx.L.zhip_seekable_close(h)


# ---------------------------------------------------------------------------------------------------- 6. damage
def test_damage(contexts, range_streams, emu):
    data, streams = range_streams
    good = streams[True]
    entries, _, at = sc.parse(good)
    ctx = contexts(3, False)
    # a bit of entry 2's checksum
    bad = bytearray(good); bad[at + 8 + 2 * 12 + 8] ^= 0x10
    assert sc.emu_validate(emu, bytes(bad))[0] == 0
    t = _dev(bad)
    rc, _, h, _ = _open(ctx, t)
    assert rc == 0
    try:
        rc, status, _, _ = _read(ctx, h, 2 * 4096 - 5, 4096)
        assert rc == 0 and status == [22, 2]
        rc, status, got, _ = _read(ctx, h, 100, 2 * 4096 - 100)
        assert rc == 0 and status == [0, 0] and got == data[100:2 * 4096]
    finally:
        ctx.L.zhip_seekable_close(h)
    # a payload byte of frame 3
    start3 = sum(e[0] for e in entries[:3])
    bad = bytearray(good); bad[start3 + entries[3][0] // 2] ^= 0x55
    assert sc.emu_validate(emu, bytes(bad))[0] == 0
    t = _dev(bad)
    rc, _, h, _ = _open(ctx, t)
    assert rc == 0
    try:
        rc, status, _, _ = _read(ctx, h, 0, len(data))
        assert rc == 0 and status[0] != 0 and status[1] == 3
        rc, status, got, _ = _read(ctx, h, 4 * 4096, 4096)
        assert rc == 0 and status == [0, 0] and got == data[4 * 4096:5 * 4096]
    finally:
        ctx.L.zhip_seekable_close(h)
    # the validator's streams: what the emulator refuses, the open call refuses with the same code, and makes no handle
    for name, stream, want in sc.validator_damage(good, 6, True):
        assert sc.emu_validate(emu, stream)[0] == want, name
        rc, code, h, _ = _open(ctx, _dev(stream))
        assert rc == 1 and code == want and h is None, name


# ---------------------------------------------------------------------------------------------------- 7. stream order
def test_stream_order(contexts):
    import torch
    src_size, fs = 40 * 4096 + 9, 4096
    data = sc.source(src_size)
    ctx = contexts(3, False)
    want, st, n = _compress(ctx, _dev(data), fs, True)
    assert st == [0, 0]
    L = ctx.L
    cap = L.zhip_seekable_bound(src_size, fs, 1)
    staged = _dev(data)
    src = torch.full((src_size,), 0x3C, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    size = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()                    # non-blocking: not ordered against the null stream
    with torch.cuda.stream(s):
        src.copy_(staged, non_blocking=True)   # a device kernel fills the source ...
    rc = L.zhip_seekable_compress_device(ctx.ctx, src.data_ptr(), src_size, fs, 1, dst.data_ptr(), cap, size.data_ptr(), status.data_ptr(), s.cuda_stream)      # ... nothing waited for
    assert rc == 0
    err = zstd_error()
    assert L.zhip_ctx_sync(ctx.ctx, s.cuda_stream, status.data_ptr(), 1, C.byref(err)) == 0
    assert int(size[0]) == n and dst[:n].cpu().numpy().tobytes() == want


# ---------------------------------------------------------------------------------------------------- 8. dictionary
def test_dictionary(zstd, contexts, ref, oracle):
    from tests.corpus import Corpus
    blob = open(os.path.join(HERE, "golden", "dict_json4k_16k.bin"), "rb").read()
    data = Corpus(frame_size=4096).json_docs(0, 40).numpy().tobytes()
    assert len(data) == 40 * 4096
    ctx = contexts(3, False, blob)
    stream, st, _ = _compress(ctx, _dev(data), 4096, True)
    assert st == [0, 0]
    _check_stream(stream, data, 4096, True, ref, oracle, 3, reflib.DEFAULT_FLAGS, dict_data=blob)
    t = _dev(stream)
    rc, _, h, info = _open(ctx, t)
    assert rc == 0 and info.nFrames == 40
    try:
        for off, ln in [(0, len(data)), (4095, 2), (4097, 8190), (39 * 4096 + 1, 4095), (17 * 4096, 4096)]:
            rc, status, got, _ = _read(ctx, h, off, ln)
            assert rc == 0 and status == [0, 0] and got == data[off:off + ln], (off, ln, status)
    finally:
        ctx.L.zhip_seekable_close(h)


# ---------------------------------------------------------------------------------------------------- 9. the size hint is the caller's
def test_size_hint_is_left_alone(zstd, ref):
    import torch
    small = sc.source(2045 * 2048)
    raws = [small[i * 2048:(i + 1) * 2048] for i in range(2045)] + [sc.source(200000), sc.source(200001), sc.source(150000)]
    frames = [ref.compress(r) for r in raws]
    flens = np.array([len(f) for f in frames], dtype=np.int64); rlens = np.array([len(r) for r in raws], dtype=np.int64)
    ssegs = np.stack([np.concatenate([[0], np.cumsum(flens)[:-1]]), flens], axis=1)
    dsegs = np.stack([np.concatenate([[0], np.cumsum(rlens)[:-1]]), rlens], axis=1)
    src = _dev(b"".join(frames)); ssegs_t = torch.from_numpy(ssegs).cuda(); dsegs_t = torch.from_numpy(dsegs).cuda()

    def plain_decode(ctx):
        dst = torch.zeros(int(rlens.sum()), dtype=torch.uint8, device="cuda")
        out_sizes = torch.zeros(2048, dtype=torch.int64, device="cuda"); status = torch.full((2048,), -1, dtype=torch.int32, device="cuda")
        ctx.decompress(src, ssegs_t, dst, dsegs_t, out_sizes, status)
        n = ctx.decode_fallbacks()
        assert not status.cpu().numpy().any() and dst.cpu().numpy().tobytes() == b"".join(raws)
        return n

    a = zstd.device.DeviceBatchContext()
    b = zstd.device.DeviceBatchContext()
    try:
        a.set_size_hint(0)
        without = plain_decode(a)
        b.set_size_hint(0)
        data = sc.source(700000)
        stream = b.seekable_compress(_dev(data), frame_size=300000, checksum=True)
        with zstd.device.SeekableStream(b, stream) as st:
            assert st.max_frame_content == 300000 and st.n_frames == 3
            assert st.read().cpu().numpy().tobytes() == data
            assert st.read(299999, 2).cpu().numpy().tobytes() == data[299999:300001]
        assert plain_decode(b) == without
        assert without >= 3, "the frames above one block are the generic kernel's without a hint: a hint left behind would have shown"
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------------- 10. the Python layer
def test_python_layer(zstd, ref):
    import zstandard_amd.seekable as seekable
    data = sc.source((1 << 20) + 3)
    stream = seekable.compress(data, level=3, frame_size=65536, checksum=True)
    entries, ck, _ = sc.parse(stream)
    assert ck and len(entries) == 17 and [e[1] for e in entries] == [65536] * 16 + [3]
    assert _libzstd_decompress(ref, stream, len(data)) == data
    total = len(data)
    assert seekable.decompress(stream) == data
    for off, ln in [(0, 0), (0, 1), (65535, 2), (65536, 65536), (65537, 2 * 65536 - 2), (total - 1, 1), (total, 0)]:
        assert seekable.decompress(stream, off, ln) == data[off:off + ln], (off, ln)
    assert seekable.decompress(stream, offset=total - 5) == data[-5:]
    assert seekable.compress(b"", frame_size=65536) == sc.table([], False)
    assert seekable.decompress(sc.table([], False)) == b""
    for bad in (stream[:-1], stream[:-9], b"", stream[:10]):
        with pytest.raises(zstd.ZstdError):
            seekable.decompress(bad)
    with pytest.raises(zstd.ZstdError):
        seekable.decompress(stream, total, 1)
    with pytest.raises(zstd.ZstdError):
        seekable.compress(data, frame_size=0)
    with pytest.raises(zstd.ZstdError):
        seekable.compress(data[: 3 * 131072 + 1], level=5)          # the one-byte last chunk is none of level 5's sources here
