"""Editing seekable streams on the GPU (include/zstd_hip.h: zhip_seekable_edit_device, zhip_seekable_edit_bound; SeekableStream.edit and what is built on it):
append, replace, drop, reorder and repeat records of a stream in HBM. The oracle is exact: the expected stream is built in Python (tests/seekable_edit_cases.model)
-- a kept frame is the old stream's bytes sliced by its table, a new frame is libzstd 1.5.7's for the record (tests/reflib.checker()), the table is written from
the format description -- and the WHOLE stream is compared byte for byte; then libzstd decodes it whole and read_records reads records back. Every destination
of the C call has 64 guard bytes of 0xC7 on both sides."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import reflib
from tests import seekable_cases as sc
from tests import seekable_edit_cases as ec
from tests import seekable_record_cases as rec

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 64, 0xC7
HERE = os.path.dirname(os.path.abspath(__file__))
F, R = ec.FRAME, ec.RECORD


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

    def get(level=3, dict_data=None, match_finder="libzstd"):
        key = (level, dict_data, match_finder)
        if key not in made:
            made[key] = zstd.device.DeviceBatchContext(level=level, dict_data=dict_data, match_finder=match_finder)
        return made[key]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def checker():
    return reflib.checker()


def _dev(data):
    import torch
    if not len(data):
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def _table(records):
    import torch
    if not len(records):
        return torch.zeros((0, 2), dtype=torch.int64, device="cuda")
    return torch.from_numpy(rec.records_array(records).view(np.int64)).cuda()


def _back_to_back(parts):
    records, at = [], 0
    for p in parts:
        records.append((at, len(p))); at += len(p)
    return records


def _libzstd_decompress(ref, stream, size):
    L = ref.lib
    L.ZSTD_decompress.restype = C.c_size_t
    L.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    dst = C.create_string_buffer(max(size, 1))
    r = L.ZSTD_decompress(dst, size, stream, len(stream))
    assert not L.ZSTD_isError(r), L.ZSTD_getErrorName(r)
    return dst.raw[:r]


@pytest.fixture(scope="module")
def base(zstd, contexts, checker):
    """the old stream of most tests: 300 records of 1 .. 9 000 bytes and EDGE_LENGTHS at level 3, with and without checksums -- libzstd's frames and the table,
    written here --, and 40 new records with libzstd's frames for them"""
    rng = np.random.default_rng(1200)
    lengths = [int(x) for x in rng.integers(1, 9001, size=300)] + rec.EDGE_LENGTHS
    data = sc.source(sum(lengths) + 200000)
    parts, at = [], 0
    for l in lengths:
        parts.append(data[at:at + l]); at += l
    frames = [checker.compress(p, 3, reflib.DEFAULT_FLAGS) for p in parts]
    new_lengths = [int(x) for x in rng.integers(1, 9001, size=38)] + [0, 131073]
    new_parts = [data[at - 50000 + 977 * j:at - 50000 + 977 * j + l] for j, l in enumerate(new_lengths)]
    new_frames = [checker.compress(p, 3, reflib.DEFAULT_FLAGS) for p in new_parts]
    streams = {ck: sc.stream_of(frames, parts, ck) for ck in (False, True)}
    # the writer under test makes the same stream (the records call's own tests compare every frame)
    got = contexts().seekable_compress_records(_dev(b"".join(parts)), _back_to_back(parts), checksum=True).cpu().numpy().tobytes()
    assert got == streams[True]
    return dict(parts=parts, frames=frames, streams=streams, new_parts=new_parts, new_frames=new_frames, n=len(parts))


def _edit(ctx, st, picks, parts=(), checksum=False, capacity=None, dst=None, stream=None, flags=None, max_record=None, records=None, src_t=None):
    """the C call into a destination with guards on both sides (dst: the caller's guarded buffer, for the call in place) -> dict(rc, status, size, host: the
    whole guarded buffer, cap). parts: the new records, laid out back to back (or records / src_t as given)"""
    import torch
    from zstandard_amd import _lib
    L = ctx.L
    n = len(parts) if records is None else len(records)
    if n:
        ctx._ensure_cparams()
    if records is None:
        records = _back_to_back(parts)
        src_t = _dev(b"".join(parts))
    pk = np.array(picks, dtype=np.uint32).reshape(-1, 2) if len(picks) else np.zeros((1, 2), dtype=np.uint32)
    k = len(picks)
    lengths = [l for _, l in records]
    max_record = max(lengths + [0]) if max_record is None else max_record
    flags = (1 if checksum else 0) if flags is None else flags
    handle = st.handle if st is not None else None
    cap = L.zhip_seekable_edit_bound(handle, pk.ctypes.data, k, max_record, flags) if capacity is None else capacity
    if dst is None:
        dst = torch.full((GUARD + cap + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    table = _table(records)
    size = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = L.zhip_seekable_edit_device(ctx.ctx, handle, pk.ctypes.data, k, src_t.data_ptr() if n else None, src_t.numel() if n else 0, table.data_ptr() if n else None, n,
                                     sum(lengths), max_record, flags, dst.data_ptr() + GUARD, cap, size.data_ptr(), status.data_ptr(), s.cuda_stream)
    message = L.zhip_last_error().decode()
    if rc == 0:
        err = _lib.Error()
        sync = L.zhip_ctx_sync(ctx.ctx, s.cuda_stream, status.data_ptr(), 1, C.byref(err))
        st2 = status.cpu().tolist()
        assert (sync == 0) == (st2[0] == 0) and (sync == 0 or (sync == 1 and err.zstdErr == st2[0]))
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    assert (host[:GUARD] == GUARD_BYTE).all() and (host[GUARD + cap:GUARD + cap + GUARD] == GUARD_BYTE).all(), "bytes outside [d_dst, d_dst + dstCapacity) were written"
    return dict(rc=rc, status=status.cpu().tolist(), size=int(size[0]), host=host, cap=cap, message=message)


def _stream_of(got):
    return got["host"][GUARD:GUARD + got["size"]].tobytes()


def _nothing_written(got, old=None):
    """after a failure: the size is 0 and the destination is what it was (in place: the old stream, guard bytes behind it)"""
    assert got["size"] == 0
    body = got["host"][GUARD:GUARD + got["cap"]]
    if old is not None:
        assert body[:len(old)].tobytes() == old, "in place the old stream is intact"
        body = body[len(old):]
    assert (body == GUARD_BYTE).all(), "a failed edit writes nothing"


def _refused(got, rc):
    assert got["rc"] == rc and got["status"] == [-1, -1] and got["size"] == -1, "a refused call queues nothing and writes nothing, the status included"
    assert (got["host"] == GUARD_BYTE).all()


def _reads_back(zstd, ctx, checker, stream, contents):
    """libzstd decodes the whole stream; read_records reads every record"""
    whole = b"".join(contents)
    assert _libzstd_decompress(checker, stream, len(whole)) == whole
    with zstd.device.SeekableStream(ctx, _dev(stream)) as st:
        assert st.n_frames == len(contents)
        views = st.read_records(list(range(len(contents))))
        assert [v.cpu().numpy().tobytes() for v in views] == list(contents)


def _contents(base, picks, new_parts):
    return [base["parts"][i] if k == F else new_parts[i] for k, i in picks]


def _in_place_buffer(old, cap):
    import torch
    buf = torch.full((GUARD + cap + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + len(old)] = _dev(old)
    return buf


# ---------------------------------------------------------------------------------------------------- 1. append
@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("in_place", [False, True])
def test_append(zstd, contexts, checker, base, checksum, in_place):
    ctx = contexts()
    old = base["streams"][checksum]
    picks = ec.identity_picks(base["n"]) + [(R, j) for j in range(40)]
    want = ec.model(old, picks, base["new_frames"], base["new_parts"])
    if not in_place:
        with zstd.device.SeekableStream(ctx, _dev(old)) as st:
            got = _edit(ctx, st, picks, base["new_parts"], checksum)
            assert got["rc"] == 0 and got["status"] == [0, 0] and got["size"] <= got["cap"]
            assert _stream_of(got) == want
            src_t, records = _dev(b"".join(base["new_parts"])), _back_to_back(base["new_parts"])
            assert st.append_records(src_t, records).cpu().numpy().tobytes() == want
    else:
        cap = len(old) + sum(rec.compress_bound(len(p)) for p in base["new_parts"]) + 12 * 40
        buf = _in_place_buffer(old, cap)
        with zstd.device.SeekableStream(ctx, buf[GUARD:GUARD + len(old)]) as st:
            got = _edit(ctx, st, picks, base["new_parts"], checksum, capacity=cap, dst=buf)
        assert got["rc"] == 0 and got["status"] == [0, 0]
        assert _stream_of(got) == want
        assert (got["host"][GUARD + got["size"]:] == GUARD_BYTE).all()
        # the Python form closes the object and returns the view to open again
        buf = _in_place_buffer(old, cap)
        room = buf[GUARD:GUARD + cap]
        st = zstd.device.SeekableStream(ctx, room[:len(old)])
        out = st.append_records(_dev(b"".join(base["new_parts"])), _back_to_back(base["new_parts"]), buffer=room)
        assert st.handle is None and out.data_ptr() == room.data_ptr() and out.cpu().numpy().tobytes() == want
        contents = base["parts"] + base["new_parts"]
        with zstd.device.SeekableStream(ctx, out) as again:                  # the result where it lies: it opens again and reads every record
            assert again.n_frames == len(contents) and again.has_checksums == checksum
            assert [v.cpu().numpy().tobytes() for v in again.read_records(list(range(len(contents))))] == contents
    _reads_back(zstd, ctx, checker, want, base["parts"] + base["new_parts"])


# ---------------------------------------------------------------------------------------------------- 2. replace, delete, reorder, repeat, identity
@pytest.mark.parametrize("checksum", [False, True])
def test_replace_delete_reorder_repeat(zstd, contexts, checker, base, checksum):
    ctx = contexts()
    old = base["streams"][checksum]
    n = base["n"]
    rng = np.random.default_rng(77)
    with zstd.device.SeekableStream(ctx, _dev(old)) as st:
        # replace 7
        idx = [int(x) for x in rng.choice(n, size=7, replace=False)]
        new = base["new_parts"][:7]
        picks = ec.identity_picks(n)
        for j, i in enumerate(idx):
            picks[i] = (R, j)
        want = ec.model(old, picks, base["new_frames"], base["new_parts"])
        assert st.replace_records(idx, _dev(b"".join(new)), _back_to_back(new)).cpu().numpy().tobytes() == want
        _reads_back(zstd, ctx, checker, want, _contents(base, picks, base["new_parts"]))
        # delete 30
        gone = set(int(x) for x in rng.choice(n, size=30, replace=False))
        picks = [(F, i) for i in range(n) if i not in gone]
        want = ec.model(old, picks)
        assert st.delete_records(sorted(gone)).cpu().numpy().tobytes() == want
        _reads_back(zstd, ctx, checker, want, _contents(base, picks, []))
        # reorder by a permutation
        order = [int(x) for x in rng.permutation(n)]
        want = ec.model(old, [(F, i) for i in order])
        assert st.reorder(order).cpu().numpy().tobytes() == want
        _reads_back(zstd, ctx, checker, want, [base["parts"][i] for i in order])
        # one frame 5 times
        order = [3, 17, 17, 17, 17, 17, 4]
        want = ec.model(old, [(F, i) for i in order])
        assert st.reorder(order).cpu().numpy().tobytes() == want
        # identity; no picks
        got = _edit(ctx, st, ec.identity_picks(n), checksum=checksum)
        assert got["status"] == [0, 0] and _stream_of(got) == old and got["size"] == got["cap"], "the bound of a pure move is exact"
        assert st.reorder([]).cpu().numpy().tobytes() == sc.table([], checksum) and len(sc.table([], checksum)) == 17


def test_identity_of_another_writers_stream(zstd, contexts, checker):
    """frames of other levels and flags, an empty frame, a skippable frame listed in the table: kept as they are"""
    parts = [sc.source(5000), b"", sc.source(70000)[60000:], sc.source(300000)[100:], b"x"]
    frames = [checker.compress(parts[0], 1, reflib.DEFAULT_FLAGS), checker.compress(b"", 3, reflib.DEFAULT_FLAGS), checker.compress(parts[2], 9, reflib.DEFAULT_FLAGS | reflib.F_CHECKSUM),
              checker.compress(parts[3], -5, reflib.DEFAULT_FLAGS), checker.compress(parts[4], 19, reflib.DEFAULT_FLAGS)]
    skippable = (0x184D2A57).to_bytes(4, "little") + (11).to_bytes(4, "little") + b"hello world"
    for checksum in (False, True):
        old = sc.stream_of(frames, parts, checksum, extra_entries=[(2, skippable)])
        ctx = contexts()
        with zstd.device.SeekableStream(ctx, _dev(old)) as st:
            assert st.n_frames == 6
            assert st.reorder(list(range(6))).cpu().numpy().tobytes() == old
            order = [5, 2, 0, 2, 1]
            got = st.reorder(order).cpu().numpy().tobytes()
        assert got == ec.model(old, [(F, i) for i in order])
        listed = parts[:2] + [b""] + parts[2:]
        assert _libzstd_decompress(checker, got, 400000) == b"".join(listed[i] for i in order)


# ---------------------------------------------------------------------------------------------------- 3. without an old stream: the records call's bytes
@pytest.mark.parametrize("kind", ["libzstd", "wave", "dictionary"])
def test_old_null_equals_the_records_call(zstd, contexts, checker, base, kind):
    if kind == "dictionary":
        from tests.corpus import Corpus
        blob = open(os.path.join(HERE, "golden", "dict_json4k_16k.bin"), "rb").read()
        docs = Corpus(frame_size=4096).json_docs(0, 256).numpy().tobytes()
        parts = [docs[i * 4096:(i + 1) * 4096] for i in range(256)]
        ctx = contexts(3, blob)
    else:
        parts = [p for p in base["parts"] if len(p) <= 131072] if kind == "wave" else base["parts"]
        ctx = contexts(3, None, kind)
    src_t, records = _dev(b"".join(parts)), _back_to_back(parts)
    n = len(parts)
    for checksum in (False, True):
        want = ctx.seekable_compress_records(src_t, records, checksum=checksum).cpu().numpy().tobytes()
        picks = [(R, j) for j in range(n)]
        got = _edit(ctx, None, picks, checksum=checksum, records=records, src_t=src_t)
        assert got["rc"] == 0 and got["status"] == [0, 0] and _stream_of(got) == want
        assert ctx.seekable_edit(picks, src_t, records, checksum=checksum).cpu().numpy().tobytes() == want
    if kind == "dictionary":
        frames = [checker.compress(p, 3, reflib.DEFAULT_FLAGS, blob) for p in parts]
        assert want == sc.stream_of(frames, parts, True)
        # and with an old stream: frames written with the dictionary kept, new ones compressed with it
        with zstd.device.SeekableStream(ctx, _dev(want)) as st:
            picks = [(F, 5), (R, 0), (F, 0), (R, 7)]
            assert st.edit(picks, src_t, records).cpu().numpy().tobytes() == ec.model(want, picks, frames, parts)
    # records in any order, repeated, dropped
    picks = [(R, 5), (R, 0), (R, 5), (R, n - 1)]
    both = ctx.seekable_edit(picks, src_t, records, checksum=True).cpu().numpy().tobytes()
    entries, _, offs = ec.frame_offsets(want)
    assert both == ec.model(None, picks, [want[offs[j]:offs[j + 1]] for j in range(n)], parts, True)


# ---------------------------------------------------------------------------------------------------- 4. frames of many tiles
def test_frames_of_many_tiles(zstd, contexts, checker, base):
    """a record of 400 000 bytes (several blocks, 98 tiles and more) among the picks, and a kept frame of that size"""
    ctx = contexts()
    old = base["streams"][True]
    n = base["n"]
    big_kept = n - 1
    assert len(base["parts"][big_kept]) == 400000
    big = sc.source(900000)[450000:850000]
    new_parts = [b"abc", big, sc.source(100)]
    new_frames = [checker.compress(p, 3, reflib.DEFAULT_FLAGS) for p in new_parts]
    assert len(new_frames[1]) > 20 * ec.COPY_TILE
    picks = [(F, 1), (R, 1), (F, big_kept), (R, 0), (F, big_kept), (R, 1), (R, 2)]
    with zstd.device.SeekableStream(ctx, _dev(old)) as st:
        got = _edit(ctx, st, picks, new_parts, True)
    want = ec.model(old, picks, new_frames, new_parts)
    assert got["status"] == [0, 0] and _stream_of(got) == want
    _reads_back(zstd, ctx, checker, want, _contents(base, picks, new_parts))


# ---------------------------------------------------------------------------------------------------- 5. scan spans longer than one tile
def test_scan_spans_longer_than_one_tile(zstd, contexts, base):
    """262 145 + 300 picks that name the 300 random old frames over and over: the table, a sample of 512 frames and the stream size against the model"""
    import torch
    ctx = contexts()
    old = base["streams"][True]
    entries, _, offs = ec.frame_offsets(old)
    k = 1024 * 256 + 1 + 300
    rng = np.random.default_rng(262445)
    index = rng.integers(0, 300, size=k)
    picks = np.stack([np.zeros(k, dtype=np.int64), index], axis=1)
    sizes = np.array([e[0] for e in entries], dtype=np.int64)[index]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    with zstd.device.SeekableStream(ctx, _dev(old)) as st:
        out = st.edit(picks)
    table_at = int(starts[-1])
    assert out.numel() == table_at + rec.table_size(k, True)
    table = out[table_at:].cpu().numpy().tobytes()
    e = np.array([entries[i] for i in range(300)], dtype=np.uint32)[index]
    assert table == sc.table([tuple(int(v) for v in row) for row in e], True)
    for p in [0, 1, k - 1, k - 2] + [int(x) for x in rng.integers(0, k, size=508)]:
        i = int(index[p])
        assert out[int(starts[p]):int(starts[p + 1])].cpu().numpy().tobytes() == old[offs[i]:offs[i + 1]], "pick %d" % p
    del out
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- 6. failures
def test_refused_record(zstd, contexts, base):
    """level 5 refuses a record of 1 000 bytes: status 40 at its pick's position; the same record unpicked does not fail the call"""
    ctx = contexts(5)
    old = base["streams"][True]
    n = base["n"]
    new_parts = [sc.source(40000)[:20000], sc.source(3000)[2000:], sc.source(90000)[50000:]]
    assert len(new_parts[1]) == 1000
    with zstd.device.SeekableStream(ctx, _dev(old)) as st:
        picks = [(F, 0), (R, 0), (F, 1), (R, 1), (R, 2), (R, 1)]
        got = _edit(ctx, st, picks, new_parts, True)
        assert got["rc"] == 0 and got["status"] == [40, 3]
        _nothing_written(got)
        with pytest.raises(zstd.ZstdError, match="position 3"):
            st.edit(picks, _dev(b"".join(new_parts)), _back_to_back(new_parts))
        got = _edit(ctx, st, ec.identity_picks(n), new_parts, True)
        assert got["status"] == [0, 0] and _stream_of(got) == old
        # in place: the old stream is still there, and still opens and reads
        cap = len(old) + 200000
        buf = _in_place_buffer(old, cap)
        with zstd.device.SeekableStream(ctx, buf[GUARD:GUARD + len(old)]) as inplace:
            got = _edit(ctx, inplace, ec.identity_picks(n) + [(R, 0), (R, 1)], new_parts, True, capacity=cap, dst=buf)
            assert got["status"] == [40, n + 1]
            _nothing_written(got, old)
            assert inplace.read_records([0, n - 2])[1].cpu().numpy().tobytes() == base["parts"][n - 2]
        with zstd.device.SeekableStream(ctx, buf[GUARD:GUARD + len(old)]) as again:
            assert again.n_frames == n and again.read_records([7])[0].cpu().numpy().tobytes() == base["parts"][7]


@pytest.mark.parametrize("in_place", [False, True])
def test_capacity(zstd, contexts, base, in_place):
    ctx = contexts()
    old = base["streams"][False]
    n = base["n"]
    new_parts = base["new_parts"][:5]
    picks = ec.identity_picks(n) + [(R, j) for j in range(5)]
    want = ec.model(old, picks, base["new_frames"], base["new_parts"])
    sizes = [e[0] for e in sc.parse(want)[0]]
    middle = next(k for k in range(n + 1, n + 4) if sum(sizes[:k + 1]) - 1 >= len(old))      # (in place the capacity holds at least the old stream)
    for cap, status in ((len(want), [0, 0]), (len(want) - 1, [70, n + 4]), (sum(sizes[:middle + 1]) - 1, [70, middle])):
        buf = _in_place_buffer(old, cap) if in_place else None
        with zstd.device.SeekableStream(ctx, buf[GUARD:GUARD + len(old)] if in_place else _dev(old)) as st:
            got = _edit(ctx, st, picks, new_parts, False, capacity=cap, dst=buf)
            assert got["rc"] == 0 and got["status"] == status, (cap, got["status"])
            if status[0]:
                _nothing_written(got, old if in_place else None)
                assert st.read_records([n - 1])[0].cpu().numpy().tobytes() == base["parts"][n - 1]
            else:
                assert _stream_of(got) == want
    with zstd.device.SeekableStream(ctx, _dev(old)) as st:
        got = _edit(ctx, st, [], checksum=False, capacity=16)
        assert got["status"][0] == 70
        _nothing_written(got)


def test_record_precheck(zstd, contexts, base):
    """72 with the RECORD index, whatever position picks it"""
    ctx = contexts()
    old = base["streams"][True]
    parts = base["new_parts"][:6]
    src = b"".join(parts)
    records = _back_to_back(parts)
    records[4] = (len(src) - 10, 11)
    with zstd.device.SeekableStream(ctx, _dev(old)) as st:
        picks = [(F, 0), (R, 4), (R, 1)]
        got = _edit(ctx, st, picks, checksum=True, records=records, src_t=_dev(src), capacity=100000)
        assert got["rc"] == 0 and got["status"] == [72, 4]
        _nothing_written(got)
        with pytest.raises(zstd.ZstdError, match="record 4"):
            st.edit(picks, _dev(src), records)
        got = _edit(ctx, st, picks, checksum=True, records=_back_to_back(parts), src_t=_dev(src), max_record=len(parts[4]) - 1, capacity=100000)
        assert got["status"][0] == 72
        _nothing_written(got)


def test_host_refusals(zstd, contexts, base):
    from zstandard_amd import _lib
    ctx = contexts()
    old = base["streams"][True]
    n = base["n"]
    parts = base["new_parts"][:3]
    with zstd.device.SeekableStream(ctx, _dev(old)) as st:
        got = _edit(ctx, st, [(F, 0), (F, n)], parts, True, capacity=100000)
        _refused(got, _lib.ERR_SIZE_MISMATCH)
        assert "position 1" in got["message"] and str(n) in got["message"]
        got = _edit(ctx, st, [(R, 0), (F, 2), (R, 3)], parts, True, capacity=100000)
        _refused(got, _lib.ERR_SIZE_MISMATCH)
        assert "position 2" in got["message"]
        _refused(_edit(ctx, st, [(F, 0)], parts, True, flags=0, capacity=100000), _lib.ERR_UNSUPPORTED)
        _refused(_edit(ctx, st, [(2, 0)], parts, True, capacity=100000), _lib.ERR_UNSUPPORTED)
        assert ctx.L.zhip_seekable_edit_bound(st.handle, None, 0, 0, 0) == 0, "the flag must be the stream's"
        with pytest.raises(zstd.ZstdError, match="position 1"):
            st.reorder([0, n])
        with pytest.raises(zstd.ZstdError, match="position 0"):
            st.edit([(R, 0)])
    _refused(_edit(ctx, None, [(R, 0), (F, 0)], parts, True, capacity=100000), _lib.ERR_UNSUPPORTED)
    with pytest.raises(zstd.ZstdError, match="position 1"):
        ctx.seekable_edit([(R, 0), (F, 0)], _dev(b"".join(parts)), _back_to_back(parts))
    # a destination that overlaps the old stream and is not the append form: at its base with other picks, inside it, ending inside it
    import torch
    cap = len(old) + 100000
    buf = _in_place_buffer(old, cap)
    was = buf.cpu().numpy()
    size = torch.full((1,), -1, dtype=torch.int64, device="cuda"); status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    base_ptr = buf.data_ptr() + GUARD
    with zstd.device.SeekableStream(ctx, buf[GUARD:GUARD + len(old)]) as st:
        for picks, ptr, room in ((ec.identity_picks(n)[1:], base_ptr, cap), ([(F, 1), (F, 0)] + ec.identity_picks(n)[2:], base_ptr, cap), (ec.identity_picks(n - 1), base_ptr, cap),
                                 (ec.identity_picks(n), base_ptr + 16, cap - 16), (ec.identity_picks(n), base_ptr - 16, 32), (ec.identity_picks(n), base_ptr + len(old) - 1, 100)):
            pk = np.array(picks, dtype=np.uint32)
            rc = ctx.L.zhip_seekable_edit_device(ctx.ctx, st.handle, pk.ctypes.data, len(pk), None, 0, None, 0, 0, 0, 1, ptr, room, size.data_ptr(), status.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream)
            assert rc == _lib.ERR_UNSUPPORTED and "overlaps" in ctx.L.zhip_last_error().decode()
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [-1, -1] and int(size[0]) == -1 and np.array_equal(buf.cpu().numpy(), was), "nothing queued, nothing written"
        # a destination that ends where the old stream begins is none of these
        rc = ctx.L.zhip_seekable_edit_device(ctx.ctx, st.handle, None, 0, None, 0, None, 0, 0, 0, 1, buf.data_ptr() + GUARD - 17, 17, size.data_ptr(), status.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0 and status.cpu().tolist() == [0, 0] and int(size[0]) == 17 and buf[GUARD - 17:GUARD].cpu().numpy().tobytes() == sc.table([], True)


# ---------------------------------------------------------------------------------------------------- 7. stream order
def test_stream_order(zstd, contexts, base):
    """source and record table are written by work queued on a non-default stream just before the call; the result is opened on that stream"""
    import torch
    ctx = contexts()
    old = base["streams"][True]
    n = base["n"]
    parts = base["new_parts"]
    src = b"".join(parts)
    records = _back_to_back(parts)
    picks = ec.identity_picks(n)[::2] + [(R, j) for j in range(40)]
    want = ec.model(old, picks, base["new_frames"], parts)
    staged_src, staged_table = _dev(src), _table(records)
    src_t = torch.zeros(len(src), dtype=torch.uint8, device="cuda")
    table = torch.full((40, 2), 1 << 40, dtype=torch.int64, device="cuda")    # what a call that ran too early would read: every record outside the source
    st = zstd.device.SeekableStream(ctx, _dev(old))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        src_t.copy_(staged_src, non_blocking=True)
        table.copy_(staged_table + 0, non_blocking=True)
        out = st.edit(picks, src_t, table, max_content_bytes=len(src) + 5, max_record_bytes=131073, stream=s)
        with zstd.device.SeekableStream(ctx, out, stream=s) as opened:
            pick = [len(picks) - 1, 0, 170, 170]
            got = [v.cpu().numpy().tobytes() for v in opened.read_records(pick, stream=s)]
    st.close()
    assert out.cpu().numpy().tobytes() == want
    contents = _contents(base, picks, parts)
    assert got == [contents[p] for p in pick]


# ---------------------------------------------------------------------------------------------------- 8. host bytes
def test_host_bytes_layer(zstd, checker, base):
    import zstandard_amd.seekable as seekable
    small = seekable.compress_records(base["parts"][:20], checksum=True)
    new = base["new_parts"][:4]
    frames = [checker.compress(p, 3, reflib.DEFAULT_FLAGS) for p in base["parts"][:20]]
    assert small == sc.stream_of(frames, base["parts"][:20], True)
    assert seekable.append_records(small, new) == ec.model(small, ec.identity_picks(20) + [(R, j) for j in range(4)], base["new_frames"], base["new_parts"])
    picks = [(F, 19), (R, 3), (F, 0), (F, 19)]
    assert seekable.edit(small, picks, new) == ec.model(small, picks, base["new_frames"], base["new_parts"])
    assert seekable.edit(small, [(F, 2)]) == ec.model(small, [(F, 2)])
    wave = seekable.append_records(small, new, match_finder="wave")
    assert wave[:sc.parse(small)[2]] == small[:sc.parse(small)[2]], "the kept frames are the old stream's"
    assert seekable.decompress_records(wave, [20, 23, 0]) == [new[0], new[3], base["parts"][0]]
    with pytest.raises(zstd.ZstdError):
        seekable.edit(b"", [])
