"""The zstd seekable format for host bytes: ``compress`` cuts the data into frames of ``frame_size`` bytes, compresses them as ONE batch on the GPU and
appends the seek table; ``decompress`` reads any byte range of such a stream by decoding only the frames that cover it, ``decompress_ranges`` many ranges as one batch. The streams are ordinary zstd:
``zstd -d`` and ``ZstdDecompressor`` decompress them whole (the table is a skippable frame). Built on ``device.DeviceBatchContext.seekable_compress`` and
``device.SeekableStream``; the data crosses the link once each way. ``compress_records`` / ``decompress_records`` do the same for a list of records of any
sizes: one frame per record, read back by index; ``append_records`` / ``edit`` make a new stream out of an old one's frames and new records."""
import torch

from .backend_hip import ZstdError
from .device import DeviceBatchContext, SeekableStream


def _to_device(data):
    raw = bytes(data)
    if not raw:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def compress(data, level=3, frame_size=131072, checksum=False, match_finder="libzstd", **ctx_kw):
    """data -> a seekable stream (bytes). match_finder: "libzstd" (frames byte for byte libzstd's) or "wave" (DeviceBatchContext.set_match_finder: valid zstd,
    not libzstd's bytes; frame_size at most 131 072). ctx_kw: what DeviceBatchContext takes (dict_data, write_checksum, window_log, ...). Raises ZstdError."""
    ctx = DeviceBatchContext(level=level, match_finder=match_finder, **ctx_kw)
    try:
        return ctx.seekable_compress(_to_device(data), frame_size=frame_size, checksum=checksum).cpu().numpy().tobytes()
    finally:
        ctx.close()


def decompress(data, offset=0, length=None, **ctx_kw):
    """content bytes [offset, offset + length) of a seekable stream (length None: to the end). Raises ZstdError for a stream without a valid seek table,
    a range outside the content, or a frame that fails."""
    if len(data) == 0:
        raise ZstdError("not a seekable stream: empty input")
    ctx = DeviceBatchContext(**ctx_kw)
    try:
        st = SeekableStream(ctx, _to_device(data))
        try:
            return st.read(offset, length).cpu().numpy().tobytes()
        finally:
            st.close()
    finally:
        ctx.close()


def decompress_ranges(data, ranges, **ctx_kw):
    """the content bytes of every (offset, length) of `ranges` as a list of bytes: ONE decode batch over the frames the ranges touch, each decoded once.
    Raises ZstdError as ``decompress`` does; a failing frame's error names the lowest range that needs it."""
    if len(data) == 0:
        raise ZstdError("not a seekable stream: empty input")
    ctx = DeviceBatchContext(**ctx_kw)
    try:
        st = SeekableStream(ctx, _to_device(data))
        try:
            views = st.read_ranges(ranges)
            if not views:
                return []
            host = torch.cat(views).cpu().numpy().tobytes()                 # (the views lie back to back in call order: one copy over the link)
            out, at = [], 0
            for v in views:
                out.append(host[at:at + v.numel()]); at += v.numel()
            return out
        finally:
            st.close()
    finally:
        ctx.close()


def compress_records(records, level=3, checksum=False, match_finder="libzstd", **ctx_kw):
    """a list of bytes -> a seekable stream (bytes) with ONE frame per record, compressed as one batch; ``decompress_records`` reads records back by index.
    match_finder: as in ``compress`` (records of at most 131 072 bytes under "wave"). ctx_kw: what DeviceBatchContext takes. Raises ZstdError."""
    raws = [bytes(r) for r in records]
    table, at = [], 0
    for r in raws:
        table.append((at, len(r))); at += len(r)
    ctx = DeviceBatchContext(level=level, match_finder=match_finder, **ctx_kw)
    try:
        return ctx.seekable_compress_records(_to_device(b"".join(raws)), table, checksum=checksum).cpu().numpy().tobytes()
    finally:
        ctx.close()


def decompress_records(data, indices, **ctx_kw):
    """the records (frames) of a seekable stream named by `indices`, in that order, as a list of bytes: ONE decode batch, each distinct frame decoded once.
    Raises ZstdError as ``decompress`` does, and for an index that is not a frame of the table."""
    if len(data) == 0:
        raise ZstdError("not a seekable stream: empty input")
    ctx = DeviceBatchContext(**ctx_kw)
    try:
        st = SeekableStream(ctx, _to_device(data))
        try:
            views = st.read_records(indices)
            if not views:
                return []
            host = torch.cat(views).cpu().numpy().tobytes()                 # (the views lie back to back in call order: one copy over the link)
            out, at = [], 0
            for v in views:
                out.append(host[at:at + v.numel()]); at += v.numel()
            return out
        finally:
            st.close()
    finally:
        ctx.close()


def _edited(data, records, level, match_finder, ctx_kw, call):
    """call(opened stream, source tensor, record table) -> the new stream's bytes"""
    if len(data) == 0:
        raise ZstdError("not a seekable stream: empty input")
    raws = [bytes(r) for r in records]
    table, at = [], 0
    for r in raws:
        table.append((at, len(r))); at += len(r)
    ctx = DeviceBatchContext(level=level, match_finder=match_finder, **ctx_kw)
    try:
        st = SeekableStream(ctx, _to_device(data))
        try:
            return call(st, _to_device(b"".join(raws)), table).cpu().numpy().tobytes()
        finally:
            st.close()
    finally:
        ctx.close()


def edit(data, picks, records=None, level=3, match_finder="libzstd", **ctx_kw):
    """a seekable stream (bytes) and a pick list -> a new seekable stream (bytes), what is kept not recompressed: picks is a sequence of (0, i) -- frame i of
    `data`, its bytes and its table entry as they are -- and (1, j) -- records[j] (a list of bytes), compressed as in ``compress_records``. A frame or a record
    may be picked any number of times; the table has checksums exactly when that of `data` has. Raises ZstdError."""
    if records is None:
        return _edited(data, [], level, match_finder, ctx_kw, lambda st, src, table: st.edit(picks))
    return _edited(data, records, level, match_finder, ctx_kw, lambda st, src, table: st.edit(picks, src, table))


def append_records(data, records, level=3, match_finder="libzstd", **ctx_kw):
    """a seekable stream (bytes) with one more frame per record of `records` (a list of bytes) behind its own: ``edit`` with every frame kept. Raises ZstdError."""
    return _edited(data, records, level, match_finder, ctx_kw, lambda st, src, table: st.append_records(src, table))
