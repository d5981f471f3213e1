"""The zstd seekable format for host bytes: ``compress`` cuts the data into frames of ``frame_size`` bytes, compresses them as ONE batch on the GPU and
appends the seek table; ``decompress`` reads any byte range of such a stream by decoding only the frames that cover it, ``decompress_ranges`` many ranges as one batch. The streams are ordinary zstd:
``zstd -d`` and ``ZstdDecompressor`` decompress them whole (the table is a skippable frame). Built on ``device.DeviceBatchContext.seekable_compress`` and
``device.SeekableStream``; the data crosses the link once each way. ``compress_records`` / ``decompress_records`` do the same for a list of records of any
sizes: one frame per record, read back by index; ``append_records`` / ``edit`` make a new stream out of an old one's frames and new records.

``compress(..., element_size=2 | 4 | 8)`` writes a TYPED stream for a tensor's bytes: groups of ``frame_size`` elements, one frame per byte position of the
elements ("byte planes"), and a marker frame that says so. ``decompress`` / ``decompress_ranges`` recognise it and return the elements; any other zstd decoder
returns the planar bytes, which ``planes_to_elements`` puts back in order (``elements_to_planes`` is its inverse) -- numpy on the host, no GPU.

``filter="delta"`` (with an element_size) is for INTEGER tensors whose neighbours are close -- offsets, sorted ids, timestamps, counters, running sums: per
group the planes are those of the differences of neighbouring elements mod 2^(8 * element_size), 13-34 % smaller streams on such data (floats gain nothing).
The marker names the filter, so the readers return the elements as before; ``elements_to_planes`` / ``planes_to_elements`` take the same ``filter``."""
import torch

from .backend_hip import ZstdError
from .device import DeviceBatchContext, SeekableStream


def _to_device(data):
    raw = bytes(data)
    if not raw:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def _filter_code(filter):
    if filter not in (None, "delta"):
        raise ValueError("filter must be None or \"delta\"")
    return 1 if filter == "delta" else 0


def elements_to_planes(data, element_size, frame_size, filter=None):
    """bytes of elements -> the planar content of the typed stream ``compress(data, frame_size=frame_size, element_size=element_size, filter=filter)`` writes:
    per group of frame_size elements, byte 0 of every element, then byte 1 of every element, ... -- under filter="delta" of the group's differences
    d[0] = x[0], d[i] = x[i] - x[i - 1] mod 2^(8 * element_size), the elements read as unsigned little-endian integers. Returns bytes."""
    import numpy as np
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    if element_size not in (2, 4, 8) or a.size % element_size or frame_size < 1:
        raise ValueError("element_size must be 2, 4 or 8, the data whole elements and frame_size at least 1")
    delta = _filter_code(filter)
    out, step = np.empty_like(a), frame_size * element_size
    for at in range(0, a.size, step):
        g = a[at:at + step]
        if delta:
            x = g.view("<u%d" % element_size)
            g = np.diff(x, prepend=x.dtype.type(0)).view(np.uint8)
        out[at:at + g.size] = g.reshape(-1, element_size).T.reshape(-1)
    return out.tobytes()


def planes_to_elements(raw, element_size, frame_size, filter=None):
    """the planar content of a typed stream, as any zstd decoder returns it (``zstd -d``, ``SeekableStream(..., raw=True).read()``), -> the elements' bytes
    (filter: the stream's, ``SeekableStream.filter`` -- under "delta" every group's inclusive prefix sum mod 2^(8 * element_size))"""
    import numpy as np
    a = np.frombuffer(bytes(raw), dtype=np.uint8)
    if element_size not in (2, 4, 8) or a.size % element_size or frame_size < 1:
        raise ValueError("element_size must be 2, 4 or 8, the data whole elements and frame_size at least 1")
    delta = _filter_code(filter)
    out, step = np.empty_like(a), frame_size * element_size
    for at in range(0, a.size, step):
        g = a[at:at + step]
        e = np.ascontiguousarray(g.reshape(element_size, -1).T).reshape(-1)
        if delta:
            d = e.view("<u%d" % element_size)
            e = np.cumsum(d, dtype=d.dtype).view(np.uint8)
        out[at:at + g.size] = e
    return out.tobytes()


def compress(data, level=3, frame_size=131072, checksum=False, match_finder="libzstd", element_size=1, filter=None, **ctx_kw):
    """data -> a seekable stream (bytes). match_finder: "libzstd" (frames byte for byte libzstd's) or "wave" (DeviceBatchContext.set_match_finder: valid zstd,
    not libzstd's bytes; frame_size at most 131 072) or "none" (no match search: every frame is libzstd's literals-only frame of its content, for NUMERIC
    TENSORS -- with element_size 2, 4 or 8 the fastest compress path, and streams the size of level 3's or up to 13 % smaller on float data; "on data with real
    repetition they lose badly: the int64 sums here, and any text", 1.9 x on int64 running sums; frame_size at most 131 072 bytes of a plane) or "auto" ("none" or "libzstd" chosen per frame by a classify kernel -- per PLANE frame of a typed stream, whose planes want different finders: every frame is byte for byte one of the two; any frame_size, a frame above 131 072 bytes goes to the search). element_size 2, 4 or 8: a typed stream -- data is elements of that many bytes, frame_size counts the
    elements of a group (see the module); filter None or "delta": the filter of a typed stream (see the module; with element_size 1 a ZstdError). ctx_kw: what DeviceBatchContext takes (dict_data, write_checksum, window_log, ...). Raises ZstdError."""
    ctx = DeviceBatchContext(level=level, match_finder=match_finder, **ctx_kw)
    try:
        return ctx.seekable_compress(_to_device(data), frame_size=frame_size, checksum=checksum, element_size=element_size, filter=filter).cpu().numpy().tobytes()
    finally:
        ctx.close()


def decompress(data, offset=0, length=None, **ctx_kw):
    """content bytes [offset, offset + length) of a seekable stream (length None: to the end); of a typed stream, the elements' bytes. Raises ZstdError for
    a stream without a valid seek table, a range outside the content, or a frame that fails."""
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
    """the content bytes of every (offset, length) of `ranges` as a list of bytes: ONE decode batch over the frames the ranges touch, each decoded once
    (of a typed stream: the elements' bytes, every plane frame a range's groups need).
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
    match_finder: as in ``compress`` (records of at most 131 072 bytes under "wave" and "none"; "none" is for records of numeric data, not text; "auto" chooses between "none" and "libzstd" per record). ctx_kw: what DeviceBatchContext takes. Raises ZstdError."""
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
    may be picked any number of times; the table has checksums exactly when that of `data` has. match_finder: as in ``compress_records``, for the records
    compressed here (kept frames are not looked at). Raises ZstdError."""
    if records is None:
        return _edited(data, [], level, match_finder, ctx_kw, lambda st, src, table: st.edit(picks))
    return _edited(data, records, level, match_finder, ctx_kw, lambda st, src, table: st.edit(picks, src, table))


def append_records(data, records, level=3, match_finder="libzstd", **ctx_kw):
    """a seekable stream (bytes) with one more frame per record of `records` (a list of bytes) behind its own: ``edit`` with every frame kept
    (match_finder: as in ``compress_records``). Raises ZstdError."""
    return _edited(data, records, level, match_finder, ctx_kw, lambda st, src, table: st.append_records(src, table))
