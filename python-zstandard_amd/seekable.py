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
The marker names the filter, so the readers return the elements as before; ``elements_to_planes`` / ``planes_to_elements`` take the same ``filter``.

``base=`` (bytes of the data's size, with an element_size; the filter's name is "xor_base") is for VERSIONS of one tensor -- the next checkpoint, a fine-tune
beside its base model: the planes are those of data XOR base, bytewise, and since versions differ in the low mantissa bits and almost nowhere else the high
planes become runs of zeros (bf16 streams 2-12 x smaller than without, fp32 1.3-1.8 x). THE STREAM DOES NOT NAME ITS BASE: ``decompress`` and
``decompress_ranges`` need the same ``base=`` (without one they raise ZstdError), and with other bytes of the right size they return wrong elements and no
error. ``elements_to_planes`` / ``planes_to_elements`` take ``base=`` too.

``decompress_chain`` / ``decompress_ranges_chain`` read the LAST version through a chain of such streams, every version compressed against its predecessor:
``[compress(v0, element_size=k), compress(v1, element_size=k, base=v0), compress(v2, element_size=k, base=v1), ...]``, or the deltas alone with ``base=v0``
(``device.SeekableChain``: per link only the frames the ranges touch are decoded, one kernel XORs all links). No stream names its predecessor either."""
import torch

from .backend_hip import ZstdError
from .device import DeviceBatchContext, SeekableChain, SeekableStream


def _to_device(data):
    raw = bytes(data)
    if not raw:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def _filter_code(filter, base=None):
    """0: none, 1: delta, 4: xor with `base` (base= alone selects it, "xor_base" is its name)"""
    if base is not None:
        if filter not in (None, "xor_base"):
            raise ValueError("a base goes with filter \"xor_base\" (or no filter argument)")
        return 4
    if filter == "xor_base":
        raise ValueError("filter \"xor_base\" needs base=")
    if filter not in (None, "delta"):
        raise ValueError("filter must be None or \"delta\"")
    return 1 if filter == "delta" else 0


def _xor_base(a, base):
    import numpy as np
    b = np.frombuffer(bytes(base), dtype=np.uint8)
    if b.size != a.size:
        raise ValueError("the base has %d bytes, the data %d" % (b.size, a.size))
    return a ^ b


def elements_to_planes(data, element_size, frame_size, filter=None, base=None):
    """bytes of elements -> the planar content of the typed stream ``compress(data, frame_size=frame_size, element_size=element_size, filter=filter)`` writes:
    per group of frame_size elements, byte 0 of every element, then byte 1 of every element, ... -- under filter="delta" of the group's differences
    d[0] = x[0], d[i] = x[i] - x[i - 1] mod 2^(8 * element_size), the elements read as unsigned little-endian integers; with base (bytes of data's size; the
    filter "xor_base") of data XOR base. Returns bytes."""
    import numpy as np
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    if element_size not in (2, 4, 8) or a.size % element_size or frame_size < 1:
        raise ValueError("element_size must be 2, 4 or 8, the data whole elements and frame_size at least 1")
    code = _filter_code(filter, base)
    delta = code == 1
    if code == 4:
        a = _xor_base(a, base)
    out, step = np.empty_like(a), frame_size * element_size
    for at in range(0, a.size, step):
        g = a[at:at + step]
        if delta:
            x = g.view("<u%d" % element_size)
            g = np.diff(x, prepend=x.dtype.type(0)).view(np.uint8)
        out[at:at + g.size] = g.reshape(-1, element_size).T.reshape(-1)
    return out.tobytes()


def planes_to_elements(raw, element_size, frame_size, filter=None, base=None):
    """the planar content of a typed stream, as any zstd decoder returns it (``zstd -d``, ``SeekableStream(..., raw=True).read()``), -> the elements' bytes
    (filter: the stream's, ``SeekableStream.filter`` -- under "delta" every group's inclusive prefix sum mod 2^(8 * element_size); a stream whose filter is
    "xor_base" needs base=, the bytes it was compressed against -- other bytes of that size give wrong elements and no error)"""
    import numpy as np
    a = np.frombuffer(bytes(raw), dtype=np.uint8)
    if element_size not in (2, 4, 8) or a.size % element_size or frame_size < 1:
        raise ValueError("element_size must be 2, 4 or 8, the data whole elements and frame_size at least 1")
    code = _filter_code(filter, base)
    delta = code == 1
    out, step = np.empty_like(a), frame_size * element_size
    for at in range(0, a.size, step):
        g = a[at:at + step]
        e = np.ascontiguousarray(g.reshape(element_size, -1).T).reshape(-1)
        if delta:
            d = e.view("<u%d" % element_size)
            e = np.cumsum(d, dtype=d.dtype).view(np.uint8)
        out[at:at + g.size] = e
    if code == 4:
        out = _xor_base(out, base)
    return out.tobytes()


def compress(data, level=3, frame_size=131072, checksum=False, match_finder="libzstd", element_size=1, filter=None, base=None, **ctx_kw):
    """data -> a seekable stream (bytes). match_finder: "libzstd" (frames byte for byte libzstd's) or "wave" (DeviceBatchContext.set_match_finder: valid zstd,
    not libzstd's bytes; frame_size at most 131 072) or "none" (no match search: every frame is libzstd's literals-only frame of its content, for NUMERIC
    TENSORS -- with element_size 2, 4 or 8 the fastest compress path, and streams the size of level 3's or up to 13 % smaller on float data; "on data with real
    repetition they lose badly: the int64 sums here, and any text", 1.9 x on int64 running sums; frame_size at most 131 072 bytes of a plane) or "auto" ("none" or "libzstd" chosen per frame by a classify kernel -- per PLANE frame of a typed stream, whose planes want different finders: every frame is byte for byte one of the two; any frame_size, a frame above 131 072 bytes goes to the search). element_size 2, 4 or 8: a typed stream -- data is elements of that many bytes, frame_size counts the
    elements of a group (see the module); filter None or "delta": the filter of a typed stream (see the module; with element_size 1 a ZstdError); base: bytes of data's size, an earlier version of the tensor -- the planes are those of data XOR base (see the module: the readers need the same base, the stream does not name it). ctx_kw: what DeviceBatchContext takes (dict_data, write_checksum, window_log, ...). Raises ZstdError."""
    ctx = DeviceBatchContext(level=level, match_finder=match_finder, **ctx_kw)
    try:
        if base is not None and len(base) != len(data):
            raise ZstdError("seekable compress: the base has %d bytes, the data %d" % (len(base), len(data)))
        return ctx.seekable_compress(_to_device(data), frame_size=frame_size, checksum=checksum, element_size=element_size, filter=filter,
                                     base=None if base is None else _to_device(base)).cpu().numpy().tobytes()
    finally:
        ctx.close()


def decompress(data, offset=0, length=None, base=None, **ctx_kw):
    """content bytes [offset, offset + length) of a seekable stream (length None: to the end); of a typed stream, the elements' bytes. base: the bytes a
    stream written with ``compress(..., base=)`` was compressed against (the whole base, whatever the range; other bytes of that size give wrong elements and
    no error). Raises ZstdError for a stream without a valid seek table, a range outside the content, a frame that fails, or such a stream without its base."""
    if len(data) == 0:
        raise ZstdError("not a seekable stream: empty input")
    ctx = DeviceBatchContext(**ctx_kw)
    try:
        st = SeekableStream(ctx, _to_device(data), base=None if base is None else _to_device(base))
        try:
            return st.read(offset, length).cpu().numpy().tobytes()
        finally:
            st.close()
    finally:
        ctx.close()


def decompress_ranges(data, ranges, base=None, **ctx_kw):
    """the content bytes of every (offset, length) of `ranges` as a list of bytes: ONE decode batch over the frames the ranges touch, each decoded once
    (of a typed stream: the elements' bytes, every plane frame a range's groups need).
    base: as in ``decompress``. Raises ZstdError as ``decompress`` does; a failing frame's error names the lowest range that needs it."""
    if len(data) == 0:
        raise ZstdError("not a seekable stream: empty input")
    ctx = DeviceBatchContext(**ctx_kw)
    try:
        st = SeekableStream(ctx, _to_device(data), base=None if base is None else _to_device(base))
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


def _with_chain(streams, base, ctx_kw, call):
    streams = list(streams)
    if any(len(s) == 0 for s in streams):
        raise ZstdError("not a seekable stream: empty input")
    ctx = DeviceBatchContext(**ctx_kw)
    try:
        chain = SeekableChain(ctx, [_to_device(s) for s in streams], base=None if base is None else _to_device(base))
        try:
            return call(chain)
        finally:
            chain.close()
    finally:
        ctx.close()


def decompress_chain(streams, offset=0, length=None, base=None, **ctx_kw):
    """bytes [offset, offset + length) (length None: to the end) of the LAST version of a tensor stored as a chain of typed streams, oldest first: an
    unfiltered typed stream of the first version and then every version ``compress(..., base=)``-ed against its predecessor -- or those alone, with base= the
    bytes of the first version. 1 ... 16 streams. No stream names its predecessor: another order behind a wrong start, a foreign stream or another base
    give wrong elements and no error. Raises ZstdError as ``decompress`` does; a refusal or a failing frame names the link."""
    return _with_chain(streams, base, ctx_kw, lambda chain: chain.read(offset, length).cpu().numpy().tobytes())


def decompress_ranges_chain(streams, ranges, base=None, **ctx_kw):
    """``decompress_ranges`` through a chain (``decompress_chain``): the last version's bytes of every (offset, length), as a list of bytes"""
    def call(chain):
        views = chain.read_ranges(ranges)
        if not views:
            return []
        host = torch.cat(views).cpu().numpy().tobytes()
        out, at = [], 0
        for v in views:
            out.append(host[at:at + v.numel()]); at += v.numel()
        return out
    return _with_chain(streams, base, ctx_kw, call)


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
