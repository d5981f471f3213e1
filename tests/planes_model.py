"""The typed seekable stream ("one byte plane per frame", include/zstd_hip.h) restated in numpy, independent of the library: the split and join of the bytes,
the marker and the table, the planar ranges and join jobs a user range becomes. tests/test_emu_seekable_typed.py and tests/test_gpu_seekable_typed.py check the
kernels and the calls against this."""
import struct

import numpy as np

from tests import seekable_cases as sc

PLANES_MAGIC, TAG, VERSION, MARKER_BYTES, XXH_EMPTY = 0x184D2A5D, b"ZHPL", 1, 24, 0x51D8E999
GROUP_SIZES = [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025]      # the 16-element vector body against its tail, a wave's 1 024-element tile against its tail


def _u8(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).reshape(-1)


def groups(n_elements, frame_size):
    """[(first element, elements)] of the groups"""
    return [(at, min(frame_size, n_elements - at)) for at in range(0, n_elements, frame_size)]


def split(data, k, frame_size):
    """interleaved bytes -> planar bytes: group g's plane p at g * k * frame_size + p * e"""
    a = _u8(data)
    assert a.size % k == 0
    out = np.empty_like(a)
    for at, e in groups(a.size // k, frame_size):
        out[at * k:(at + e) * k] = a[at * k:(at + e) * k].reshape(e, k).T.reshape(-1)
    return out


def join(planar, k, frame_size):
    a = _u8(planar)
    assert a.size % k == 0
    out = np.empty_like(a)
    for at, e in groups(a.size // k, frame_size):
        out[at * k:(at + e) * k] = a[at * k:(at + e) * k].reshape(k, e).T.reshape(-1)
    return out


elements_to_planes, planes_to_elements = split, join


def planes(data, k, frame_size):
    """the content of the plane frames, in frame order"""
    a = _u8(data)
    out = []
    for at, e in groups(a.size // k, frame_size):
        g = a[at * k:(at + e) * k].reshape(e, k)
        out += [g[:, p].tobytes() for p in range(k)]
    return out


def marker(k, frame_size):
    return struct.pack("<II4sIII", PLANES_MAGIC, 16, TAG, VERSION, k, frame_size)


def stream_of(frames, contents, k, frame_size, checksum):
    """plane frames (compressed) and their contents -> the typed stream: frames, marker, table with the marker's entry"""
    entries = [(len(f), len(c), sc.xxh64(c) & 0xFFFFFFFF) for f, c in zip(frames, contents)] + [(MARKER_BYTES, 0, XXH_EMPTY)]
    return b"".join(frames) + marker(k, frame_size) + sc.table(entries, checksum)


def plan(n_elements, k, frame_size, offset, length):
    """one user range (bytes of the interleaved content) -> (planar ranges [(planar content offset, length)], jobs [(elements, head trim, tail trim)]): a
    run of whole groups is one planar range, a partly covered group k of them; one job per group"""
    if not length:
        return [], []
    e0, e1 = offset // k, (offset + length - 1) // k
    ranges, jobs, run = [], [], False
    for at, e in groups(n_elements, frame_size):
        lo, hi = max(e0, at), min(e1 + 1, at + e)
        if lo >= hi:
            continue
        jobs.append((hi - lo, offset - e0 * k if lo == e0 else 0, (e1 + 1) * k - (offset + length) if hi == e1 + 1 else 0))
        if hi - lo == e:
            if run:
                ranges[-1] = (ranges[-1][0], ranges[-1][1] + e * k)
            else:
                ranges.append((at * k, e * k))
            run = True
        else:
            ranges += [(at * k + p * e + (lo - at), hi - lo) for p in range(k)]
            run = False
    return ranges, jobs
