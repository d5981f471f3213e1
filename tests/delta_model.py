"""The delta filter of typed seekable streams (include/zstd_hip.h, "filters") restated in numpy, independent of the library: numpy's diff and
cumsum in the element's unsigned dtype per group, then the planes of tests/planes_model.py; the marker with its filter bits, the tile offsets of the delta
join, and the planar ranges and jobs a user range becomes under the filter. tests/test_emu_seekable_delta.py and tests/test_gpu_seekable_delta.py check the
kernels and the calls against this."""
import struct

import numpy as np

from tests import planes_model as pm
from tests import seekable_cases as sc

NONE, DELTA = 0, 1
TILE = 1024
DTYPES = {2: np.dtype("<u2"), 4: np.dtype("<u4"), 8: np.dtype("<u8")}
# the 16-element body against its tail, a wave's tile against its tail, and groups of two and three whole tiles with a tail behind them (the tile offsets)
GROUP_SIZES = [1, 15, 16, 17, 1023, 1024, 1025, 2067, 3077]
LAST_GROUPS = [1, 15, 17]


def _u8(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).reshape(-1)


def delta(data, k, frame_size):
    """elements' bytes -> the bytes of d: per group d[0] = x[0], d[i] = x[i] - x[i - 1] mod 2^(8k)"""
    x = _u8(data).view(DTYPES[k])
    out = np.empty_like(x)
    for at, e in pm.groups(x.size, frame_size):
        out[at:at + e] = np.diff(x[at:at + e], prepend=x.dtype.type(0))
    return out.view(np.uint8)


def undelta(data, k, frame_size):
    d = _u8(data).view(DTYPES[k])
    out = np.empty_like(d)
    for at, e in pm.groups(d.size, frame_size):
        out[at:at + e] = np.cumsum(d[at:at + e], dtype=d.dtype)
    return out.view(np.uint8)


def split(data, k, frame_size):
    """elements' bytes -> the planar content of the filtered stream"""
    return pm.split(delta(data, k, frame_size), k, frame_size)


def join(planar, k, frame_size):
    return undelta(pm.join(planar, k, frame_size), k, frame_size)


def planes(data, k, frame_size):
    return pm.planes(delta(data, k, frame_size), k, frame_size)


def marker(k, frame_size, filt=DELTA):
    return struct.pack("<II4sIII", pm.PLANES_MAGIC, 16, pm.TAG, pm.VERSION, k | (filt << 8), frame_size)


def stream_of(frames, contents, k, frame_size, checksum, filt=DELTA):
    entries = [(len(f), len(c), sc.xxh64(c) & 0xFFFFFFFF) for f, c in zip(frames, contents)] + [(pm.MARKER_BYTES, 0, pm.XXH_EMPTY)]
    return b"".join(frames) + marker(k, frame_size, filt) + sc.table(entries, checksum)


def tile_offsets(data, k, frame_size):
    """what the tile-sums area holds behind a whole-buffer join: per tile of 1 024 elements of a group the sum, mod 2^64, of the group's DIFFERENCES in front of it"""
    d = delta(data, k, frame_size).view(DTYPES[k]).astype(np.uint64)
    out = []
    for at, e in pm.groups(d.size, frame_size):           # (every group has the tiles of a full one: behind a shorter last group's elements they are empty)
        sums = [int(d[at + t:at + min(t + TILE, e)].sum(dtype=np.uint64)) if t < e else 0 for t in range(0, frame_size, TILE)]
        run = 0
        for s in sums:
            out.append(run)
            run = (run + s) & 0xFFFFFFFFFFFFFFFF
    return out


def plan(n_elements, k, frame_size, offset, length):
    """pm.plan under the filter: a group covered in part is fetched from its first element -- k planar ranges that start at the planes' starts, hi elements
    long, and a job (elements, head trim, tail trim, skip) of hi elements that skips lo"""
    if not length:
        return [], []
    e0, e1 = offset // k, (offset + length - 1) // k
    ranges, jobs, run = [], [], False
    for at, e in pm.groups(n_elements, frame_size):
        lo, hi = max(e0, at), min(e1 + 1, at + e)
        if lo >= hi:
            continue
        h, t = offset - e0 * k if lo == e0 else 0, (e1 + 1) * k - (offset + length) if hi == e1 + 1 else 0
        if hi - lo == e:
            jobs.append((e, h, t, 0))
            if run:
                ranges[-1] = (ranges[-1][0], ranges[-1][1] + e * k)
            else:
                ranges.append((at * k, e * k))
            run = True
        else:
            jobs.append((hi - at, h, t, lo - at))
            ranges += [(at * k + p * e, hi - at) for p in range(k)]
            run = False
    return ranges, jobs


def values(kind, k, n_elements, frame_size, seed=0):
    """the test sources, as bytes of n_elements elements: "random" full-range (every subtraction wraps), "constant", "increasing", "ones" (all bits set, then
    one 0), "carry" (every difference 2^(8k) - 1: each tile sum carries through every byte)"""
    dt = DTYPES[k]
    top = (1 << (8 * k)) - 1
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, n_elements * k, dtype=np.uint8)
    if kind == "constant":
        x = np.full(n_elements, 0xA1B2C3D4E5F60718 & top, dtype=dt)
    elif kind == "increasing":
        x = (np.arange(n_elements, dtype=np.uint64) * 3 + 250).astype(dt)
    elif kind == "ones":
        x = np.full(n_elements, top, dtype=dt); x[-1] = 0
    elif kind == "carry":
        return undelta(np.full(n_elements * k, 0xFF, dtype=np.uint8), k, frame_size).copy()
    else:
        raise ValueError(kind)
    return x.view(np.uint8).copy()


KINDS = ["random", "constant", "increasing", "ones", "carry"]
