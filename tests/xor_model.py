"""The xor-with-base filter of typed seekable streams (include/zstd_hip.h, "ZHIP_FILTER_XOR_BASE") restated in numpy, independent of the
library: the bytewise XOR of the elements with a base of the same size, then the planes of tests/planes_model.py; the marker with filter 4 and the stream
layout (tests/delta_model.py's, the filter a parameter there); the content offsets a user range's jobs carry. tests/test_emu_seekable_xor_base.py and
tests/test_gpu_seekable_xor_base.py check the kernels and the calls against this."""
import numpy as np

from tests import delta_model as dm
from tests import planes_model as pm

NONE, DELTA, XOR_BASE = 0, 1, 4
# the 16-element body against its tail, a wave's 1 024-element tile against its tail, a group of two whole tiles and a tail
GROUP_SIZES = [1, 15, 16, 17, 1023, 1024, 1025, 2500]
LAST_GROUPS = [1, 15, 17]                 # the short last group behind two full ones (as far as a group holds them)
BASES = ["same", "random", "low_bits"]


def _u8(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).reshape(-1)


def xor(data, base):
    a, b = _u8(data), _u8(base)
    assert a.size == b.size
    return a ^ b


def split(data, base, k, frame_size):
    """elements' bytes and the base's -> the planar content of the filtered stream"""
    return pm.split(xor(data, base), k, frame_size)


def join(planar, base, k, frame_size):
    return xor(pm.join(planar, k, frame_size), base)


def planes(data, base, k, frame_size):
    return pm.planes(xor(data, base), k, frame_size)


def marker(k, frame_size):
    return dm.marker(k, frame_size, XOR_BASE)


def stream_of(frames, contents, k, frame_size, checksum):
    return dm.stream_of(frames, contents, k, frame_size, checksum, XOR_BASE)


def plan(n_elements, k, frame_size, offset, length):
    """pm.plan (the filter changes no planar range and no job), and per job the content offset of its first element: where its base bytes stand"""
    ranges, jobs = pm.plan(n_elements, k, frame_size, offset, length)
    content = []
    if length:
        e0, e1 = offset // k, (offset + length - 1) // k
        content = [max(e0, at) * k for at, e in pm.groups(n_elements, frame_size) if max(e0, at) < min(e1 + 1, at + e)]
    return ranges, jobs, content


def shapes(m):
    """two full groups of m and a short last group -> the element counts"""
    return sorted({2 * m + min(last, m) for last in LAST_GROUPS})


def source(k, n_elements, seed=0):
    return np.random.default_rng(seed).integers(0, 256, n_elements * k, dtype=np.uint8)


def base_of(kind, src, k, seed=0):
    """"same": the source (all-zero planes); "random"; "low_bits": the source with the low 3 bits of every element's byte 0 redrawn (what versions look like)"""
    if kind == "same":
        return src.copy()
    rng = np.random.default_rng(1000 + seed)
    if kind == "random":
        return rng.integers(0, 256, src.size, dtype=np.uint8)
    if kind == "low_bits":
        b = src.copy()
        b[::k] ^= rng.integers(0, 8, src.size // k, dtype=np.uint8)
        return b
    raise ValueError(kind)


def checkpoint_pair(k_dtype, n_elements, rel, seed):
    """(w0, w1) as bytes in the storage type ("bf16" or "fp32"): w0 ~ N(0, 1) * 0.02 in fp32, w1 = w0 + N(0, 1) * 0.02 * rel, both rounded with torch on the CPU"""
    import torch
    rng = np.random.default_rng(seed)
    w0 = (rng.standard_normal(n_elements) * 0.02).astype(np.float32)
    w1 = (w0 + rng.standard_normal(n_elements) * 0.02 * rel).astype(np.float32)
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[k_dtype]
    return tuple(torch.from_numpy(w).to(dt).contiguous().view(torch.uint8).numpy().tobytes() for w in (w0, w1))
