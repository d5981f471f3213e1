"""Chains of xor-with-base links (include/zstd_hip.h, "CHAINS of xor-with-base streams") restated in numpy, independent of the library:
versions v0, v1, ... of one tensor, every version stored against its PREDECESSOR -- v0 as an unfiltered typed stream (or held by the reader as the base),
v(i) as the planes of v(i) ^ v(i-1) -- and version n read back as the XOR of all links, joined once, XORed with the base where there is one.
tests/test_emu_seekable_chain.py and tests/test_gpu_seekable_chain.py check the kernel and the calls against this."""
import numpy as np

from tests import planes_model as pm
from tests import xor_model as xm

CHAIN_MAX = 16
LINK_COUNTS = [1, 2, 3, 16]


def versions(k, n_elements, n, seed=0):
    """n + 1 versions of one tensor as byte arrays: v0 random, v(i) = v(i-1) with the low 3 bits of every element's byte 0 redrawn (xm.base_of's "low_bits")"""
    out = [xm.source(k, n_elements, seed=seed)]
    for i in range(n):
        out.append(xm.base_of("low_bits", out[-1], k, seed=seed + 31 * (i + 1)))
    return out


def link_sources(vs, full):
    """the chain that reads vs[-1] -> ([(data, base or None)] per link, oldest first, and the reader's base or None). full: v0 is link 0, an unfiltered
    stream; else v0 is the reader's base and link 0 is v1 ^ v0"""
    links = [(vs[0], None)] if full else []
    links += [(vs[i], vs[i - 1]) for i in range(1, len(vs))]
    return links, (None if full else vs[0])


def planar_of(data, base, k, frame_size):
    """a link's planar content"""
    return pm.split(data, k, frame_size) if base is None else xm.split(data, base, k, frame_size)


def join_chain(planars, base, k, frame_size):
    """the XOR of the links' planar buffers, joined, XORed with the base where there is one"""
    acc = np.zeros_like(xm._u8(planars[0]))
    for p in planars:
        acc = acc ^ xm._u8(p)
    out = pm.join(acc, k, frame_size)
    return out if base is None else out ^ xm._u8(base)


def random_planars(k, n_elements, n_links, seed=0):
    rng = np.random.default_rng(4000 + seed)
    return [rng.integers(0, 256, n_elements * k, dtype=np.uint8) for _ in range(n_links)]


def drifting_versions(k_dtype, n_elements, steps, rel, seed):
    """steps + 1 versions as bytes in the storage type ("bf16" or "fp32"): w0 ~ N(0, 1) * 0.02 in fp32, w(i) = w(i-1) + N(0, 1) * 0.02 * rel kept in fp32,
    every version rounded to the storage type with torch on the CPU (xm.checkpoint_pair, continued)"""
    import torch
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal(n_elements) * 0.02).astype(np.float32)
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[k_dtype]
    out = []
    for i in range(steps + 1):
        if i:
            w = (w + rng.standard_normal(n_elements) * 0.02 * rel).astype(np.float32)
        out.append(torch.from_numpy(w).to(dt).contiguous().view(torch.uint8).numpy().tobytes())
    return out
