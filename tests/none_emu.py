"""The literals-only kernel (match_finder="none") on the host emulator (tests/emu/emu_none_finder.cpp): builds the emulator program and runs batches through it.
Used by tests/test_emu_none_finder.py."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PARAM_NAMES = ("window_log", "chain_log", "hash_log", "search_log", "min_match", "target_length", "strategy")


def build(out_dir):
    """compiles zhemu.cpp + emu_none_finder.cpp into out_dir and returns the loaded library"""
    out = os.path.join(str(out_dir), "libzhip_emu_none_finder.so")
    d = os.path.join(HERE, "emu")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + d, "-w", "-o", out, os.path.join(d, "zhemu.cpp"), os.path.join(d, "emu_none_finder.cpp")])
    lib = C.CDLL(out)
    lib.emu_none_frames.restype = C.c_int
    lib.emu_none_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32,
                                    C.c_int, C.c_uint32, C.c_void_p]
    lib.emu_none_bound.restype = C.c_uint64
    lib.emu_none_bound.argtypes = [C.c_uint64]
    lib.emu_none_plan.restype = None
    lib.emu_none_plan.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_void_p]
    return lib


def plan(lib, n, num_cu=256, e2_per_cu=14, echunk=0):
    """ze_none_plan's (chunk, grid, metaBytes)"""
    out = np.zeros(3, dtype=np.uint64)
    lib.emu_none_plan(n, num_cu, e2_per_cu, echunk, out.ctypes.data)
    return tuple(int(x) for x in out)


def frames(lib, raws, level=3, checksum=False, content_size=True, magicless=False, dictionary=False, path="none", blocks=3, echunk=0, **params):
    """one batch through the literals-only kernel and the trailer kernel under emulation (path "none"), or through the sequence loader with empty lists, the entropy
    kernel and the trailer kernel (path "sequences": what zhip_compress_sequences_device does for count 0). Every source lies in the batch's buffer back to back, the
    last one ending at the buffer's end; every destination is a slot of exactly zhip_compress_bound bytes, back to back, and that is the capacity the kernel is
    told. Returns (frames, statuses, modes); raises RuntimeError where the call as a whole is refused."""
    n = len(raws)
    lens = np.array([len(r) for r in raws], dtype=np.uint64)
    caps = np.array([lib.emu_none_bound(len(r)) for r in raws], dtype=np.uint64)          # exactly zhip_compress_bound, by the product's own function
    ssegs = np.zeros((n, 2), dtype=np.uint64); ssegs[:, 1] = lens; ssegs[1:, 0] = np.cumsum(lens)[:-1]
    dsegs = np.zeros((n, 2), dtype=np.uint64); dsegs[:, 1] = caps; dsegs[1:, 0] = np.cumsum(caps)[:-1]
    joined = b"".join(raws)
    src = np.frombuffer(joined, dtype=np.uint8).copy() if joined else np.zeros(1, dtype=np.uint8)
    dst = np.zeros(int(caps.sum()), dtype=np.uint8)
    sizes = np.zeros(n, dtype=np.uint64); st = np.full(n, -1, dtype=np.int32)
    assert set(params) <= set(PARAM_NAMES), params
    ov = np.array([params.get(k, 0) for k in PARAM_NAMES], dtype=np.int32)
    meta = np.zeros((n, 4), dtype=np.uint32)
    flags = (1 if content_size else 0) | (2 if checksum else 0) | (4 if magicless else 0) | (8 if dictionary else 0)
    rc = lib.emu_none_frames(src.ctypes.data, ssegs.ctypes.data, n, dst.ctypes.data, dsegs.ctypes.data, sizes.ctypes.data, st.ctypes.data, level, ov.ctypes.data,
                             flags, blocks, {"sequences": 0, "none": 1}[path], echunk, meta.ctypes.data)
    if rc:
        raise RuntimeError("the call is refused (%d)" % rc)
    out = [dst[int(dsegs[i, 0]): int(dsegs[i, 0] + sizes[i])].tobytes() for i in range(n)]
    return out, st.tolist(), meta[:, 2].tolist()
