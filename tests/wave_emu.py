"""The wave-parallel match finder on the host emulator (tests/emu/emu_wave_finder.cpp): builds the emulator program and runs batches through it. Shared by
tests/test_emu_wave_finder.py, tests/golden/make_wave_finder.py and tests/tools/wave_finder_ratio.py."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PARAM_NAMES = ("window_log", "chain_log", "hash_log", "search_log", "min_match", "target_length", "strategy")
SEQ_STRIDE = 131072 // 4 + 8


def build(out_dir):
    """compiles zhemu.cpp + emu_wave_finder.cpp into out_dir and returns the loaded library"""
    out = os.path.join(str(out_dir), "libzhip_emu_wave_finder.so")
    d = os.path.join(HERE, "emu")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + d, "-w", "-o", out, os.path.join(d, "zhemu.cpp"), os.path.join(d, "emu_wave_finder.cpp")])
    lib = C.CDLL(out)
    lib.emu_wave_frames.restype = C.c_int
    lib.emu_wave_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32,
                                    C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
    return lib


def unpack(q):
    """packed sequences -> [(litLength, matchLength, offBase)]"""
    q = np.asarray(q, dtype=np.uint64)
    ofb = (q & np.uint64(0xFFFFFFF)).astype(np.int64); ll = ((q >> np.uint64(28)) & np.uint64(0x3FFFF)).astype(np.int64); ml = (q >> np.uint64(46)).astype(np.int64)
    return list(zip(ll.tolist(), ml.tolist(), ofb.tolist()))


def frames(lib, raws, level=3, checksum=False, content_size=True, finder="wave", hlog=12, want_seqs=False, blocks=3, **params):
    """one batch through the match kernel (the wave finder's, or the default dispatch's lane-serial one), the entropy kernel and the trailer kernel under emulation.
    Every source lies in the batch's buffer back to back, the last one ending at the buffer's end. Returns (frames, statuses) or, with want_seqs,
    (frames, statuses, sequence lists, modes); raises RuntimeError where the call as a whole is refused."""
    n = len(raws)
    lens = np.array([len(r) for r in raws], dtype=np.uint64)
    caps = lens + (lens >> np.uint64(8)) + np.uint64(64 + 32)
    ssegs = np.zeros((n, 2), dtype=np.uint64); ssegs[:, 1] = lens; ssegs[1:, 0] = np.cumsum(lens)[:-1]
    dsegs = np.zeros((n, 2), dtype=np.uint64); dsegs[:, 1] = caps; dsegs[1:, 0] = np.cumsum(caps)[:-1]
    joined = b"".join(raws)
    src = np.frombuffer(joined, dtype=np.uint8).copy() if joined else np.zeros(1, dtype=np.uint8)
    dst = np.zeros(int(caps.sum()), dtype=np.uint8)
    sizes = np.zeros(n, dtype=np.uint64); st = np.full(n, -1, dtype=np.int32)
    ov = np.array([params.get(k, 0) for k in PARAM_NAMES], dtype=np.int32)
    assert set(params) <= set(PARAM_NAMES), params
    seqs = np.zeros((n, SEQ_STRIDE), dtype=np.uint64) if want_seqs else None
    meta = np.zeros((n, 4), dtype=np.uint32)
    rc = lib.emu_wave_frames(src.ctypes.data, ssegs.ctypes.data, n, dst.ctypes.data, dsegs.ctypes.data, sizes.ctypes.data, st.ctypes.data, level, ov.ctypes.data,
                             (1 if content_size else 0) | (2 if checksum else 0), blocks, {"libzstd": 0, "wave": 1}[finder], hlog,
                             seqs.ctypes.data if want_seqs else None, SEQ_STRIDE, meta.ctypes.data)
    if rc:
        raise RuntimeError("the call is refused (%d)" % rc)
    out = [dst[int(dsegs[i, 0]): int(dsegs[i, 0] + sizes[i])].tobytes() for i in range(n)]
    if not want_seqs:
        return out, st.tolist()
    return out, st.tolist(), [unpack(seqs[i, :int(meta[i, 0])]) if meta[i, 2] == 4 else None for i in range(n)], meta[:, 2].tolist()
