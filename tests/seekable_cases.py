"""What the seekable-stream tests share (tests/test_emu_seekable.py on the host, tests/test_gpu_seekable.py on the GPU): the (srcSize, frameSize) cases, the
seek table written and parsed in Python from the layout in include/zstd_hip.h, XXH64 in Python, and the host wave emulator's build of the kernels."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

SKIP_MAGIC, SEEK_MAGIC = 0x184D2A5E, 0x8F92EAB1
MAX_FRAMES, MAX_CONTENT = 1 << 27, 1 << 30
UNSUPPORTED, SIZE_MISMATCH = 6, 3            # ZHIP_ERR_UNSUPPORTED, ZHIP_ERR_SIZE_MISMATCH (include/zstd_hip.h): what a refused call returns, emulated or not

# (srcSize, frameSize) of the streams the GPU suite writes
CASES = [(0, 4096), (1, 4096), (4095, 4096), (4096, 4096), (4097, 4096), (5 * 4096 + 17, 4096), (5, 1), (3 * 131072 + 1, 131072), (2 * 131072 + 20000, 131072)]
RANGE_CASE = (5 * 4096 + 17, 4096)


def ranges_of(total):
    """(offset, length) of the range reads, for a content of `total` bytes cut every 4096"""
    return [(0, 0), (0, 1), (0, total), (4095, 2), (4096, 4096), (4097, 8190), (total - 1, 1), (total, 0)]


_source = {}


def source(n):
    """the first n bytes of the corpus' frames 40, 41, ... (text, records, binary, ... as tests/corpus.py mixes them)"""
    from tests.corpus import Corpus
    if "data" not in _source or len(_source["data"]) < n:
        _source["data"] = b"".join(Corpus().frame_list(40, max(4, (n + 131071) // 131072)))
    return _source["data"][:n]


def chunks(data, frame_size):
    return [data[i:i + frame_size] for i in range(0, len(data), frame_size)]


def xxh64(data, seed=0):
    """XXH64, the public algorithm, in Python integers"""
    M = (1 << 64) - 1
    P1, P2, P3, P4, P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
    rotl = lambda x, r: ((x << r) | (x >> (64 - r))) & M
    rnd = lambda acc, v: (rotl((acc + v * P2) & M, 31) * P1) & M
    n, p = len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed, (seed - P1) & M]
        while p + 32 <= n:
            for k, w in enumerate(struct.unpack_from("<4Q", data, p)):
                v[k] = rnd(v[k], w)
            p += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for x in v:
            h = ((h ^ rnd(0, x)) * P1 + P4) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while p + 8 <= n:
        h = (rotl(h ^ rnd(0, struct.unpack_from("<Q", data, p)[0]), 27) * P1 + P4) & M; p += 8
    if p + 4 <= n:
        h = (rotl(h ^ (struct.unpack_from("<I", data, p)[0] * P1) & M, 23) * P2 + P3) & M; p += 4
    while p < n:
        h = (rotl(h ^ (data[p] * P5) & M, 11) * P1) & M; p += 1
    h ^= h >> 33; h = (h * P2) & M; h ^= h >> 29; h = (h * P3) & M; h ^= h >> 32
    return h


def table(entries, checksum, descriptor_extra=0, n_frames=None, frame_size_field=None):
    """the table frame for entries [(compressedSize, decompressedSize, checksum)]; the keyword arguments overwrite single fields (damage for the validator)"""
    n = len(entries)
    e = 12 if checksum else 8
    body = b"".join(struct.pack("<III", *x) if checksum else struct.pack("<II", x[0], x[1]) for x in entries)
    nf = n if n_frames is None else n_frames
    fs = nf * e + 9 if frame_size_field is None else frame_size_field
    return struct.pack("<II", SKIP_MAGIC, fs) + body + struct.pack("<IBI", nf, (0x80 if checksum else 0) | descriptor_extra, SEEK_MAGIC)


def parse(stream):
    """-> (entries [(compressedSize, decompressedSize, checksum or None)], checksum flag, offset of the table frame); asserts the layout"""
    stream = bytes(stream)
    n, desc, magic = struct.unpack_from("<IBI", stream, len(stream) - 9)
    assert magic == SEEK_MAGIC and not desc & 0x7C
    ck = bool(desc & 0x80)
    e = 12 if ck else 8
    at = len(stream) - (8 + n * e + 9)
    assert at >= 0 and struct.unpack_from("<II", stream, at) == (SKIP_MAGIC, n * e + 9)
    ent = []
    for i in range(n):
        f = struct.unpack_from("<III" if ck else "<II", stream, at + 8 + i * e)
        ent.append((f[0], f[1], f[2] if ck else None))
    assert sum(x[0] for x in ent) == at
    return ent, ck, at


def stream_of(frames, contents, checksum, extra_entries=()):
    """frames back to back + their table (what a correct writer makes of them); extra_entries: [(position, frame bytes)] listed with Decompressed_Size 0"""
    items = [(f, len(c), xxh64(c) & 0xFFFFFFFF) for f, c in zip(frames, contents)]
    for pos, blob in extra_entries:
        items.insert(pos, (blob, 0, xxh64(b"") & 0xFFFFFFFF))
    return b"".join(x[0] for x in items) + table([(len(x[0]), x[1], x[2]) for x in items], checksum)


def validator_damage(good, n, checksum):
    """single changes to a good stream of n frames -> [(name, stream, zstd error code the open call must give)]"""
    e = 12 if checksum else 8
    at = len(good) - (8 + n * e + 9)
    g = bytearray(good)

    def put(off, fmt, v):
        b = bytearray(g); struct.pack_into(fmt, b, off, v); return bytes(b)

    frame_size = n * e + 9
    c2 = struct.unpack_from("<I", g, at + 8 + 2 * e)[0]
    out = [("seekable magic", put(len(g) - 4, "<I", SEEK_MAGIC ^ 1), 10),
           ("skippable magic", put(at, "<I", SKIP_MAGIC ^ 0x10), 10),
           ("Frame_Size + 1", put(at + 4, "<I", frame_size + 1), 20),
           ("Frame_Size - 1", put(at + 4, "<I", frame_size - 1), 20),
           ("Compressed_Size + 1", put(at + 8 + 2 * e, "<I", c2 + 1), 20),
           ("Compressed_Size - 1", put(at + 8 + 2 * e, "<I", c2 - 1), 20),
           ("Decompressed_Size 2^30 + 1", put(at + 8 + 3 * e + 4, "<I", MAX_CONTENT + 1), 20),
           ("Number_Of_Frames 2^27 + 1", put(at + 4, "<I", (MAX_FRAMES + 1) * e + 9)[:len(g) - 9] + struct.pack("<I", MAX_FRAMES + 1) + bytes(g[len(g) - 5:]), 20),
           # a stream cut short no longer ends in the seekable magic: the footer is read from the last 9 bytes that are there
           ("truncated by 1", bytes(g[:-1]), 10),
           ("truncated by 9", bytes(g[:-9]), 10)]
    for bit in range(2, 7):
        out.append(("reserved bit %d" % bit, put(len(g) - 5, "<B", g[len(g) - 5] | (1 << bit)), 20))
    return out


_emu = {}


def emu(tmp_dir):
    """the kernels of python-zstandard_amd/csrc/zhip_seekable.hpp built for the host wave emulator (tests/emu/emu_seekable.cpp)"""
    if "lib" in _emu:
        return _emu["lib"]
    out = os.path.join(str(tmp_dir), "libzhip_emu_seekable.so")
    d = os.path.join(HERE, "emu")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + d, "-w", "-o", out, os.path.join(d, "zhemu.cpp"), os.path.join(d, "emu_seekable.cpp")])
    lib = C.CDLL(out)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    lib.emu_seekable_tiles.restype = None; lib.emu_seekable_tiles.argtypes = [vp]
    lib.emu_seekable_scan.restype = u64; lib.emu_seekable_scan.argtypes = [vp, vp, u32, vp]
    lib.emu_seekable_table.restype = u64; lib.emu_seekable_table.argtypes = [vp, u64, u32, u32, vp, vp, vp, u64, vp, vp, vp]
    lib.emu_seekable_validate.restype = C.c_int; lib.emu_seekable_validate.argtypes = [vp, u64, vp, vp, vp, vp]
    lib.emu_seekable_range.restype = C.c_int; lib.emu_seekable_range.argtypes = [vp, u64, vp, u64, u64, vp, C.c_int64, vp, vp, vp]
    lib.emu_seekable_bound.restype = u64; lib.emu_seekable_bound.argtypes = [u64, u32, C.c_int]
    lib.emu_seekable_xxh64.restype = u64; lib.emu_seekable_xxh64.argtypes = [vp, u32]
    _emu["lib"] = lib
    return lib


def emu_validate(lib, stream):
    """-> (zstd error code, info or None): the open call's checks under emulation, on exactly len(stream) bytes"""
    buf = np.frombuffer(bytes(stream), dtype=np.uint8).copy() if len(stream) else np.zeros(1, dtype=np.uint8)
    info = np.zeros(5, dtype=np.uint64)
    code = lib.emu_seekable_validate(buf.ctypes.data, len(stream), info.ctypes.data, None, None, None)
    return code, (None if code else [int(x) for x in info])
