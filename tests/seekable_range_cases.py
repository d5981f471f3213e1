"""What the many-ranges tests share (tests/test_emu_seekable_ranges.py on the host, tests/test_gpu_seekable_ranges.py on the GPU): the host wave emulator's build
of the plan and the three gather kernels (tests/emu/emu_seekable_ranges.cpp), its stand-alone sanitizer build, the random tables and range lists, destinations
with guards, and a brute-force model of which frames a range list touches."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from tests import seekable_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
GUARD_BYTE = 0x5A
DEFAULT_LIMIT = 1 << 30
LIMITS = (0, 1, 4096, 20000)                 # 0: the default

# (seed, frames, ranges): every test of the plan and of the emulated path runs all of these
SEEDS = [(1, 1, 0), (2, 1, 3), (3, 2, 9), (4, 7, 1), (5, 33, 40), (6, 64, 64), (7, 65, 300), (8, 120, 17), (9, 257, 130), (10, 400, 300), (11, 400, 5), (12, 13, 300)]

_emu = {}


def emu(tmp_dir):
    """tests/emu/emu_seekable_ranges.cpp as a shared library"""
    if "lib" in _emu:
        return _emu["lib"]
    out = os.path.join(str(tmp_dir), "libzhip_emu_seekable_ranges.so")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + EMU_DIR, "-w", "-o", out, os.path.join(EMU_DIR, "zhemu.cpp"),
                           os.path.join(EMU_DIR, "emu_seekable_ranges.cpp")])
    lib = C.CDLL(out)
    vp, u64, i64 = C.c_void_p, C.c_uint64, C.c_int64
    lib.emu_gather_plan.restype = C.c_int; lib.emu_gather_plan.argtypes = [vp, u64, vp, u64, u64, u64, vp, vp, u64, vp, u64, vp, u64, vp]
    lib.emu_gather_run.restype = C.c_int; lib.emu_gather_run.argtypes = [vp, u64, vp, vp, u64, vp, u64, u64, i64, i64, C.c_int32, vp, vp, vp, u64]
    lib.emu_seekable_xxh64.restype = u64; lib.emu_seekable_xxh64.argtypes = [vp, C.c_uint32]
    _emu["lib"] = lib
    return lib


def sanitizer_program(tmp_dir):
    """the same file as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer -> its path (the runtimes linked in: the program runs
    whatever else the process environment loads in front of it)"""
    out = os.path.join(str(tmp_dir), "emu_seekable_ranges_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-DZSK_RANGES_MAIN",
                           "-I" + EMU_DIR, "-w", "-o", out, os.path.join(EMU_DIR, "zhemu.cpp"), os.path.join(EMU_DIR, "emu_seekable_ranges.cpp")])
    return out


def _xxh_low(lib, chunk):
    b = np.frombuffer(chunk, dtype=np.uint8).copy() if len(chunk) else np.zeros(1, dtype=np.uint8)
    return int(lib.emu_seekable_xxh64(b.ctypes.data, len(chunk))) & 0xFFFFFFFF


def stream_for(lib, sizes, content, checksum, rng):
    """a stream whose table lists frames of `sizes` content bytes (the frames themselves are a few random bytes each: nothing here decodes them)"""
    at, entries, frames = 0, [], []
    for s in sizes:
        blob = bytes(rng.integers(0, 256, size=int(rng.integers(1, 12)), dtype=np.uint8))
        frames.append(blob)
        entries.append((len(blob), int(s), _xxh_low(lib, content[at:at + s]) if checksum else 0))
        at += s
    return b"".join(frames) + sc.table(entries, checksum)


def random_sizes(rng, n):
    """n Decompressed_Size values in 0 .. 9000 with runs of empty entries, single bytes and repeated sizes"""
    sizes = rng.integers(1, 9001, size=n)
    i = 0
    while i < n:
        kind = int(rng.integers(0, 12))
        run = int(rng.integers(1, 5))
        if kind == 0:
            sizes[i:i + run] = 0
        elif kind == 1:
            sizes[i:i + run] = 4096
        elif kind == 2:
            sizes[i] = 1
        i += run
    return [int(x) for x in sizes]


def random_ranges(rng, d_off, count):
    """`count` (offset, length) from the issue's ingredients: zero-length, whole content, duplicates, nested, ending exactly on frame boundaries, inside one frame"""
    total, n = int(d_off[-1]), len(d_off) - 1
    out = []
    while len(out) < count:
        kind = int(rng.integers(0, 8))
        if total == 0 or kind == 0:
            out.append((int(rng.integers(0, total + 1)), 0))
        elif kind == 1:
            out.append((0, total))
        elif kind == 2 and out:
            out.append(out[int(rng.integers(0, len(out)))])
        elif kind == 3 and out and out[-1][1] > 2:                          # nested in the one before
            o, l = out[-1]
            a = int(rng.integers(0, l - 1)); b = int(rng.integers(a + 1, l + 1))
            out.append((o + a, b - a))
        elif kind == 4:                                                    # frame boundary to frame boundary
            a, b = sorted(int(x) for x in rng.integers(0, n + 1, size=2))
            out.append((int(d_off[a]), int(d_off[b] - d_off[a])))
        elif kind == 5:                                                    # ends exactly on a frame boundary
            b = int(d_off[int(rng.integers(1, n + 1))])
            a = int(rng.integers(0, b + 1))
            out.append((a, b - a))
        elif kind == 6:                                                    # inside one frame
            f = int(rng.integers(0, n))
            if d_off[f + 1] > d_off[f]:
                a = int(rng.integers(d_off[f], d_off[f + 1])); b = int(rng.integers(a, d_off[f + 1])) + 1
                out.append((a, b - a))
        else:
            a = int(rng.integers(0, total)); l = int(rng.integers(1, min(total - a, 30000) + 1))
            out.append((a, l))
    return out


def place_destinations(rng, ranges, max_gap=40):
    """every range a destination of its own, in a random order with guard gaps -> ([(offset, length, dstOffset)], capacity)"""
    order = rng.permutation(len(ranges)) if len(ranges) else []
    at = int(rng.integers(0, max_gap + 1))
    dst = [0] * len(ranges)
    for r in order:
        dst[r] = at
        at += ranges[r][1] + int(rng.integers(0, max_gap + 1))
    return [(o, l, d) for (o, l), d in zip(ranges, dst)], at + int(rng.integers(0, max_gap + 1))


class Case:
    """one seed: the table, its content and stream, a range list with destinations"""

    def __init__(self, lib, seed, n, n_ranges, checksum):
        rng = np.random.default_rng(7000 + seed)
        self.sizes = random_sizes(rng, n)
        self.d_off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.total = int(self.d_off[-1])
        self.content = bytes(rng.integers(0, 256, size=self.total, dtype=np.uint8))
        self.stream = stream_for(lib, self.sizes, self.content, checksum, rng)
        self.ranges, self.capacity = place_destinations(rng, random_ranges(rng, self.d_off, n_ranges))
        self.name = "seed %d: %d frames, %d ranges" % (seed, n, n_ranges)


_cases = {}


def cases(lib, checksum=False):
    if checksum not in _cases:
        _cases[checksum] = [Case(lib, s, n, r, checksum) for s, n, r in SEEDS]
    return _cases[checksum]


def ranges_array(ranges):
    a = np.array(ranges, dtype=np.uint64).reshape(-1, 3) if len(ranges) else np.zeros((1, 3), dtype=np.uint64)
    return np.ascontiguousarray(a)


def model(d_off, ranges):
    """brute force over frames x ranges -> (touch count per frame, frames that lie wholly inside exactly one range and are touched by no other); frames of no
    content count as untouched"""
    lo, hi = d_off[:-1][:, None], d_off[1:][:, None]
    r = np.array([(o, o + l) for o, l, _ in ranges if l], dtype=np.int64).reshape(-1, 2)
    if not len(r):
        z = np.zeros(len(d_off) - 1, dtype=np.int64)
        return z, z.astype(bool)
    a, b = r[:, 0][None, :], r[:, 1][None, :]
    touch = (lo < b) & (hi > a) & (hi > lo)
    inside = touch & (a <= lo) & (hi <= b)
    count = touch.sum(axis=1)
    return count, (count == 1) & (inside.sum(axis=1) == 1)


def plan(lib, stream, ranges, capacity, limit):
    """-> (rc, stats, segs [(first, frames, item, home, inPlace, pass)], jobs [(pass, src, dst, bytes)], passes [(scratch, item0, item1, tiles)], [(f0, f1)])"""
    buf = np.frombuffer(stream, dtype=np.uint8).copy()
    rg = ranges_array(ranges)
    R = len(ranges)
    frames = len(stream) // 8                                               # (more than the table has entries)
    cap, job_cap = 4 * R + 2 * frames + 16, (R + 1) * (frames + 1)          # a scratch frame may be a pass of its own, and a job is per range and pass
    stats = np.zeros(8, dtype=np.uint64)
    segs = np.zeros((cap, 6), dtype=np.uint64); jobs = np.zeros((job_cap, 4), dtype=np.uint64); passes = np.zeros((cap, 4), dtype=np.uint64)
    fr = np.zeros((max(R, 1), 2), dtype=np.uint64)
    rc = lib.emu_gather_plan(buf.ctypes.data, len(stream), rg.ctypes.data, R, capacity, limit, stats.ctypes.data, segs.ctypes.data, cap, jobs.ctypes.data, job_cap,
                             passes.ctypes.data, cap, fr.ctypes.data)
    st = [int(x) for x in stats]
    as_rows = lambda a, k: [tuple(int(v) for v in row) for row in a[:k]]
    return rc, st, as_rows(segs, st[5]), as_rows(jobs, st[3]), as_rows(passes, st[4]), as_rows(fr, R)


def run(lib, stream, content, ranges, capacity, limit=0, short_frame=-1, code_frame=-1, code=0, guard=64):
    """the emulated call into a destination with `guard` bytes on both sides -> (rc, status list [2 + 2R], destination bytes, stats,
    items [(frame, 0 d_dst / 1 scratch, offset, length, pass)]); asserts the guards"""
    buf = np.frombuffer(stream, dtype=np.uint8).copy()
    c = np.frombuffer(content, dtype=np.uint8).copy() if len(content) else np.zeros(1, dtype=np.uint8)
    rg = ranges_array(ranges)
    R = len(ranges)
    dst = np.full(guard + capacity + guard, GUARD_BYTE, dtype=np.uint8)
    status = np.full(2 + 2 * R, -1, dtype=np.int32)
    stats = np.zeros(8, dtype=np.uint64)
    cap = len(stream) // 8 + 1
    items = np.zeros((cap, 5), dtype=np.uint64)
    rc = lib.emu_gather_run(buf.ctypes.data, len(stream), c.ctypes.data, rg.ctypes.data, R, dst[guard:].ctypes.data, capacity, limit, short_frame, code_frame, code,
                            status.ctypes.data, stats.ctypes.data, items.ctypes.data, cap)
    assert (dst[:guard] == GUARD_BYTE).all() and (dst[guard + capacity:] == GUARD_BYTE).all(), "bytes outside [d_dst, d_dst + dstCapacity) were written"
    st = [int(x) for x in stats]
    return rc, status.tolist(), dst[guard:guard + capacity], st, [tuple(int(v) for v in row) for row in items[:st[0]]]


def untouched_mask(ranges, capacity):
    """True where no range's destination lies"""
    m = np.ones(capacity, dtype=bool)
    for _, l, d in ranges:
        m[d:d + l] = False
    return m


def write_case_file(path, case_list, limits, append=False):
    """the sanitizer program's input: every case at every limit -> how many were written"""
    with open(path, "ab" if append else "wb") as f:
        for c in case_list:
            for limit in limits:
                f.write(struct.pack("<Q", len(c.stream))); f.write(c.stream)
                f.write(struct.pack("<Q", len(c.content))); f.write(c.content)
                f.write(struct.pack("<Q", len(c.ranges))); f.write(ranges_array(c.ranges)[:len(c.ranges)].tobytes())
                f.write(struct.pack("<QQ", c.capacity, limit))
    return len(case_list) * len(limits)
