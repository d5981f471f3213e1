"""What the record tests of the seekable streams share (tests/test_emu_seekable_records.py on the host, tests/test_gpu_seekable_records.py on the GPU): record
layouts (shuffled, with gaps and shared bytes), Python models of the two record scans, of the pre-check and of the slot arithmetic, the pre-check's failing
cases, the host wave emulator's build of tests/emu/emu_seekable_records.cpp and its stand-alone sanitizer build with the case file it reads."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
GUARD_BYTE = 0x5A
NONE = (1 << 64) - 1
SRCSIZE_WRONG, DSTSIZE_TOO_SMALL = 72, 70
MAX_RECORDS, MAX_RECORD = 1 << 27, 1 << 30

# the lengths around every size at which the slot arithmetic changes: empty, below / at / above one block, several blocks
EDGE_LENGTHS = [0, 1, 63, 64, 4095, 131071, 131072, 131073, 400000]

_emu = {}


def emu(tmp_dir):
    """tests/emu/emu_seekable_records.cpp as a shared library"""
    if "lib" in _emu:
        return _emu["lib"]
    out = os.path.join(str(tmp_dir), "libzhip_emu_seekable_records.so")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + EMU_DIR, "-w", "-o", out, os.path.join(EMU_DIR, "zhemu.cpp"),
                           os.path.join(EMU_DIR, "emu_seekable_records.cpp")])
    lib = C.CDLL(out)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    lib.emu_seekable_tiles.restype = None; lib.emu_seekable_tiles.argtypes = [vp]
    lib.emu_records_scan.restype = u64; lib.emu_records_scan.argtypes = [vp, u32, u32, u64, u64, vp]
    lib.emu_records_compress.restype = u64; lib.emu_records_compress.argtypes = [vp, u64, vp, u32, u64, u64, u32, vp, vp, vp, u64, vp, vp, vp, vp]
    lib.emu_records_bound.restype = u64; lib.emu_records_bound.argtypes = [u64, u64, C.c_int]
    lib.emu_frame_offsets.restype = C.c_int; lib.emu_frame_offsets.argtypes = [vp, u64, u32, u32, vp]
    lib.emu_frames_run.restype = C.c_int; lib.emu_frames_run.argtypes = [vp, u64, vp, vp, u64, vp, vp, u64, u64, vp, vp, vp, vp, u64]
    lib.emu_seekable_xxh64.restype = u64; lib.emu_seekable_xxh64.argtypes = [vp, u32]
    lib.emu_seekable_validate.restype = C.c_int; lib.emu_seekable_validate.argtypes = [vp, u64, vp, vp, vp, vp]
    _emu["lib"] = lib
    return lib


def sanitizer_program(tmp_dir):
    """the same file as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer -> its path (the runtimes linked in: the program runs
    whatever else the process environment loads in front of it)"""
    out = os.path.join(str(tmp_dir), "emu_seekable_records_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-DZSK_RECORDS_MAIN", "-I" + EMU_DIR, "-w", "-o", out, os.path.join(EMU_DIR, "zhemu.cpp"), os.path.join(EMU_DIR, "emu_seekable_records.cpp")])
    return out


def compress_bound(n):
    """zhip_compress_bound"""
    return n + (n >> 8) + (((128 << 10) - n) >> 11 if n < (128 << 10) else 0)


def slot_stride(n):
    return (compress_bound(n) + 15) & ~15


def slot_bytes(max_content, n):
    """what the host reserves for the slots of n records whose lengths sum to at most max_content"""
    return max_content + (max_content >> 8) + 80 * n


def table_size(n, checksum):
    return 8 + n * (12 if checksum else 8) + 9


def layout(lengths, rng, shuffle=True, max_gap=40, share=0):
    """records of `lengths` placed in a source: in index order or shuffled, with gaps of 0 .. max_gap bytes, and `share` records that name the bytes another
    record of at least their length starts with -> ([(offset, length)], source size)"""
    n = len(lengths)
    order = [int(x) for x in rng.permutation(n)] if shuffle and n else list(range(n))
    offs, at = [0] * n, int(rng.integers(0, max_gap + 1)) if max_gap else 0
    for i in order:
        offs[i] = at
        at += lengths[i] + (int(rng.integers(0, max_gap + 1)) if max_gap else 0)
    for _ in range(share):
        i, j = (int(x) for x in rng.integers(0, n, size=2))
        if i != j and lengths[j] >= lengths[i]:
            offs[i] = offs[j]
    return list(zip(offs, lengths)), at


def records_array(records):
    a = np.array(records, dtype=np.uint64).reshape(-1, 2) if len(records) else np.zeros((1, 2), dtype=np.uint64)
    return np.ascontiguousarray(a)


def scan_model(records, mode, limit=MAX_RECORD, src_size=NONE):
    """-> (exclusive prefix sums with the total, as uint64 wraps them; lowest bad record or NONE) of the scan's record modes (3: lengths, 4: slot strides)"""
    lens = [int(l) for _, l in records]
    vals = lens if mode == 3 else [slot_stride(l) & NONE for l in lens]
    offs, at = [0], 0
    for v in vals:
        at = (at + v) & NONE
        offs.append(at)
    bad = NONE
    if mode == 3:
        for i, (o, l) in enumerate(records):
            if l > limit or o + l > src_size or o + l > NONE:
                bad = i
                break
    return np.array(offs, dtype=np.uint64), bad


def precheck_model(records, src_size, max_content, max_record):
    """-> [code, index] the device's pre-check gives"""
    limit = min(max_record, MAX_RECORD)
    for i, (o, l) in enumerate(records):
        if l > limit or o + l > src_size or o + l > NONE:
            return [SRCSIZE_WRONG, i]
    at = 0
    for i, (_, l) in enumerate(records):
        at += l
        if at > max_content:
            return [SRCSIZE_WRONG, i]
    return [0, 0]


def precheck_failures(n=70, seed=5):
    """the failing pre-checks, each one change to `n` good records of 1 .. 3000 bytes laid out with gaps -> [(name, records, source size, maxContentBytes,
    maxRecordBytes, [72, index])]; the expected index is the Python model's and is stated by every case as well"""
    rng = np.random.default_rng(seed)
    lengths = [int(x) for x in rng.integers(1, 3001, size=n)]
    max_record = max(lengths)
    good, src_size = layout(lengths, rng, shuffle=True)
    total = sum(lengths)
    out = []

    def case(name, records, content, want_index, src=src_size):
        want = [SRCSIZE_WRONG, want_index]
        assert precheck_model(records, src, content, max_record) == want, name
        out.append((name, records, src, content, max_record, want))

    for i in (0, n // 2, n - 1):
        r = list(good); r[i] = (0, max_record + 1)
        case("length maxRecordBytes + 1 at %d" % i, r, total + max_record + 1, i)
    last = max(range(n), key=lambda k: good[k][0] + good[k][1])
    r = list(good); r[last] = (src_size + 1 - good[last][1], good[last][1])
    case("offset + length == srcSize + 1 at %d" % last, r, total, last)
    r = list(good); r[n // 3] = (NONE - 5, 10)
    case("offset + length wraps at %d" % (n // 3), r, total, n // 3)
    r = list(good); r[n - 2] = (0, max_record + 1); r[7] = (src_size, 1)
    case("two failures: the lower index", r, total + max_record, 7)
    case("the sum is maxContentBytes + 1: the last record", list(good), total - 1, n - 1)
    # the running end crosses in the middle: the bound is the sum of the first 20 records less one byte
    case("the running end crosses at 19", list(good), sum(lengths[:20]) - 1, 19)
    case("maxContentBytes 0", list(good), 0, 0)
    return out


def run_compress(lib, src, records, max_content, max_record, checksum, sizes=None, status=None, capacity=None, guard=64):
    """the emulated compress call into a destination with guards -> dict(size, status, dst (the capacity's bytes), src_segs, slot_segs, slot_bytes, pre,
    refused (None or the first item whose segments lay outside a buffer), copied); asserts the guards"""
    n = len(records)
    s = np.frombuffer(bytes(src), dtype=np.uint8).copy() if len(src) else np.zeros(1, dtype=np.uint8)
    rec = records_array(records)
    given = np.array(sizes if sizes is not None else [0] * n, dtype=np.uint64) if n else np.zeros(1, dtype=np.uint64)
    st = np.array(status if status is not None else [0] * n, dtype=np.int32) if n else np.zeros(1, dtype=np.int32)
    if capacity is None:
        capacity = int(given[:n].sum()) + table_size(n, checksum)
    dst = np.full(guard + capacity + guard, GUARD_BYTE, dtype=np.uint8)
    ssegs = np.full((max(n, 1), 2), NONE, dtype=np.uint64); dsegs = np.full((max(n, 1), 2), NONE, dtype=np.uint64)
    out = np.full(2, -1, dtype=np.int32); info = np.zeros(4, dtype=np.uint64)
    size = lib.emu_records_compress(s.ctypes.data, len(src), rec.ctypes.data, n, max_content, max_record, int(checksum), given.ctypes.data, st.ctypes.data,
                                    dst[guard:].ctypes.data, capacity, ssegs.ctypes.data, dsegs.ctypes.data, out.ctypes.data, info.ctypes.data)
    assert (dst[:guard] == GUARD_BYTE).all() and (dst[guard + capacity:] == GUARD_BYTE).all(), "bytes outside [d_dst, d_dst + dstCapacity) were written"
    return dict(size=int(size), status=out.tolist(), dst=dst[guard:guard + capacity], src_segs=[tuple(int(v) for v in r) for r in ssegs[:n]],
                slot_segs=[tuple(int(v) for v in r) for r in dsegs[:n]], slot_bytes=int(info[0]), pre=int(info[1]), refused=(int(info[2]) - 1 if info[2] else None),
                copied=int(info[3]))


def stand_in_frame(i, size):
    """what the emulator's stand-in for the batch writes for item i"""
    return bytes((31 * i + j) & 0xFF for j in range(size))


def frames_run(lib, stream, content, frames, dst_offsets=None, capacity=None, limit=0, guard=64):
    """the emulated read by index -> (rc, status [2 + 2n], destination bytes, stats [8], ranges [(offset, length, dstOffset)]); asserts the guards"""
    buf = np.frombuffer(stream, dtype=np.uint8).copy()
    c = np.frombuffer(content, dtype=np.uint8).copy() if len(content) else np.zeros(1, dtype=np.uint8)
    n = len(frames)
    fr = np.array(frames, dtype=np.uint32) if n else np.zeros(1, dtype=np.uint32)
    offs = None if dst_offsets is None else (np.array(dst_offsets, dtype=np.uint64) if n else np.zeros(1, dtype=np.uint64))
    if capacity is None:
        capacity = len(content) * 3 + 64
    dst = np.full(guard + capacity + guard, GUARD_BYTE, dtype=np.uint8)
    status = np.full(2 + 2 * n, -1, dtype=np.int32)
    stats = np.zeros(8, dtype=np.uint64)
    rg = np.full((max(n, 1), 3), NONE, dtype=np.uint64)
    rc = lib.emu_frames_run(buf.ctypes.data, len(stream), c.ctypes.data, fr.ctypes.data, n, None if offs is None else offs.ctypes.data, dst[guard:].ctypes.data, capacity, limit,
                            status.ctypes.data, stats.ctypes.data, rg.ctypes.data, None, 0)
    assert (dst[:guard] == GUARD_BYTE).all() and (dst[guard + capacity:] == GUARD_BYTE).all(), "bytes outside [d_dst, d_dst + dstCapacity) were written"
    return rc, status.tolist(), dst[guard:guard + capacity], [int(x) for x in stats], [tuple(int(v) for v in r) for r in rg[:n]]


def frame_offsets(lib, stream, first, count):
    buf = np.frombuffer(stream, dtype=np.uint8).copy()
    out = np.full(count + 2, NONE, dtype=np.uint64)
    rc = lib.emu_frame_offsets(buf.ctypes.data, len(stream), first, count, out.ctypes.data)
    assert out[count + 1] == NONE, "count + 1 values, no more"
    return rc, [int(x) for x in out[:count + 1]]


def _blob(b):
    return struct.pack("<Q", len(b)) + bytes(b)


def write_compress_case(f, src, records, max_content, max_record, checksum, sizes, capacity, want):
    n = len(records)
    f.write(struct.pack("<Q", 1) + _blob(src) + struct.pack("<Q", n) + records_array(records)[:n].tobytes())
    f.write(struct.pack("<QQQ", max_content, max_record, int(checksum)) + np.array(sizes, dtype=np.uint64).tobytes() + struct.pack("<QQQ", capacity, want[0], want[1]))


def write_frames_case(f, stream, content, frames, limit):
    f.write(struct.pack("<Q", 2) + _blob(stream) + _blob(content) + struct.pack("<Q", len(frames)) + np.array(frames, dtype=np.uint32).tobytes() + struct.pack("<Q", limit))


def index_lists(rng, n):
    """the orders a read by index is asked in, for a table of n frames: ascending, reversed, with repeats, a random pick, none"""
    if not n:
        return [[]]
    some = sorted(set(int(x) for x in rng.integers(0, n, size=max(1, n // 2))))
    return [list(range(n)), list(range(n))[::-1], some, some[::-1], some + some[:3] + [some[0]], [int(x) for x in rng.integers(0, n, size=n + 5)], []]
