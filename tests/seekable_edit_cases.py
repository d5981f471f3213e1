"""What the edit tests of the seekable streams share (tests/test_emu_seekable_edit.py on the host, tests/test_gpu_seekable_edit.py on the GPU): the Python model
of an edited stream -- kept frames sliced out of the old stream by its table, new frames as given, the table written from the format description --, the
model of the verdict, pick lists, case builders, the host wave emulator's build of tests/emu/emu_seekable_edit.cpp and its stand-alone sanitizer build with the
case file it reads."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from tests import seekable_cases as sc
from tests import seekable_record_cases as rec

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
GUARD_BYTE, POISON_BYTE = 0x5A, 0xC3
FRAME, RECORD = 0, 1
COPY_TILE = 4096
UNSUPPORTED, SIZE_MISMATCH = 6, 3
# frame sizes of the copy at every alignment: around the 16 bytes of a lane, around the tile
COPY_SIZES = [0, 1, 15, 16, 17, 47, COPY_TILE - 1, COPY_TILE, COPY_TILE + 1, 3 * COPY_TILE + 5]
PICK_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257]

_emu = {}
_SOURCES = ["zhemu.cpp", "emu_seekable_edit.cpp"]


def emu(tmp_dir):
    """tests/emu/emu_seekable_edit.cpp as a shared library"""
    if "lib" in _emu:
        return _emu["lib"]
    out = os.path.join(str(tmp_dir), "libzhip_emu_seekable_edit.so")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + EMU_DIR, "-w", "-o", out] + [os.path.join(EMU_DIR, x) for x in _SOURCES])
    lib = C.CDLL(out)
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32
    lib.emu_edit_tiles.restype = None; lib.emu_edit_tiles.argtypes = [vp]
    lib.emu_edit_tile_scan.restype = None; lib.emu_edit_tile_scan.argtypes = [vp, u32, vp]
    lib.emu_edit_bound.restype = u64; lib.emu_edit_bound.argtypes = [vp, u64, vp, u64, u64, C.c_int]
    lib.emu_edit_run.restype = C.c_int
    lib.emu_edit_run.argtypes = [vp, u64, vp, u32, vp, vp, u32, vp, vp, vp, vp, i32, vp, u32, vp, u64, u32, vp, vp, vp, vp]
    _emu["lib"] = lib
    return lib


def sanitizer_program(tmp_dir):
    """the same file as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer -> its path (the runtimes linked in: the program runs
    whatever else the process environment loads in front of it)"""
    out = os.path.join(str(tmp_dir), "emu_seekable_edit_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-DZSK_EDIT_MAIN", "-I" + EMU_DIR, "-w", "-o", out] + [os.path.join(EMU_DIR, x) for x in _SOURCES])
    return out


# ---------------------------------------------------------------------------------------------------- the model
def frame_offsets(stream):
    """-> (entries, checksum flag, [compressed offset of frame i] + [the table's offset])"""
    entries, ck, at = sc.parse(stream)
    offs = [0]
    for e in entries:
        offs.append(offs[-1] + e[0])
    assert offs[-1] == at
    return entries, ck, offs


def model(old, picks, new_frames=(), new_contents=(), checksum=None):
    """the edited stream: pick (0, i) is frame i of `old` sliced by its table, with its entry as it is; pick (1, j) is new_frames[j] with the entry
    (its size, len(new_contents[j]), XXH64 low word of new_contents[j]); the table follows. checksum: the old stream's flag where there is one"""
    if old is not None:
        entries, ck, offs = frame_offsets(old)
        assert checksum is None or checksum == ck
        checksum = ck
    frames, table = [], []
    for kind, index in picks:
        if kind == FRAME:
            frames.append(bytes(old[offs[index]:offs[index + 1]]))
            table.append((entries[index][0], entries[index][1], entries[index][2] or 0))
        else:
            frames.append(bytes(new_frames[index]))
            table.append((len(new_frames[index]), len(new_contents[index]), sc.xxh64(bytes(new_contents[index])) & 0xFFFFFFFF))
    return b"".join(frames) + sc.table(table, bool(checksum))


def verdict_model(sizes, statuses, capacity, checksum):
    """zsk_verdict_body's rule over picks -> [code, position]: the lowest refused pick keeps its code; else 70 at the first pick whose frame ends beyond the
    capacity, at the last pick where only the table does not fit"""
    for k, st in enumerate(statuses):
        if st:
            return [int(st), k]
    n = len(sizes)
    if sum(sizes) + rec.table_size(n, checksum) <= capacity:
        return [0, 0]
    at = 0
    for k, s in enumerate(sizes):
        at += s
        if at > capacity:
            return [70, k]
    return [70, n - 1 if n else 0]


def tile_prefix(sizes):
    t = (np.array(sizes, dtype=np.uint64) + np.uint64(COPY_TILE - 1)) // np.uint64(COPY_TILE) if len(sizes) else np.zeros(0, dtype=np.uint64)
    return np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(t, dtype=np.uint64)])


def bound_model(old, picks, max_record, checksum):
    offs = frame_offsets(old)[2] if old is not None else None
    return sum(offs[i + 1] - offs[i] if k == FRAME else rec.compress_bound(max_record) for k, i in picks) + rec.table_size(len(picks), checksum)


# ---------------------------------------------------------------------------------------------------- streams and cases of random bytes (the emulator's)
def random_stream(rng, sizes, checksum, empty=(), skippable=()):
    """frames of random bytes of `sizes` with entries of random decompressed sizes and checksum words -- the edit never looks inside --; the frames at the
    positions `empty` have Decompressed_Size 0 (an empty frame's entry), those at `skippable` start with a skippable frame's magic and have Decompressed_Size 0"""
    frames, entries = [], []
    for i, s in enumerate(sizes):
        f = bytearray(rng.integers(0, 256, size=s, dtype=np.uint8).tobytes())
        d = int(rng.integers(1, 1 << 20))
        if i in skippable:
            assert s >= 8
            f[:8] = struct.pack("<II", 0x184D2A53, s - 8); d = 0
        if i in empty:
            d = 0
        frames.append(bytes(f)); entries.append((s, d, int(rng.integers(0, 1 << 32))))
    return b"".join(frames) + sc.table(entries, checksum)


def new_case(old=None, picks=(), contents=(), frames=(), rec_status=None, pre=None, pre_status=(0, 0), checksum=None, capacity=None, in_place=False, poison=False):
    """one call of the emulated edit. contents: the new records' source bytes, frames: what the batch "compressed" them to (any bytes); pre: None where there are
    no records, else the pre-check's go word; capacity None: exactly the stream's size"""
    if checksum is None:
        checksum = frame_offsets(old)[1] if old is not None else False
    n = len(contents)
    c = dict(old=old, picks=[(int(k), int(i)) for k, i in picks], contents=[bytes(x) for x in contents], frames=[bytes(x) for x in frames],
             rec_status=list(rec_status) if rec_status is not None else [0] * n, pre=(-1 if not n else 1) if pre is None else pre, pre_status=list(pre_status),
             checksum=bool(checksum), in_place=bool(in_place), poison=bool(poison))
    c["capacity"] = len(expected_stream(c)) if capacity is None else capacity
    return c


def pick_sizes(c):
    offs = frame_offsets(c["old"])[2] if c["old"] is not None else None
    sizes = [offs[i + 1] - offs[i] if k == FRAME else (0 if c["rec_status"][i] else len(c["frames"][i])) for k, i in c["picks"]]
    return sizes, [0 if k == FRAME else c["rec_status"][i] for k, i in c["picks"]]


def expected_stream(c):
    return model(c["old"], c["picks"], c["frames"], c["contents"], c["checksum"])


def expected(c):
    """-> (status pair, the stream or None where the call fails)"""
    if c["pre"] == 0:
        return list(c["pre_status"]), None
    sizes, statuses = pick_sizes(c)
    v = verdict_model(sizes, statuses, c["capacity"], c["checksum"])
    return v, (None if v[0] else expected_stream(c))


def _arrays(c):
    """the buffers of a case as the emulator takes them: source and record table (records back to back), slots 16-aligned in index order"""
    n = len(c["contents"])
    src = b"".join(c["contents"])
    records, at = [], 0
    for x in c["contents"]:
        records.append((at, len(x))); at += len(x)
    slot_segs, slots = [], bytearray()
    for i, f in enumerate(c["frames"]):
        cap = max(rec.compress_bound(len(c["contents"][i])), len(f))
        slots += bytes((-len(slots)) % 16)
        slot_segs.append((len(slots), cap))
        slots += f + bytes(cap - len(f))
    sizes = [len(f) for f in c["frames"]]
    return src, records, bytes(slots), slot_segs, sizes


def run(lib, c, guard=64):
    """the emulated call into a destination with guards -> dict(rc, status, size, go, position, dst (the capacity's bytes), offs, tile_offs, in_place); asserts
    the guards in front of and behind [d_dst, d_dst + dstCapacity)"""
    src, records, slots, slot_segs, sizes = _arrays(c)
    n, k = len(records), len(c["picks"])
    u8 = lambda b: np.frombuffer(bytes(b), dtype=np.uint8).copy() if len(b) else np.zeros(1, dtype=np.uint8)
    cap = c["capacity"]
    dst = np.full(guard + cap + guard, GUARD_BYTE, dtype=np.uint8)
    old = c["old"]
    if c["in_place"]:
        assert len(old) <= cap
        dst[guard:guard + len(old)] = np.frombuffer(old, dtype=np.uint8)
        old_ptr, old_buf = dst[guard:].ctypes.data, None
    else:
        old_buf = u8(old) if old is not None else None
        old_ptr = old_buf.ctypes.data if old is not None else None
    pk = np.array(c["picks"], dtype=np.uint32).reshape(-1, 2) if k else np.zeros((1, 2), dtype=np.uint32)
    s8, sl8 = u8(src), u8(slots)
    r64, seg64 = rec.records_array(records), rec.records_array(slot_segs)
    sz = np.array(sizes if n else [0], dtype=np.uint64); st = np.array(c["rec_status"] if n else [0], dtype=np.int32)
    pre_status = np.array(c["pre_status"], dtype=np.int32)
    out = np.full(2, -1, dtype=np.int32); info = np.zeros(8, dtype=np.uint64)
    offs = np.full(k + 1, rec.NONE, dtype=np.uint64); tiles = np.full(k + 1, rec.NONE, dtype=np.uint64)
    rc = lib.emu_edit_run(old_ptr, len(old) if old is not None else 0, pk.ctypes.data, k, s8.ctypes.data, r64.ctypes.data, n, sl8.ctypes.data, seg64.ctypes.data, sz.ctypes.data,
                          st.ctypes.data, c["pre"], pre_status.ctypes.data, int(c["checksum"]), dst[guard:].ctypes.data, cap, int(c["poison"]), out.ctypes.data, offs.ctypes.data,
                          tiles.ctypes.data, info.ctypes.data)
    assert (dst[:guard] == GUARD_BYTE).all() and (dst[guard + cap:] == GUARD_BYTE).all(), "bytes outside [d_dst, d_dst + dstCapacity) were written"
    if old_buf is not None:
        assert old_buf.tobytes()[:len(old)] == old, "the old stream was written"
    return dict(rc=rc, status=out.tolist(), size=int(info[0]), go=int(info[1]), position=int(info[7]), dst=dst[guard:guard + cap], offs=offs, tile_offs=tiles,
                in_place=bool(info[2]))


def untouched(c):
    """what the destination holds after a call that failed or was refused"""
    buf = bytearray([GUARD_BYTE]) * c["capacity"]
    if c["in_place"]:
        buf[:len(c["old"])] = c["old"]
    return bytes(buf)


def check(lib, c, want_rc=0):
    """runs the case and compares everything with the model: the whole stream byte for byte, or an untouched destination"""
    got = run(lib, c)
    assert got["rc"] == want_rc, got["rc"]
    if want_rc:
        assert got["status"] == [-1, -1] and got["dst"].tobytes() == untouched(c), "a refused call writes nothing, the status included"
        return got
    status, stream = expected(c)
    assert got["status"] == status, (got["status"], status)
    if stream is None:
        assert got["size"] == 0 and got["go"] == 0
        assert got["dst"].tobytes() == untouched(c), "a failed edit writes nothing" + (": the old stream is intact" if c["in_place"] else "")
        return got
    assert got["size"] == len(stream) and got["go"] == 1
    want = bytearray(untouched(c)); want[:len(stream)] = stream
    if c["in_place"] and c["poison"]:
        kept = frame_offsets(c["old"])[2][-1]
        want[:kept] = bytes([POISON_BYTE]) * kept
    assert got["dst"].tobytes() == bytes(want), "the stream differs from the model at byte %d" % next(i for i, (x, y) in enumerate(zip(got["dst"].tobytes(), bytes(want))) if x != y)
    sizes = pick_sizes(c)[0]
    assert np.array_equal(got["tile_offs"], tile_prefix(sizes)), "the tile prefix is numpy.cumsum of ceil(size / tile)"
    assert np.array_equal(got["offs"], np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(np.array(sizes, dtype=np.uint64), dtype=np.uint64)]))
    return got


def write_case(f, c, want_rc=0):
    """the case in the form the stand-alone program reads"""
    src, records, slots, slot_segs, sizes = _arrays(c)
    n, k = len(records), len(c["picks"])
    status, stream = expected(c) if not want_rc else ([0, 0], None)
    blob = lambda b: struct.pack("<Q", len(b)) + bytes(b)
    f.write(blob(c["old"] or b"") + struct.pack("<Q", k) + np.array(c["picks"], dtype=np.uint32).tobytes() + blob(src) + struct.pack("<Q", n))
    f.write(rec.records_array(records)[:n].tobytes() + blob(slots) + rec.records_array(slot_segs)[:n].tobytes() + np.array(sizes, dtype=np.uint64).tobytes())
    f.write(np.array(c["rec_status"], dtype=np.int32).tobytes() + struct.pack("<qii", c["pre"], *c["pre_status"]))
    f.write(struct.pack("<QQQQQ", int(c["checksum"]), c["capacity"], int(c["in_place"]), int(c["poison"]), want_rc) + struct.pack("<ii", *status) + blob(stream or b""))


# ---------------------------------------------------------------------------------------------------- case builders
def alignment_case(checksum=False, seed=11):
    """an old stream that holds every size of COPY_SIZES at each of the 16 source residues, and a pick order that puts each of them at each of the 16
    destination residues: 2 560 copies; frames of 1 .. 15 bytes adjust the residues on both sides. -> (case, {(size, source residue, destination residue)})"""
    rng = np.random.default_rng(seed)
    sizes, at, where = list(range(1, 16)), sum(range(1, 16)), {}            # frames 0 .. 14: the fillers of 1 .. 15 bytes
    for s in COPY_SIZES:
        for r in range(16):
            pad = (r - at) % 16
            if pad:
                sizes.append(pad); at += pad
            where[(s, r)] = len(sizes)
            sizes.append(s); at += s
    old = random_stream(rng, sizes, checksum)
    offs = frame_offsets(old)[2]
    picks, at, covered = [], 0, set()
    for s in COPY_SIZES:
        for r in range(16):
            i = where[(s, r)]
            assert offs[i] % 16 == r and offs[i + 1] - offs[i] == s
            for d in range(16):
                pad = (d - at) % 16
                if pad:
                    picks.append((FRAME, pad - 1)); at += pad
                picks.append((FRAME, i)); covered.add((s, offs[i] % 16, at % 16)); at += s
    return new_case(old=old, picks=picks), covered


def mixed_case(n_picks, checksum, seed, in_place=False, poison=False):
    """n_picks picks over an old stream of 14 frames (an empty frame's entry, a skippable frame, a frame above the tile) and 6 new records (one empty), with one
    frame and one record picked several times; in place the picks begin with every old frame and only records follow where `poison` is set"""
    rng = np.random.default_rng(seed)
    sizes = [int(x) for x in rng.integers(9, 700, size=14)]
    sizes[3], sizes[9] = 13, COPY_TILE + 77
    old = random_stream(rng, sizes, checksum, empty=(3,), skippable=(6,))
    contents = [rng.integers(0, 256, size=int(s), dtype=np.uint8).tobytes() for s in (100, 0, 3000, 1, 17, 5000)]
    frames = [rng.integers(0, 256, size=int(s), dtype=np.uint8).tobytes() for s in (40, 9, 2 * COPY_TILE + 3, 10, 16, 333)]
    picks = [(int(k), int(rng.integers(0, 14 if k == FRAME else 6))) for k in rng.integers(0, 2, size=n_picks)]
    if poison:
        picks = [(RECORD, i % 6) for _, i in picks]
    for at, p in ((2, (FRAME, 5)), (7, (FRAME, 5)), (11, (FRAME, 5)), (4, (RECORD, 2)), (20, (RECORD, 2)), (33, (RECORD, 2)), (40, (FRAME, 3)), (41, (FRAME, 6))):
        if at < len(picks) and not (poison and p[0] == FRAME):
            picks[at] = p
    if in_place:
        picks = [(FRAME, i) for i in range(14)] + picks
    c = new_case(old=old, picks=picks, contents=contents, frames=frames, in_place=in_place, poison=poison)
    return c


def identity_picks(n):
    return [(FRAME, i) for i in range(n)]
