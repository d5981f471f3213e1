"""The edit call of the seekable streams (zhip_seekable_edit_device) without a GPU: the kernels behind the records' front half -- pick sizes, the two scans, the
verdict over picks, the tiled copy at every alignment, the table writer -- on the host wave emulator, every stream compared byte for byte with the Python
model of tests/seekable_edit_cases.py; the host's refusals; zhip_seekable_edit_bound; and the same cases as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer. The kernels never look inside a frame, so random bytes serve as frames."""
import os
import subprocess

import numpy as np
import pytest

from tests import seekable_edit_cases as ec
from tests import seekable_record_cases as rec

F, R = ec.FRAME, ec.RECORD


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return ec.emu(tmp_path_factory.mktemp("emu_seekable_edit"))


def test_tile_sizes(lib):
    t = np.zeros(2, dtype=np.uint32)
    lib.emu_edit_tiles(t.ctypes.data)
    assert int(t[0]) == ec.COPY_TILE, "the copy tile changed: COPY_SIZES has to follow it"
    assert int(t[1]) < 3 * 16 * 16, "the emulated copy grid is smaller than the alignment case's tiles: the stride over the tiles is walked"


# ---------------------------------------------------------------------------------------------------- 1. the copy at every alignment
@pytest.mark.parametrize("checksum", [False, True])
def test_copy_at_every_alignment(lib, checksum):
    case, covered = ec.alignment_case(checksum)
    assert covered == {(s, a, b) for s in ec.COPY_SIZES for a in range(16) for b in range(16)}, "every size from every source residue to every destination residue"
    ec.check(lib, case)


def test_copy_from_slots_at_every_destination_residue(lib):
    """new frames come from 16-aligned slots: each size at each destination residue, between kept frames of 1 .. 15 bytes"""
    rng = np.random.default_rng(12)
    old = ec.random_stream(rng, list(range(1, 16)), True)
    contents = [rng.integers(0, 256, size=s + 3, dtype=np.uint8).tobytes() for s in ec.COPY_SIZES]
    frames = [rng.integers(0, 256, size=s, dtype=np.uint8).tobytes() for s in ec.COPY_SIZES]
    picks, at = [], 0
    for j, s in enumerate(ec.COPY_SIZES):
        for d in range(16):
            pad = (d - at) % 16
            if pad:
                picks.append((F, pad - 1)); at += pad
            picks.append((R, j)); at += s
    ec.check(lib, ec.new_case(old=old, picks=picks, contents=contents, frames=frames))


# ---------------------------------------------------------------------------------------------------- 2. pick counts, duplicates, the table
@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("n", ec.PICK_COUNTS)
def test_pick_counts(lib, n, checksum):
    """the wave and the scan tile; one frame and one record picked several times; an empty frame's entry and a skippable frame among the kept ones; kept
    entries and their checksum words as they were (the model copies them from the old table)"""
    case = ec.mixed_case(n, checksum, 100 + n)
    if n > 41:
        assert case["picks"].count((F, 5)) >= 3 and case["picks"].count((R, 2)) >= 3 and (F, 3) in case["picks"] and (F, 6) in case["picks"]
    got = ec.check(lib, case)
    assert got["size"] == len(ec.expected_stream(case)) and got["dst"][got["size"] - 5] == (0x80 if checksum else 0), "the descriptor follows the old stream's"
    if n == 0:
        assert got["size"] == 17, "no picks: the 17-byte stream"


def test_without_an_old_stream(lib):
    """old == NULL: records only, the flag decides the checksums"""
    rng = np.random.default_rng(5)
    contents = [rng.integers(0, 256, size=s, dtype=np.uint8).tobytes() for s in (10, 0, 9000)]
    frames = [rng.integers(0, 256, size=s, dtype=np.uint8).tobytes() for s in (12, 9, 4097)]
    for checksum in (False, True):
        for picks in ([(R, 0), (R, 1), (R, 2)], [(R, 2), (R, 2), (R, 0)], []):
            ec.check(lib, ec.new_case(picks=picks, contents=contents, frames=frames, checksum=checksum))


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1024 * 256 + 1])
def test_tile_prefix_scan_matches_cumsum(lib, n):
    rng = np.random.default_rng(40 + n % 1000)
    sizes = rng.integers(0, 3 * ec.COPY_TILE, size=n, dtype=np.uint64)
    if n:
        sizes[rng.integers(0, n, size=max(1, n // 7))] = rng.choice(np.array([0, 1, ec.COPY_TILE - 1, ec.COPY_TILE, ec.COPY_TILE + 1, 1 << 30], dtype=np.uint64), size=max(1, n // 7))
    offs = np.full(n + 1, rec.NONE, dtype=np.uint64)
    a = sizes if n else np.zeros(1, dtype=np.uint64)
    lib.emu_edit_tile_scan(a.ctypes.data, n, offs.ctypes.data)
    assert np.array_equal(offs, ec.tile_prefix(sizes))


# ---------------------------------------------------------------------------------------------------- 3. in place
@pytest.mark.parametrize("checksum", [False, True])
def test_append_in_place(lib, checksum):
    """the kept frames are neither read nor written (poisoned once the entries are stashed, and still poison afterwards); the kept entries come from the stash;
    frames picked again behind the prefix are read from where they are"""
    case = ec.mixed_case(30, checksum, 7, in_place=True, poison=True)
    case["capacity"] += 100
    got = ec.check(lib, case)
    assert got["in_place"]
    case = ec.mixed_case(30, checksum, 8, in_place=True)
    assert any(k == F for k, _ in case["picks"][14:]), "kept frames are picked again behind the prefix"
    assert ec.check(lib, case)["in_place"]
    # nothing appended: the stream is written over itself and stays what it was
    old = case["old"]
    got = ec.check(lib, ec.new_case(old=old, picks=ec.identity_picks(14), in_place=True))
    assert got["in_place"] and got["dst"].tobytes() == old


# ---------------------------------------------------------------------------------------------------- 4. the verdict
@pytest.mark.parametrize("in_place", [False, True])
def test_verdict(lib, in_place):
    base = ec.mixed_case(40, True, 21, in_place=in_place)
    first_record = lambda j: next(k for k, p in enumerate(base["picks"]) if p == (R, j))
    # a refused record: at the lowest position, in the middle, at the last position; a refused record nobody picks does not fail the call
    for where in ("lowest", "middle", "last"):
        c = dict(base); c["picks"] = list(base["picks"]); c["rec_status"] = [0] * 6; c["capacity"] = base["capacity"] + 100000
        if where == "lowest":
            c["rec_status"][2] = 40; c["rec_status"][4] = 41
            k = min(first_record(2), first_record(4))
            want = [c["rec_status"][c["picks"][k][1]], k]
        elif where == "middle":
            k = len(c["picks"]) // 2
            c["picks"][k] = (R, 3); c["picks"] = [(R, 0) if p == (R, 3) and i != k else p for i, p in enumerate(c["picks"])]
            c["rec_status"][3] = 40; want = [40, k]
        else:
            k = len(c["picks"]) - 1
            c["picks"] = [(R, 0) if p == (R, 5) else p for p in c["picks"]]; c["picks"][k] = (R, 5)
            c["rec_status"][5] = 40; want = [40, k]
        assert ec.expected(c)[0] == want
        ec.check(lib, c)
    c = dict(base); c["picks"] = [p if p[0] == F or p[1] != 1 else (R, 0) for p in base["picks"]]; c["rec_status"] = [0, 40, 0, 0, 0, 0]
    c["capacity"] = len(ec.expected_stream(c))
    assert ec.expected(c)[0] == [0, 0]
    ec.check(lib, c)
    # the capacity: exactly enough; one byte short of the table: 70 at the last pick; one byte short of a frame in the middle: 70 at that pick
    need = len(ec.expected_stream(base))
    sizes = ec.pick_sizes(base)[0]
    n = len(sizes)
    c = dict(base, capacity=need); assert ec.expected(c)[0] == [0, 0]; ec.check(lib, c)
    c = dict(base, capacity=need - 1); assert ec.expected(c)[0] == [70, n - 1]; ec.check(lib, c)
    k = max(i for i in range(14 if in_place else 0, n * 2 // 3) if sizes[i])
    cap = sum(sizes[:k + 1]) - 1
    if in_place:
        cap = max(cap, len(base["old"]))
        k = next(i for i in range(n) if sum(sizes[:i + 1]) > cap)
    c = dict(base, capacity=cap); assert ec.expected(c)[0] == [70, k]; ec.check(lib, c)
    # a failed pre-check: its status with the RECORD index, whatever the harmless batch said
    c = dict(base, pre=0, pre_status=[72, 4]); assert ec.expected(c) == ([72, 4], None); ec.check(lib, c)


def test_host_refusals(lib):
    base = ec.mixed_case(20, False, 31)
    n = len(base["picks"])
    for picks, rc, pos in (([(F, 14)], ec.SIZE_MISMATCH, 0), (base["picks"] + [(R, 6)], ec.SIZE_MISMATCH, n), ([(F, 0), (2, 0)], ec.UNSUPPORTED, 1)):
        got = ec.check(lib, dict(base, picks=picks), want_rc=rc)
        assert got["position"] == pos
    # a frame pick without a stream
    got = ec.check(lib, dict(base, old=None, picks=[(R, 0), (F, 0)]), want_rc=ec.UNSUPPORTED)
    assert got["position"] == 1
    # the checksum flag must be the old stream's
    ec.check(lib, dict(base, checksum=True), want_rc=ec.UNSUPPORTED)
    # a destination at the old stream's base whose picks are not the append form
    for picks in (ec.identity_picks(14)[1:], ec.identity_picks(13), [(F, 0), (F, 2), (F, 1)] + ec.identity_picks(14)[3:], [(R, 0)] + ec.identity_picks(14)):
        ec.check(lib, dict(base, picks=picks, in_place=True, capacity=len(base["old"]) + 9000), want_rc=ec.UNSUPPORTED)


# ---------------------------------------------------------------------------------------------------- 5. the bound
def test_bound(lib):
    import zstandard_amd as zstd
    L = zstd._lib.lib()
    case = ec.mixed_case(50, True, 3)
    old = np.frombuffer(case["old"], dtype=np.uint8).copy()
    pk = np.array(case["picks"], dtype=np.uint32)
    for max_record in (0, 5000, 131072, 1 << 30):
        assert lib.emu_edit_bound(old.ctypes.data, len(old), pk.ctypes.data, len(pk), max_record, 1) == ec.bound_model(case["old"], case["picks"], max_record, True)
    assert lib.emu_edit_bound(old.ctypes.data, len(old), pk.ctypes.data, len(pk), 5000, 0) == 0, "the flag must be the old stream's"
    assert lib.emu_edit_bound(old.ctypes.data, len(old), pk.ctypes.data, len(pk), (1 << 30) + 1, 1) == 0
    bad = np.array([[0, 14]], dtype=np.uint32)
    assert lib.emu_edit_bound(old.ctypes.data, len(old), bad.ctypes.data, 1, 5000, 1) == 0, "no such frame"
    # without a handle the library's own function needs no GPU
    rp = np.array([[1, 0], [1, 7], [1, 0]], dtype=np.uint32)
    for ck in (0, 1):
        assert L.zhip_seekable_edit_bound(None, None, 0, 0, ck) == 17
        assert L.zhip_seekable_edit_bound(None, rp.ctypes.data, 3, 1000, ck) == 3 * rec.compress_bound(1000) + rec.table_size(3, ck) == lib.emu_edit_bound(None, 0, rp.ctypes.data, 3, 1000, ck)
    assert L.zhip_seekable_edit_bound(None, bad.ctypes.data, 1, 1000, 0) == 0, "a frame pick without a stream"
    assert L.zhip_seekable_edit_bound(None, rp.ctypes.data, 3, 1000, 2) == 0, "unknown flag"
    assert L.zhip_seekable_edit_bound(None, rp.ctypes.data, (1 << 27) + 1, 1000, 0) == 0
    # a record's frame is never above its term of the bound, whatever it is shorter than
    assert all(rec.compress_bound(a) <= rec.compress_bound(a + 1) for a in list(range(0, 70000)) + list(range(131072 - 3000, 131072 + 3000)))


# ---------------------------------------------------------------------------------------------------- 6. the sanitizer run
def test_sanitizer_run(lib, tmp_path):
    """the cases above as a stand-alone program built with -fsanitize=address,undefined, in a child process: every buffer has exactly the size the call is given"""
    prog = ec.sanitizer_program(tmp_path)
    path = os.path.join(str(tmp_path), "cases.bin")
    cases = 0
    with open(path, "wb") as f:
        ec.write_case(f, ec.alignment_case(True)[0]); cases += 1
        for n in ec.PICK_COUNTS:
            for checksum in (False, True):
                ec.write_case(f, ec.mixed_case(n, checksum, 100 + n)); cases += 1
        for checksum in (False, True):
            ec.write_case(f, ec.mixed_case(30, checksum, 7, in_place=True, poison=True)); cases += 1
            ec.write_case(f, ec.mixed_case(30, checksum, 8, in_place=True)); cases += 1
        for in_place in (False, True):
            base = ec.mixed_case(40, True, 21, in_place=in_place)
            need = len(ec.expected_stream(base))
            ec.write_case(f, dict(base, capacity=need - 1)); cases += 1
            ec.write_case(f, dict(base, capacity=max(need // 2, len(base["old"]) if in_place else 0))); cases += 1
            ec.write_case(f, dict(base, rec_status=[0, 0, 40, 0, 0, 0])); cases += 1
            ec.write_case(f, dict(base, pre=0, pre_status=[72, 4])); cases += 1
        base = ec.mixed_case(20, False, 31)
        ec.write_case(f, dict(base, picks=[(F, 14)]), want_rc=ec.SIZE_MISMATCH); cases += 1
        ec.write_case(f, dict(base, picks=ec.identity_picks(13), in_place=True, capacity=len(base["old"]) + 9000), want_rc=ec.UNSUPPORTED); cases += 1
    done = subprocess.run([prog, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode(errors="replace")[-4000:]
    assert done.stdout.decode().strip().endswith("%d cases" % cases)
