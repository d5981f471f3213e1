"""The flat fast-strategy search (ze_fast_flat_np: one lane per source, a pair or two of the reference's pair loop per trip, tagged and numbered
cells) against the lane-serial restatement it replaces for one-block sources (ze_fast), sequence by sequence, on the host. ze_fast is pinned to
libzstd's parse by test_emulated_fast_strategy_matches_golden and the GPU suite, so equality here is equality with libzstd."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MMLS = (4, 5, 6, 7)
TLENS = (0, 1, 3, 7, 50)            # 0: levels 1 and 2; n: level -n
HLOGS = (10, 13, 15)
PAIRS = (1, 2)
GRID = [(m, t, h, p) for m in MMLS for t in TLENS for h in HLOGS for p in PAIRS]


@pytest.fixture(scope="module")
def ff(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_fast_flat") / "libzhip_emu_fast_flat.so")
    emu = os.path.join(HERE, "emu")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + emu, "-w", "-o", out,
                           os.path.join(emu, "zhemu.cpp"), os.path.join(emu, "emu_fast_flat.cpp")])
    lib = ctypes.CDLL(out)
    u8p, u32p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    lib.emu_fast_flat.restype = ctypes.c_uint32
    lib.emu_fast_flat.argtypes = [u8p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, u32p, u64p]
    lib.emu_fast_serial.restype = ctypes.c_uint32
    lib.emu_fast_serial.argtypes = [u8p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, u64p]

    class FF:
        def flat(self, raw, hlog, mml, tlen, pairs, epoch=0, table=None):
            src = np.frombuffer(raw, dtype=np.uint8).copy()           # exactly len(raw) bytes: the search may not read past them
            if table is None: table = np.zeros(1 << hlog, dtype=np.uint32)
            seqs = np.zeros(len(raw) // 4 + 8, dtype=np.uint64)
            n = lib.emu_fast_flat(src.ctypes.data_as(u8p), len(raw), hlog, mml, tlen, pairs, epoch, table.ctypes.data_as(u32p), seqs.ctypes.data_as(u64p))
            return seqs[:n]

        def serial(self, raw, hlog, mml, tlen):
            src = np.frombuffer(raw, dtype=np.uint8).copy()
            seqs = np.zeros(len(raw) // 4 + 8, dtype=np.uint64)
            n = lib.emu_fast_serial(src.ctypes.data_as(u8p), len(raw), hlog, mml, tlen, seqs.ctypes.data_as(u64p))
            return seqs[:n]

    return FF()


def _same(ff, raw, combos, what):
    want = {}
    for m, t, h, p in combos:
        if (m, t, h) not in want: want[(m, t, h)] = ff.serial(raw, h, m, t)
        got = ff.flat(raw, h, m, t, p)
        w = want[(m, t, h)]
        assert len(got) == len(w) and np.array_equal(got, w), "%s (%d bytes): mml %d tlen %d hlog %d pairs %d: %d sequences against %d, first difference at %s" % (
            what, len(raw), m, t, h, p, len(got), len(w), next((i for i in range(min(len(got), len(w))) if got[i] != w[i]), min(len(got), len(w))))
    return sum(len(w) for w in want.values())


SIZES = (64, 65, 71, 72, 73, 79, 80, 81, 127, 128, 129, 4095, 131071, 131072)


def test_exit_test_and_last_position_guard(ff, corpus):
    """the `ip3 >= ilimit` exit and the `ip0 <= ilimit` guard of the insertions: sources that end at every residue of the pair loop, text and a short period (matches up to the end)"""
    rng = np.random.default_rng(5)
    text = corpus.frame_bytes(9)
    period = (rng.bytes(37) * (131072 // 37 + 1))
    total = 0
    for n in SIZES:
        combos = GRID if n < 4096 else GRID[n % 7::7]
        total += _same(ff, text[:n], combos, "text")
        total += _same(ff, period[:n], combos, "period 37")
        total += _same(ff, text[131072 - n:], combos, "text tail")
    assert total > 1000


def test_step_past_four_flips_the_pending_write(ff, corpus):
    """2-4 KiB without a match raise `step` past 4 (one per 128 bytes): after a hit at a pair's second position the cell of the pair's third is then NOT written"""
    rng = np.random.default_rng(6)
    text = corpus.frame_bytes(3)
    for k in (2048, 3000, 4096):
        for rep in range(3):
            raw = rng.bytes(k) + text[rep * 500: rep * 500 + 6000] + rng.bytes(700) + text[:3000]
            assert _same(ff, raw, GRID, "random then text") > 0


def test_equal_hashes_inside_a_trip(ff):
    """alphabets of 2 and 3 symbols: the positions of a trip share hash cells all the time, so every read depends on the forwarding of the trip's earlier writes"""
    rng = np.random.default_rng(7)
    for syms in (2, 3):
        for n in (200, 3001, 20000):
            raw = bytes(rng.integers(0, syms, n, dtype=np.uint8))
            assert _same(ff, raw, GRID if n < 20000 else GRID[syms::5], "alphabet of %d" % syms) > 0


def test_repeat_offset_loop_and_matches_into_the_end(ff):
    rng = np.random.default_rng(8)
    for blk_len in (1, 2, 3, 4, 5, 7, 8, 9, 31, 64, 129, 500, 900):
        blk = rng.bytes(blk_len)
        for k in (2, 3, 40):
            raw = blk * k
            if len(raw) >= 16: _same(ff, raw, GRID, "block of %d x %d" % (blk_len, k))
        # two blocks interleaved: both repeat offsets in use
        other = rng.bytes(blk_len + 3)
        raw = (blk + other + blk + blk + other + other + blk) * 3
        if len(raw) >= 16: _same(ff, raw, GRID, "two blocks of %d" % blk_len)
    for n in (64, 100, 1000, 131072):
        assert _same(ff, b"a" * n, GRID if n < 131072 else GRID[::9], "one byte") > 0
    # the forward count reaching the end of the source: the second copy of a block ends 0 .. 9 bytes before it
    blk = rng.bytes(100)
    for j in range(10):
        for tail in (b"", b"\x01" * j):
            raw = blk + rng.bytes(50) + blk[: 100 - j] + tail
            assert _same(ff, raw, GRID, "match into the last bytes") > 0


def test_general_inputs(ff, corpus):
    from tests.test_emu_kernels import _flat_search_inputs
    rng = np.random.default_rng(9)
    raws = [r for r in _flat_search_inputs(corpus) if len(r) >= 8]
    raws += [corpus.frame_bytes(int(rng.integers(0, 500)))[: int(rng.integers(64, 131073))] for _ in range(24)]
    total = 0
    for i, raw in enumerate(raws):
        total += _same(ff, raw, GRID[i % 10::10], "input %d" % i)
    assert total > 100000


def test_launch_numbers_in_a_table_that_is_never_zeroed_again(ff, corpus):
    """one allocation, zeroed once, launches 1 .. 63 each with another source (and other parameters) in the slot: cells of earlier launches read as empty"""
    rng = np.random.default_rng(10)
    table = np.zeros(1 << 15, dtype=np.uint32)
    for epoch in range(1, 64):
        m, t, h, p = GRID[(epoch * 7) % len(GRID)]
        kind = epoch % 3
        n = int(rng.integers(64, 40000))
        raw = corpus.frame_bytes(epoch % 5)[:n] if kind == 0 else (rng.bytes(300) * (n // 300 + 1))[:n] if kind == 1 else bytes(rng.integers(0, 3, n, dtype=np.uint8))
        got = ff.flat(raw, h, m, t, p, epoch=epoch, table=table)
        assert np.array_equal(got, ff.serial(raw, h, m, t)), (epoch, m, t, h, p, n)
    assert int((table >> 26).max()) == 63 and np.count_nonzero(table & 0x3FFFF) > 4096          # (the launches really shared the cells)
