"""The greedy search with the row match finder (ze_greedy_row, what level 5 runs on sources of 16 385 ... 131 072 bytes) on the host, sequence by sequence against
libzstd 1.5.7's own parse (ZSTD_generateSequences): litLength, matchLength and the resolved offset of every sequence, and the last literals. For each aimed
source the test first asserts, from libzstd's sequences, that the source has the property it is there for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import greedy_sources as gs

HERE = os.path.dirname(os.path.abspath(__file__))


class _Seq(C.Structure):          # ZSTD_Sequence (zstd.h)
    _fields_ = [("offset", C.c_uint), ("litLength", C.c_uint), ("matchLength", C.c_uint), ("rep", C.c_uint)]


@pytest.fixture(scope="module")
def lz():
    """libzstd 1.5.7's sequences for one source: [(litLength, matchLength, offset)], last literals"""
    from tests import reflib
    if not reflib.have_ref():
        pytest.skip("no libzstd 1.5.7 available")
    ref = reflib.RefZstd()
    L = ref.lib
    L.ZSTD_sequenceBound.restype = C.c_size_t; L.ZSTD_sequenceBound.argtypes = [C.c_size_t]
    L.ZSTD_generateSequences.restype = C.c_size_t; L.ZSTD_generateSequences.argtypes = [C.c_void_p, C.POINTER(_Seq), C.c_size_t, C.c_char_p, C.c_size_t]

    def run(raw, **params):
        ctx = L.ZSTD_createCCtx()
        try:
            L.ZSTD_CCtx_setParameter(ctx, 100, 5)
            for k, v in params.items():
                assert not L.ZSTD_isError(L.ZSTD_CCtx_setParameter(ctx, ref.PARAM_IDS[k], v))
            cap = L.ZSTD_sequenceBound(len(raw))
            buf = (_Seq * cap)()
            n = L.ZSTD_generateSequences(ctx, buf, cap, raw, len(raw))
            assert not L.ZSTD_isError(n), L.ZSTD_getErrorName(n)
            a = np.frombuffer(buf, dtype=np.uint32, count=4 * n).reshape(n, 4)
            assert n >= 1 and a[-1, 0] == 0 and a[-1, 2] == 0 and not ((a[:-1, 0] == 0) | (a[:-1, 2] == 0)).any(), "one block: one delimiter, at the end"
            return a[:-1, [1, 2, 0]].astype(np.int64), int(a[-1, 1])
        finally:
            L.ZSTD_freeCCtx(ctx)

    return run


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_greedy_row") / "libzhip_emu_greedy_row.so")
    d = os.path.join(HERE, "emu")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + d, "-w", "-o", out, os.path.join(d, "zhemu.cpp"), os.path.join(d, "emu_greedy_row.cpp")])
    lib = C.CDLL(out)
    lib.emu_greedy_row.restype = C.c_int64
    lib.emu_greedy_row.argtypes = [C.POINTER(C.c_uint8), C.c_uint32] + [C.c_int] * 7 + [C.POINTER(C.c_uint64)]

    lib.emu_greedy_frames.restype = C.c_int
    lib.emu_greedy_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32]

    def frames(raws, level=5, checksum=False, **params):
        """whole frames through the greedy match kernel and the entropy kernel under emulation: (frames, statuses)"""
        n = len(raws)
        lens = np.array([len(r) for r in raws], dtype=np.uint64)
        caps = lens + (lens >> np.uint64(8)) + np.uint64(64 + 32)
        ssegs = np.zeros((n, 2), dtype=np.uint64); ssegs[:, 1] = lens; ssegs[1:, 0] = np.cumsum(lens)[:-1]
        dsegs = np.zeros((n, 2), dtype=np.uint64); dsegs[:, 1] = caps; dsegs[1:, 0] = np.cumsum(caps)[:-1]
        src = np.frombuffer(b"".join(raws), dtype=np.uint8).copy()
        dst = np.zeros(int(caps.sum()), dtype=np.uint8)
        sizes = np.zeros(n, dtype=np.uint64); st = np.full(n, -1, dtype=np.int32)
        ov = np.array([params.get(k, 0) for k in ("window_log", "chain_log", "hash_log", "search_log", "min_match", "target_length", "strategy")], dtype=np.int32)
        lib.emu_greedy_frames(src.ctypes.data, ssegs.ctypes.data, n, dst.ctypes.data, dsegs.ctypes.data, sizes.ctypes.data, st.ctypes.data, level, ov.ctypes.data, 1 | (2 if checksum else 0), 3)
        return [dst[int(dsegs[i, 0]): int(dsegs[i, 0] + sizes[i])].tobytes() for i in range(n)], st.tolist()

    def run(raw, **params):
        """the search's sequences with their offsets resolved against the repeat-offset history, and the last literals; an int when the row is refused"""
        row = dict(gs.LEVEL5_ROW); row.update(params)
        src = np.frombuffer(raw, dtype=np.uint8).copy()               # exactly len(raw) bytes: the search may not read past them
        seqs = np.zeros(len(raw) // 4 + 8, dtype=np.uint64)
        n = lib.emu_greedy_row(src.ctypes.data_as(C.POINTER(C.c_uint8)), len(raw), row["window_log"], row["chain_log"], row["hash_log"], row["search_log"], row["min_match"],
                               row["target_length"], row["strategy"], seqs.ctypes.data_as(C.POINTER(C.c_uint64)))
        if n < 0: return int(n)
        q = seqs[:n]
        ofb = (q & np.uint64(0xFFFFFFF)).astype(np.int64); ll = ((q >> np.uint64(28)) & np.uint64(0x3FFFF)).astype(np.int64); ml = (q >> np.uint64(46)).astype(np.int64)
        reps = [1, 4, 8]
        out = np.zeros((n, 3), dtype=np.int64)
        for i in range(n):
            if ofb[i] > 3: off = int(ofb[i]) - 3; reps = [off, reps[0], reps[1]]
            else:
                k = int(ofb[i]) - 1 + (1 if ll[i] == 0 else 0)
                if k == 0: off = reps[0]
                elif k == 3: off = reps[0] - 1; reps = [off, reps[0], reps[1]]
                else: off = reps[k]; reps = [off] + reps[:k] + reps[k + 1:]
            out[i] = (ll[i], ml[i], off)
        return out, len(raw) - int(out[:, 0].sum() + out[:, 1].sum())

    run.frames = frames
    return run


def _same(lz, emu, raw, what, param_sets=gs.PARAM_SETS):
    total = 0
    for p in param_sets:
        want, want_last = lz(raw, **p)
        got = emu(raw, **p)
        assert not isinstance(got, int), "%s (%d bytes) %r: refused with status %d" % (what, len(raw), p, -got)
        got, got_last = got
        first = next((i for i in range(min(len(got), len(want))) if tuple(got[i]) != tuple(want[i])), min(len(got), len(want)))
        assert len(got) == len(want) and first == len(want) and got_last == want_last, "%s (%d bytes) %r: %d sequences against libzstd's %d, first difference at %d: %s against %s; last literals %d against %d" % (
            what, len(raw), p, len(got), len(want), first, got[first] if first < len(got) else None, want[first] if first < len(want) else None, got_last, want_last)
        total += len(want)
    return total


def test_sizes_around_the_tail(lz, emu, corpus):
    for n, raw in zip(gs.TAIL_SIZES, gs.tail_sources(corpus)):
        assert len(raw) == n
        want, last = lz(raw)
        assert last == 0 and want[-1][1] >= 24, ("libzstd does not find the match at the end", n, want[-3:], last)
        assert _same(lz, emu, raw, "tail") > 0
    assert _same(lz, emu, corpus.frame_bytes(9), "text, one whole block") > 1000


def test_constant_bytes(lz, emu):
    for raw in gs.constant_sources():
        want, last = lz(raw)
        assert want.tolist() == [[2, len(raw) - 2, 1]] and last == 0, want[:4]
        assert _same(lz, emu, raw, "constant") > 0


def test_lazy_skipping_and_the_skip_threshold(lz, emu):
    raw = gs.lazy_skipping_source()
    want, last = lz(raw)
    assert want.tolist() == [[9000, 1000, 8900], [2500, 40, 11000]] and last == 5000, (want, last)
    assert _same(lz, emu, raw, "lazy skipping") > 0


def test_copies_of_a_region_passed_under_lazy_skipping(lz, emu):
    raw = gs.skipped_region_source()
    want, last = lz(raw)
    assert len(want) == 0 and last == len(raw), ("libzstd finds a copy of bytes it passed under lazy skipping", want[:4])
    _same(lz, emu, raw, "skipped region")
    got, got_last = emu(raw)
    assert len(got) == 0 and got_last == len(raw)


def test_where_lazy_skipping_begins(lz, emu):
    raw, p, gap = gs.lazy_threshold_source()
    want, last = lz(raw)
    # the 64-byte match that ends the skipping, then X after Y and the gap as literals: Y (from P + 1, never inserted) is not found, X (up to P, inserted) is
    assert want.tolist() == [[4000, 64, 4000], [8 + gap, 8, 4000 + 64 + 8 + gap - (p - 7)]] and last == 13000, (p, want[:4], last)
    assert _same(lz, emu, raw, "lazy threshold") > 0


def test_first_96_and_last_32_of_a_pending_stretch(lz, emu):
    raw, probes = gs.pending_stretch_source()
    want, _ = lz(raw)
    at = np.concatenate([[0], np.cumsum(want[:, 0] + want[:, 1])[:-1]]) + want[:, 0]           # where each match starts
    assert want[0].tolist() == [1500, 600, 1500], want[:2]
    found = {int(a): (int(ml), int(off)) for a, (_, ml, off) in zip(at, want)}
    assert [found.get(pos) for pos, _ in probes] == [(8, off) for _, off in probes], ("libzstd's offsets for the probes", [found.get(pos) for pos, _ in probes], probes)
    assert _same(lz, emu, raw, "pending stretch") > 0


def test_pending_stretch_of_385_and_of_384(lz, emu):
    for raw, pos, off in gs.skip_threshold_sources():
        want, _ = lz(raw)
        at = np.concatenate([[0], np.cumsum(want[:, 0] + want[:, 1])[:-1]]) + want[:, 0]
        found = {int(a): (int(ml), int(o)) for a, (_, ml, o) in zip(at, want)}
        assert want[0][0] == 1500 and want[0][2] == 1500 and found.get(pos) == (8, off), ("libzstd's offset for the probe", want[:3], pos, off, found.get(pos))
        assert _same(lz, emu, raw, "pending stretch at the threshold") > 0


def test_repeat_offset_at_the_last_position(lz, emu, corpus):
    raw = gs.last_position_source(corpus)
    want, last = lz(raw)
    assert want[-1][0] == 0 and want[-1][1] == 12 and last == 4, ("libzstd does not take the repeat offset at ilimit", want[-3:], last)
    assert _same(lz, emu, raw, "last position") > 0


def test_full_rows_and_the_attempt_cap(lz, emu):
    plain, varied = gs.full_row_sources()
    gram = plain[:4]
    for raw in (plain, varied):
        at = gs.gram_positions(raw, gram)
        assert len(at) - 1 >= 17 and len(raw) > 16384, "at least 17 occurrences before the last: the row wraps past slot 0, more than 8 equal tags"
    want, _ = lz(varied)
    assert len(want) >= 17 and any(ml > 4 for _, ml, _ in want.tolist()), want[:8]
    assert len({off for _, _, off in want.tolist()}) > 2, "libzstd's sequences on the varied source are not all repeat offsets"
    assert _same(lz, emu, plain, "full row") > 0
    assert _same(lz, emu, varied, "full row, varied") > 0


def test_repeat_offset_loop(lz, emu):
    raw = gs.repeat_offset_source()
    assert len(raw) > 16384
    want, _ = lz(raw)
    assert sum(1 for ll, _, _ in want.tolist() if ll == 0) >= 20, "libzstd takes the second repeat offset right after a match"
    assert _same(lz, emu, raw, "repeat offsets") > 0


def test_corpus_classes(lz, emu):
    raws = gs.corpus_sources()
    assert len(raws) == 28 and {len(r) for r in raws} == {20000, 131072}
    total = 0
    for i, raw in enumerate(raws):
        total += _same(lz, emu, raw, "corpus source %d" % i)
    assert total > 100000


def test_out_of_scope_rows_are_refused(emu, corpus):
    raw = corpus.frame_bytes(9)
    assert emu(raw[:20000], search_log=5) == -40 and emu(raw[:20000], search_log=6) == -40                # rows of 32 and 64 entries
    assert emu(raw[:16384], window_log=14) == -40 and emu(raw[:20000], window_log=14) == -40              # the hash-chain finder
    assert emu(raw, hash_log=18) == -40                                                                 # tables above hashLog 17: refused before the search
    assert emu(raw[:40000], window_log=15) == -40                                                        # a window that does not cover the source
    assert emu(raw, strategy=4) == -40 and emu(raw, strategy=5) == -40                                    # lazy, lazy2


def test_whole_frames_through_the_emulated_kernels(emu, corpus):
    """the greedy match kernel (ze_match_body<true>) and the entropy kernel on the host wave emulator: frames byte for byte libzstd's at level 5 and with explicit greedy
    parameters, with and without the checksum trailer; in the same batch sources of 16 384 bytes and less, and of several blocks, refused with status 40 at their own index"""
    from tests import reflib
    if not reflib.have_ref():
        pytest.skip("no libzstd 1.5.7 available")
    ref = reflib.RefZstd()
    text = corpus.frame_bytes(9)
    aimed = [r for name, r in gs.aimed_sources(corpus) if len(r) < 60000 or name in ("text 131072", "constant 131072")]
    raws = aimed[:6] + [text[:16384], b"abc", text[:50]] + aimed[6:] + [text + text[:1]]
    for checksum, kw in ((False, {}), (True, {}), (False, dict(strategy=3, search_log=4, min_match=3)), (True, dict(strategy=3, search_log=1, min_match=6))):
        got, st = emu.frames(raws, checksum=checksum, **kw)
        flags = reflib.DEFAULT_FLAGS | (reflib.F_CHECKSUM if checksum else 0)
        for i, r in enumerate(raws):
            if len(r) <= 16384 or len(r) > 131072:
                assert st[i] == 40, (i, len(r), st[i])
                continue
            want = ref.compress_advanced(r, level=5, flags=flags, **kw) if kw else ref.compress(r, level=5, flags=flags)
            assert st[i] == 0 and got[i] == want, (kw, checksum, i, len(r), st[i], len(got[i]), len(want))
