"""match_finder="auto" (ZHIP_FINDER_AUTO: ze_classify_body and the partition / gather / scatter kernels of zhip_encode_auto.hpp, with the literals-only kernel and the
default finder's kernels behind them) on the 64-fiber host emulator (tests/emu/emu_auto_finder.cpp). Choice bytes and statistics must equal the numpy model's
(tests/auto_model.py) for every source, every frame must be libzstd 1.5.7's for the chosen mode -- ZSTD_compressSequences with the list that is only the block delimiter, or
ZSTD_compress2 --, and status, size and the first failing index must be what the two pure finders give. The rule itself is judged elsewhere, against libzstd's sizes
(tests/test_auto_rule.py). Also the plan, the refusals and the stand-alone bounds program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import auto_model as am
from tests import planes_model as pm
from tests import reflib

HERE = os.path.dirname(os.path.abspath(__file__))
PARAM_NAMES = ("window_log", "chain_log", "hash_log", "search_log", "min_match", "target_length", "strategy")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("emu_auto_finder")), "libzhip_emu_auto_finder.so")
    d = os.path.join(HERE, "emu")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + d, "-w", "-o", out, os.path.join(d, "zhemu.cpp"), os.path.join(d, "emu_auto_finder.cpp")])
    lib = C.CDLL(out)
    lib.emu_auto_frames.restype = C.c_int
    lib.emu_auto_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emu_auto_classify.restype = None
    lib.emu_auto_classify.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    lib.emu_auto_bound.restype = C.c_uint64
    lib.emu_auto_bound.argtypes = [C.c_uint64]
    lib.emu_auto_plan.restype = None
    lib.emu_auto_plan.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_void_p]
    return lib


def _layout(raws):
    n = len(raws)
    lens = np.array([len(r) for r in raws], dtype=np.uint64)
    ssegs = np.zeros((n, 2), dtype=np.uint64); ssegs[:, 1] = lens; ssegs[1:, 0] = np.cumsum(lens)[:-1]
    joined = b"".join(raws)
    src = np.frombuffer(joined, dtype=np.uint8).copy() if joined else np.zeros(1, dtype=np.uint8)      # every source back to back, the last one ends at the buffer's end
    return src, ssegs


def classify(lib, raws, blocks=3, chunk=0):
    src, ssegs = _layout(raws)
    choice = np.full(len(raws), 7, dtype=np.uint8); stats = np.full((len(raws), 4), 0xA5A5A5A5, dtype=np.uint32)
    lib.emu_auto_classify(src.ctypes.data, ssegs.ctypes.data, len(raws), choice.ctypes.data, stats.ctypes.data, blocks, chunk)
    return choice.tolist(), stats.tolist()


def frames(lib, raws, finder="auto", level=3, checksum=False, dictionary=False, blocks=3, echunk=0, caps=None, **params):
    """one batch under the emulated finder: (frames, statuses, choice bytes, statistics, (match, literals-only, classify) launches). Destinations are slots of exactly
    zhip_compress_bound bytes (or caps[i]), back to back. Raises RuntimeError where the call as a whole is refused."""
    n = len(raws)
    src, ssegs = _layout(raws)
    cap = np.array([lib.emu_auto_bound(len(r)) if caps is None or caps[i] is None else caps[i] for i, r in enumerate(raws)], dtype=np.uint64)
    dsegs = np.zeros((n, 2), dtype=np.uint64); dsegs[:, 1] = cap; dsegs[1:, 0] = np.cumsum(cap)[:-1]
    dst = np.zeros(int(cap.sum()) + 1, dtype=np.uint8)
    sizes = np.zeros(n, dtype=np.uint64); st = np.full(n, -1, dtype=np.int32)
    ov = np.array([params.get(k, 0) for k in PARAM_NAMES], dtype=np.int32)
    choice = np.full(n, 7, dtype=np.uint8); stats = np.zeros((n, 4), dtype=np.uint32); launches = np.zeros(3, dtype=np.uint32)
    flags = 1 | (2 if checksum else 0) | (8 if dictionary else 0)
    rc = lib.emu_auto_frames(src.ctypes.data, ssegs.ctypes.data, n, dst.ctypes.data, dsegs.ctypes.data, sizes.ctypes.data, st.ctypes.data, level, ov.ctypes.data, flags, blocks,
                             echunk, {"libzstd": 0, "none": 2, "auto": 4}[finder], choice.ctypes.data, stats.ctypes.data, launches.ctypes.data)
    if rc == 6:
        raise RuntimeError("the call is refused")
    assert rc == 0, rc
    out = [dst[int(dsegs[i, 0]): int(dsegs[i, 0] + sizes[i])].tobytes() for i in range(n)]
    return out, st.tolist(), choice.tolist(), stats.tolist(), tuple(int(x) for x in launches)


def _flags(checksum):
    return reflib.F_CONTENTSIZE | (reflib.F_CHECKSUM if checksum else 0) | reflib.F_DICTID


def libzstd_frame(ref, raw, choice, level=3, checksum=False):
    if choice == am.LITERALS:
        return ref.compress_sequences(raw, [], len(raw), level=level, flags=_flags(checksum))
    return ref.compress(raw, level=level, flags=_flags(checksum))


def hold(lib, ref, named, level=3, checksum=False, **kw):
    """the batch under "auto": model's choices and statistics, libzstd's frames for them, decodable"""
    raws = [r for _, r in named]
    got, st, choice, stats, launches = frames(lib, raws, level=level, checksum=checksum, **kw)
    for (name, raw), f, s, ch, sv in zip(named, got, st, choice, stats):
        want_ch, want_stats = am.classify(raw)
        assert (ch, sv) == (want_ch, want_stats), (name, len(raw), ch, sv, want_ch, want_stats)
        assert s == 0, (name, s)
        assert f == libzstd_frame(ref, raw, ch, level, checksum), (name, len(raw), ch)
        assert ref.decompress(f, len(raw)) == raw, name
    return choice, launches


@pytest.fixture(scope="module")
def classes(corpus):
    """one source of each class of DESIGN.md 4.2's table at 131 072 bytes"""
    text = am.text_frames(2)
    bf = pm.planes(am.bf16_values(), 2, am.BLOCK_MAX)
    sums = pm.planes(am.sums_values(), 8, am.BLOCK_MAX)
    from tests import delta_model as dm
    dsums = dm.planes(am.sums_values(), 8, am.BLOCK_MAX)
    srt = pm.planes(am.sorted_values(), 4, am.BLOCK_MAX)
    return [("text 0", text[0]), ("text 1", text[1]), ("bf16 mantissa plane", bf[0]), ("bf16 exponent plane", bf[1]), ("sums plane 1", sums[1]), ("sums plane 2", sums[2]),
            ("sums plane 3", sums[3]), ("sums plane 4", sums[4]), ("delta plane 1", dsums[1]), ("sorted plane 2", srt[2])]


def front_only(n=am.BLOCK_MAX):
    """redundancy that lies wholly in front of the first window and of the stretch that feeds it: a 512-byte piece repeated up to there, noise behind"""
    first, _, start, _ = am.windows(n)[0]
    rng = np.random.default_rng(5)
    piece = rng.integers(0, 256, 512, dtype=np.uint8).tobytes()
    head = (piece * (first // 512 + 1))[:first - 64]
    return head + rng.integers(0, 256, n - len(head), dtype=np.uint8).tobytes()


def sized(classes):
    """text and the exponent plane at every length where the classifier or the sample layout takes another path"""
    text, expo = classes[0][1], classes[3][1]
    lens = [0, 1, 6, 7, am.MIN - 1, am.MIN, am.MIN + 1, 66, 67, 68, 127, 128, 129, am.ALL - 1, am.ALL, am.ALL + 1, am.ALL + am.STRIDE - 1, 5 * am.WIN + 517]
    return [("text %d" % n, text[:n]) for n in lens] + [("exponent %d" % n, expo[1000:1000 + n]) for n in lens if n >= am.MIN - 1]


def test_model_layout_is_what_the_header_says():
    """the sample: all of a source up to 8 192 bytes; above, four windows of 1 536 bytes that do not overlap, the last one ending at the source's end, each fed from up
    to 4 096 bytes in front of it at stride 8 -- at most 14 KiB of a 131 072-byte source, an eighth of it or less"""
    assert am.MIN <= 64
    assert am.windows(am.ALL) == [(0, 0, 0, am.ALL)]
    for n in (am.ALL + 1, 20000, am.BLOCK_MAX):
        w = am.windows(n)
        assert len(w) == am.NWIN and w[-1][2] + w[-1][3] == n
        assert all(a[2] + a[3] <= b[0] for a, b in zip(w, w[1:])) and all(f + c * am.STRIDE == s and s - f <= am.FEED for f, c, s, _ in w)
        assert sum(ln + 4 * c for _, c, _, ln in w) * 8 <= max(n, am.BLOCK_MAX)
    assert [am.log2fp(x) for x in (1, 2, 3, 1024, 6144)] == [0, 256, 406, 2560, 3222]


def test_classes_at_one_block(lib, ref, classes):
    choice, launches = hold(lib, ref, classes)
    assert choice == [0, 0, 1, 1, 0, 0, 0, 0, 1, 0], choice          # (sums plane 4 is one byte repeated: the search, five bytes worse than the literals-only frame)
    assert launches == (1, 1, 1)


def test_every_length_where_a_path_changes(lib, ref, classes):
    named = sized(classes)
    choice, _ = hold(lib, ref, named, checksum=True)
    assert all(ch == 0 for (name, raw), ch in zip(named, choice) if len(raw) < am.MIN)
    one = classify(lib, [r for _, r in named], blocks=1)              # one wave takes every source in turn; launches of 5 sources
    cut = classify(lib, [r for _, r in named], blocks=4, chunk=5)
    assert one == cut and one[0] == choice


def test_one_block_and_above(lib, ref, classes):
    """131 072 bytes are sampled; 131 073 go to the search unsampled, and the search serves them (two blocks)"""
    expo = classes[3][1]
    named = [("exponent 131072", expo), ("exponent 131073", expo + expo[:1]), ("text 131073", classes[0][1] + b"x"), ("exponent 300000", (expo * 3)[:300000])]
    choice, _ = hold(lib, ref, named, checksum=True)
    assert choice == [1, 0, 0, 0]


def test_redundancy_in_front_of_the_first_window_is_not_seen(lib, ref):
    raw = front_only()
    choice, _ = hold(lib, ref, [("front only", raw)])
    assert choice == [1]
    lit, search = am.both_sizes(ref, raw)
    assert search < lit                                                 # what a bounded sample costs: the search would have won here


def test_batches_of_one_kind_launch_nothing_of_the_other(lib, ref, classes):
    expo, text = classes[3][1], classes[0][1]
    floats = [("exponent %d" % k, expo[k * 9000:k * 9000 + 9000 + k]) for k in range(5)]
    texts = [("text %d" % k, text[k * 9000:k * 9000 + 9000 + k]) for k in range(5)]
    choice, launches = hold(lib, ref, floats)
    assert choice == [1] * 5 and launches == (0, 1, 1)
    choice, launches = hold(lib, ref, texts)
    assert choice == [0] * 5 and launches == (1, 0, 1)
    choice, launches = hold(lib, ref, floats[:1])
    assert choice == [1] and launches == (0, 1, 1)


def test_status_sizes_and_first_failure_are_the_pure_finders(lib, classes):
    """a mixed batch with destinations too small scattered among served ones: every source's status and size are what the pure finder of its choice gives AT ITS OWN
    INDEX, and so is the lowest failing index; over several tiles of the partition and several chunks"""
    expo, text = classes[3][1], classes[0][1]
    raws, caps = [], []
    for k in range(75):
        raw = (expo if k % 3 else text)[k * 1500:k * 1500 + 900 + 13 * k]
        raws.append(raw); caps.append(8 if k in (7, 8, 30, 74) else None)
    raws += [b"", b"abc"]; caps += [None, None]
    auto, st, choice, _, launches = frames(lib, raws, checksum=True, caps=caps, echunk=32)
    assert [am.classify(r)[0] for r in raws] == choice and 0 < sum(choice) < len(choice)
    assert launches[2] == 3 and launches[1] == (sum(choice) + 31) // 32
    pure = {0: frames(lib, raws, finder="libzstd", checksum=True, caps=caps), 1: frames(lib, raws, finder="none", checksum=True, caps=caps)}
    for i, ch in enumerate(choice):
        assert (st[i], auto[i]) == (pure[ch][1][i], pure[ch][0][i]), (i, ch, st[i])
    assert [i for i, s in enumerate(st) if s] == [7, 8, 30, 74] and all(st[i] == 70 for i in (7, 8, 30, 74))
    again = frames(lib, raws, checksum=True, caps=caps, blocks=1)
    assert (again[0], again[1], again[2]) == (auto, st, choice)


def test_refusals(lib, classes):
    """the call's refusals are ze_none_refusal's: a dictionary, or a level whose one-block row is not fast / double-fast"""
    text = classes[0][1]
    for kw in (dict(level=5), dict(level=3, strategy=3, search_log=4), dict(level=3, dictionary=True)):
        with pytest.raises(RuntimeError):
            frames(lib, [text[:40000]], **kw)
    for level in (1, 4, -1):
        got, st, choice, _, _ = frames(lib, [text[:40000], classes[3][1][:40000]], level=level)
        assert st == [0, 0] and choice == [0, 1], level


def test_plan(lib):
    """ze_auto_plan: classify launches of 65 536 sources on the kernel's resident waves, gather / scatter a lane per source, the scratch 49 bytes a source and a header"""
    def plan(n, num_cu=256, per_cu=9, echunk=0):
        out = np.zeros(4, dtype=np.uint64)
        lib.emu_auto_plan(n, num_cu, per_cu, echunk, out.ctypes.data)
        return tuple(int(x) for x in out)
    assert plan(1) == (1, 1, 1, 64 + 16 + 16 + 16 + 16 + 8 + 16)
    assert plan(65536)[:3] == (65536, 256 * 9, 1024) and plan(65537)[:3] == (65536, 256 * 9, 1025)
    assert plan(1 << 20)[:3] == (65536, 256 * 9, 2048) and plan(1 << 20)[3] == 64 + 49 * (1 << 20)
    assert plan(1000, num_cu=8, per_cu=4, echunk=100)[:3] == (100, 32, 16)


def test_bounds_program_is_clean(tmp_path, classes):
    """AddressSanitizer + UBSan over the classifier with every source in a heap block of EXACTLY its size -- the last window ends at the allocation's end -- as a
    stand-alone program (tests/emu/auto_bounds_main.cpp); nothing sanitized is loaded into this process. The program also compresses each source under the emulated
    "auto" into an exactly zhip_compress_bound-sized block."""
    exe = str(tmp_path / "auto_bounds")
    subprocess.check_call(["sh", os.path.join(HERE, "emu", "build_auto_bounds.sh"), exe])
    named = sized(classes) + [classes[3], classes[6], ("exponent 131073", classes[3][1] + b"\0")]
    files = []
    for i, (name, raw) in enumerate(named):
        p = str(tmp_path / ("%03d.bin" % i))
        open(p, "wb").write(raw)
        files.append(p)
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.startswith("ok: %d sources" % len(named)), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = [int(x) for x in r.stdout.split("choices:")[1].split()]
    assert got == [am.classify(raw)[0] for _, raw in named]
