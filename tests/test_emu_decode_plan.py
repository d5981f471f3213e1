"""The launch plan of device decompress (python-zstandard_amd/csrc/zhip_decode_plan.hpp) on the CPU: every decision zhip_decompress_batch_device reads -- the several-block mode,
the side stream, K0, the lane pass, chunk and slots, the arena budget, every reservation, every grid, the form of K1, K2 and K3 of a chunk -- at both sides of every switch point.

Two checks. (1) Equality with tests/golden/decode_plan.json, which was recorded from the decisions of the commit BEFORE the plan existed (that commit's lines of
zhip_decompress_batch_device pasted verbatim into a function of the same inputs, its launches behind a macro that notes kernel and grid), not from the plan's code: a SHA-256 of
the rows of the WHOLE cross product of the axes below (77 520 cases, one digest per knob variant, device and dictionary), and some 400 cases around each switch spelled out,
which say WHAT differs where a digest does. (2) The switch points the project documents (tests/test_gpu_launch_shapes.py's docstrings, the plan's comments) asserted directly, so
that a fixture regenerated from wrong code cannot hide them.

The device shape is an input: 256 CUs, or 8 so that every grid clamp bites at small batches, and for the per-CU wave counts of the generic kernel, K1 and K3 the fallbacks
zhip_ctx_create uses when its occupancy query fails (8, 8, 16) -- stand-ins, no real occupancy is claimed. K2's and K1b's workgroups per CU are the real ones: a CU's LDS over
the kernels' own structures. ZHIP_PLAN_SO names another library with the same entry (how the fixture was recorded: python -m tests.test_emu_decode_plan --record)."""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

import pytest

from tests import emulib

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "decode_plan.json")

FIELDS = ["tooLarge", "mb", "side", "pre", "k1Lanes", "chunk", "slots", "nChunks", "nslot", "arenaBudget16", "arenaBytes",
          "scratchBytes", "counterBytes", "basesBytes", "metaBytes", "litBytes", "countersBytes", "fallbackBytes", "fseBytes", "orderBytes", "hufBytes", "orderLitBytes",
          "preBytes", "itemFrameBytes", "itemRepsBytes", "frameRecsBytes", "genericGrid"]
CHUNK_FIELDS = ["itemCap", "items", "k1", "k2", "k3", "gPre", "gLanes", "g1", "gBin", "gHuf", "g2", "g3", "gCheck"]
ALL_FIELDS = FIELDS + ["first." + f for f in CHUNK_FIELDS] + ["last." + f for f in CHUNK_FIELDS]
K1_PLAIN, K1_LANES, K1_MB = range(3)
K3_EXEC, K3_PROF, K3_DICT, K3_MB, K3_MB_DICT = range(5)
D_NONE, D_CONTENT, D_ENTROPY = range(3)

BLOCK = 1 << 17
ZP_SEQ_STRIDE, ZP_LIT_STRIDE = 45056 * 8, BLOCK + 256          # zhip_format.hpp
SWITCHES = (1, 1, 3)                    # ZHIP_SIDE, ZHIP_K0, ZHIP_NSLOT as the product builds
DEV_BIG, DEV_SMALL = (256, 8, 8, 16), (8, 8, 8, 16)          # numCU, then waves per CU of the generic kernel, K1, K3
DEVS = [DEV_BIG, DEV_SMALL]
KNOB_NAMES = ["k0Min", "dchunk", "nslot", "k3PerCU"]
KNOB_DEFAULT = dict(k0Min=6144, dchunk=65536, nslot=2, k3PerCU=0)
KNOBS = [{}, dict(k0Min=0), dict(k0Min=10 ** 9), dict(dchunk=32768), dict(k3PerCU=24)]          # (dchunk 32 768: build_variants.sh's dchunk32k)

NS = [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 6143, 6144, 10922, 10923, 65535, 65536, 65537, 131073, 196608, 262145]
HINTS = [0, 1, 256, 4096, 16384, 16385, 131071, 131072, 131073, 262144, 262145, 1 << 20, (1 << 31) - 1, 1 << 31]


def is_mb(hint):
    return BLOCK < hint <= (1 << 31) - 1


def slot_hints(n, hint):
    """the host API's slot hint is read in the several-block mode only; the last one trips "frame too large for the block arenas\""""
    return [0, n, 2 * n + 2, 6 * n, n << 31] if is_mb(hint) else [0]


def case(n, hint=0, slots=0, host=0, d=D_NONE, prof=0, knobs=None, dev=DEV_BIG):
    return dict(n=n, hint=hint, slots=slots, host=host, dict=d, prof=prof, knobs=knobs or {}, dev=dev)


def product_slices():
    """the whole cross product, a slice per (knob variant, device, dictionary)"""
    for ki, kv in enumerate(KNOBS):
        for vi, dev in enumerate(DEVS):
            for d in (D_NONE, D_CONTENT, D_ENTROPY):
                yield "knobs%d.dev%d.dict%d" % (ki, vi, d), (case(n, hint, s, host, d, prof, kv, dev) for n in NS for hint in HINTS for s in slot_hints(n, hint)
                                                             for host in (0, 1) for prof in (0, 1))


def spelled_cases():
    """the cases whose rows the fixture spells out: each axis swept around the points where the others' switches lie"""
    out = [case(n, hint, host=host) for n in NS for hint in (0, 4096, 16385, 262144) for host in (0, 1)]                             # frames x the four kinds of hint
    out += [case(n, hint, host=host) for n in (1, 4096, 65537) for hint in HINTS for host in (0, 1)]                                 # the size hint
    out += [case(n, hint, s, host=1) for n in (1, 1025, 10923, 65537) for hint in (131073, 1 << 20) for s in slot_hints(n, hint)]     # the host API's slot hint
    out += [case(n, hint, d=d, prof=prof) for n in (1, 6144, 65537) for hint in (0, 4096, 262144) for d in (D_NONE, D_CONTENT, D_ENTROPY) for prof in (0, 1)]      # K1's and K3's forms
    out += [case(n, hint, knobs=kv) for kv in KNOBS[1:] for n in (1, 6143, 6144, 32769, 65537) for hint in (0, 262144)]               # the knobs
    out += [case(n, hint, host=host, dev=DEV_SMALL) for n in NS[:12] for hint in (0, 262144) for host in (0, 1)]                     # eight CUs: the grid clamps
    return out


def digest(lib, cases):
    h = hashlib.sha256()
    for c in cases:
        h.update((",".join(map(str, lib.row(**c))) + "\n").encode())
    return h.hexdigest()


class PlanLib:
    def __init__(self, path=None):
        path = path or os.environ.get("ZHIP_PLAN_SO") or emulib.EMU_SO
        if not os.path.exists(path):
            emulib.build()
        self.lib = C.CDLL(path)
        self.lib.emu_decode_plan.restype = C.c_int
        self.sw = (C.c_int64 * 3)(*SWITCHES)
        self.out = (C.c_uint64 * 64)()

    def row(self, n, hint=0, slots=0, host=0, dict=D_NONE, prof=0, knobs=None, dev=DEV_BIG):
        kn = KNOB_DEFAULT.copy(); kn.update(knobs or {})
        cnt = self.lib.emu_decode_plan(C.c_uint64(n), C.c_uint64(hint), C.c_uint64(slots), C.c_int(host), C.c_int(dict), C.c_int(prof),
                                       (C.c_int64 * 4)(*[kn[k] for k in KNOB_NAMES]), (C.c_int64 * 4)(*dev), self.sw, self.out)
        assert cnt == len(ALL_FIELDS), cnt
        return list(self.out[:cnt])

    def plan(self, n, **kw):
        return dict(zip(ALL_FIELDS, self.row(n, **kw)))

    def host_hint(self, lens, blocks):
        out = (C.c_uint64 * 3)()
        self.lib.emu_decode_host_hint((C.c_uint64 * len(lens))(*lens), (C.c_uint32 * len(lens))(*blocks), C.c_uint64(len(lens)), out)
        return tuple(out)


@pytest.fixture(scope="module")
def lib():
    return PlanLib()


def test_plan_is_the_parent_commits_decisions(lib):
    fx = json.load(open(FIXTURE))
    assert fx["fields"] == ALL_FIELDS
    spelled = spelled_cases()
    assert len(spelled) == len(fx["expected"]) and len(spelled) > 350
    bad = []
    for c, want in zip(spelled, fx["expected"]):
        got = lib.row(**c)
        if got != want:
            bad.append((c, {f: (w, g) for f, w, g in zip(ALL_FIELDS, want, got) if w != g}))
    assert not bad, "%d of %d cases differ from the recorded decisions (field: (recorded, plan)); the first: %r" % (len(bad), len(spelled), bad[:3])
    got = {name: digest(lib, cases) for name, cases in product_slices()}
    assert len(got) == 30 and got == fx["product_sha256"], "slices of the whole cross product that differ from the recorded decisions: %r" % sorted(k for k in got if got[k] != fx["product_sha256"].get(k))


# ---- the documented switch points, stated directly
def test_several_block_mode_between_a_block_and_2_to_the_31(lib):
    for hint, mb in ((BLOCK, 0), (BLOCK + 1, 1), ((1 << 31) - 1, 1), (1 << 31, 0), (0, 0)):
        p = lib.plan(1024, hint=hint)
        assert p["mb"] == mb and p["first.k1"] == (K1_MB if mb else K1_PLAIN) and p["first.k2"] == mb and (p["first.itemCap"] != 0) == bool(mb), hint


def test_side_stream_and_slots(lib):
    """K1b beside K2 unless the host pipeline calls or the frames are small (1 ... 16 384); with it one slot; without, small frames get up to three slots, others two;
    never more slots than chunks"""
    for host, hint in itertools.product((0, 1), HINTS):
        small = 1 <= hint <= 16384
        side = int(not host and not small)
        for n, chunks in ((1, 1), (65537, 2), (262145, 5)):
            if is_mb(hint):
                continue          # (the several-block mode's chunks are counted below)
            p = lib.plan(n, hint=hint, host=host)
            assert p["side"] == side and p["nChunks"] == chunks and p["nslot"] == (1 if side else min(chunks, 3 if small else 2)), (host, hint, n)
        if is_mb(hint):
            p = lib.plan(262145, hint=hint, host=host)
            assert p["side"] == side and p["nChunks"] > 2 and p["nslot"] == (1 if side else 2)


def test_frames_per_chunk(lib):
    """65 536 frames; in the several-block mode 65 536 block slots at 2 per 128 KiB + 2 a frame -- 10 922 frames at a 256 KiB hint --, or with the host API's slot hint
    n x 32 768 / slotsHint + 1: half the pool for what the chunk is expected to use"""
    assert lib.plan(65536)["nChunks"] == 1 and lib.plan(65537)["chunk"] == 65536 and lib.plan(65537)["nChunks"] == 2
    assert lib.plan(65537, knobs=dict(dchunk=32768))["chunk"] == 32768
    p = lib.plan(10923, hint=256 << 10)
    assert p["chunk"] == 10922 and p["slots"] == 65536 and p["nChunks"] == 2 and p["first.itemCap"] == 65536 and p["last.itemCap"] == 12
    assert lib.plan(10922, hint=256 << 10)["nChunks"] == 1
    assert lib.plan(1, hint=256 << 10)["slots"] == 12          # (a chunk of few frames has no pool to lean on: twice its share)
    for n, s in ((65537, 65537), (65537, 6 * 65537), (1025, 2 * 1025 + 2)):
        p = lib.plan(n, hint=1 << 20, slots=s, host=1)
        chunk = min(n, n * 32768 // s + 1)
        assert p["chunk"] == chunk and p["slots"] == max(chunk, 2 * (chunk * s // n + 1) + 64), (n, s)
    assert lib.plan(1025, hint=1 << 20, slots=1025 << 31, host=1)["tooLarge"] == 1
    assert lib.plan(1025, hint=1 << 20, slots=6 * 1025, host=1)["tooLarge"] == 0
    assert lib.plan(65537, hint=4096, slots=65537 << 31, host=1)["tooLarge"] == 0          # (the slot hint is not read outside the mode)


def test_k0_and_the_lane_pass(lib):
    """K0 from k0Min frames a chunk on, not in the several-block mode, not where the dictionary has entropy tables -- there the lane pass runs in front of K1"""
    for d in (D_NONE, D_CONTENT):
        assert lib.plan(6143, dict=d)["pre"] == 0 and lib.plan(6143, dict=d)["first.gPre"] == 0 and lib.plan(6143, dict=d)["preBytes"] == 0
        p = lib.plan(6144, dict=d)
        assert p["pre"] == 1 and p["first.gPre"] == 6144 // 64 and p["preBytes"] > 0 and p["first.k1"] == K1_PLAIN and p["first.gLanes"] == 0
        assert lib.plan(1, dict=d, knobs=dict(k0Min=0))["pre"] == 1 and lib.plan(65536, dict=d, knobs=dict(k0Min=10 ** 9))["pre"] == 0
        assert lib.plan(65537, dict=d)["pre"] == 1          # (the chunk counts, not the tail)
    assert lib.plan(6144, hint=256 << 10)["pre"] == 0 and lib.plan(6144, hint=256 << 10, dict=D_ENTROPY)["first.k1"] == K1_MB
    p = lib.plan(6144, dict=D_ENTROPY)
    assert p["pre"] == 0 and p["k1Lanes"] == 1 and p["first.k1"] == K1_LANES and p["first.gLanes"] == 6144 // 64 and p["first.gPre"] == 0
    assert lib.plan(6144, dict=D_ENTROPY, knobs=dict(k0Min=0))["pre"] == 0
    assert lib.plan(65536, dev=DEV_SMALL)["first.gPre"] == 8 * 7 and lib.plan(65536, dict=D_ENTROPY, dev=DEV_SMALL)["first.gLanes"] == 8 * 8


def test_grids(lib):
    """the bin kernel: 2 waves below 4 096 items, 128 from there; K1 / K3 by their waves per CU, K2 / K1b by LDS (4 and 4 one-wave workgroups a CU), KX 8 waves a CU"""
    assert lib.plan(4095)["first.gBin"] == 2 and lib.plan(4096)["first.gBin"] == 128
    assert lib.plan(342, hint=256 << 10)["first.items"] == 4104 and lib.plan(342, hint=256 << 10)["first.gBin"] == 128 and lib.plan(341, hint=256 << 10)["first.gBin"] == 2
    p = lib.plan(65536)
    assert (p["first.g1"], p["first.g3"], p["first.g2"], p["first.gHuf"], p["first.gCheck"]) == (256 * 8, 256 * 16, 256 * 4, 256 * 4, 1024)
    assert lib.plan(65536, knobs=dict(k3PerCU=24))["first.g3"] == 256 * 24
    p = lib.plan(65)
    assert (p["first.g1"], p["first.g3"], p["first.g2"], p["first.gHuf"], p["first.gCheck"]) == (65, 65, 5, 6, 2)
    p = lib.plan(65537)
    assert (p["last.g1"], p["last.g3"], p["last.g2"], p["last.gHuf"], p["last.gCheck"], p["last.gBin"]) == (1, 1, 1, 1, 1, 2)
    p = lib.plan(1024, dev=DEV_SMALL)
    assert (p["first.g1"], p["first.g3"], p["first.g2"], p["first.gHuf"], p["first.gCheck"]) == (64, 128, 32, 32, 16)


def test_arena_room_per_frame(lib):
    """160 KiB a slot; frames the caller says are below one block 4 x the size + 1 KiB where that is less; never less than the worst case of up to 1 024 frames"""
    worst = ZP_SEQ_STRIDE + ZP_LIT_STRIDE
    for n, hint in itertools.product((1, 1023, 1024, 1025, 65536, 65537), (0, 1, 256, 4096, 16384, 16385, 131071, 131072)):
        p = lib.plan(n, hint=hint)
        small = 4 * hint + 1024 if 0 < hint < BLOCK else 0
        room = min(small, 160 << 10) if small else 160 << 10
        want = max(p["slots"] * (room // 16), min(p["slots"], 1024) * ((small or worst) // 16))
        assert p["slots"] == min(n, 65536) and p["arenaBudget16"] == want and p["arenaBytes"] == want * 16 + 512 and p["litBytes"] == p["nslot"] * p["arenaBytes"] + 256, (n, hint)
    assert lib.plan(65536, hint=4096)["arenaBudget16"] == 65536 * (17 << 10) // 16          # (4 KiB documents get 17 KiB each instead of 160)
    assert lib.plan(65536)["arenaBudget16"] == 65536 * (160 << 10) // 16
    p = lib.plan(262145, hint=1 << 20, slots=6 * 262145, host=1)
    assert p["arenaBudget16"] == min(p["slots"] * (160 << 10) // 16, 0xFFFFFFF0)


def test_generic_grid(lib):
    """the fallback list is usually empty: 1 024 waves at most -- unless the caller says its frames exceed a block outside the several-block mode: then the list is the batch"""
    assert lib.plan(1000)["genericGrid"] == 1000 and lib.plan(4096)["genericGrid"] == 1024 and lib.plan(4096)["scratchBytes"] == 2048 * ZP_LIT_STRIDE
    assert lib.plan(4096, hint=256 << 10)["genericGrid"] == 1024 and lib.plan(4096, hint=BLOCK)["genericGrid"] == 1024
    assert lib.plan(4096, hint=1 << 31)["genericGrid"] == 2048
    assert lib.plan(4096, dev=DEV_SMALL)["genericGrid"] == 64 and lib.plan(63, dev=DEV_SMALL)["genericGrid"] == 63


def test_each_of_the_five_k3_kernels(lib):
    for hint, d, prof, k3 in ((0, D_NONE, 0, K3_EXEC), (0, D_NONE, 1, K3_PROF), (0, D_CONTENT, 0, K3_DICT), (0, D_ENTROPY, 1, K3_DICT), (256 << 10, D_NONE, 1, K3_MB),
                              (256 << 10, D_NONE, 0, K3_MB), (256 << 10, D_CONTENT, 0, K3_MB_DICT), (256 << 10, D_ENTROPY, 1, K3_MB_DICT)):
        p = lib.plan(65537, hint=hint, dict=d, prof=prof)
        assert p["first.k3"] == p["last.k3"] == k3, (hint, d, prof)


def test_the_host_pipelines_hint(lib):
    """zd_host_hint: the largest content size; a slot per one-block frame, blocks + 1 where the block count is known, 2 per 128 KiB + 2 where it is not; and from one frame in
    sixteen of one block's size that the block splitter cut on, a size hint just above a block: the several-block mode"""
    assert lib.host_hint([1000, BLOCK, 5, 0], [1, 1, 0, 1]) == (BLOCK, 4, 1)
    assert lib.host_hint([1 << 20], [9]) == (1 << 20, 10, 1) and lib.host_hint([1 << 20], [0]) == (1 << 20, 2 * 8 + 2, 1)
    assert lib.host_hint([BLOCK + 1], [0]) == (BLOCK + 1, 2 * 2 + 2, 1)
    assert lib.host_hint([100000] * 16, [2] + [1] * 15) == (BLOCK + 1, 15 + 3, 1)
    assert lib.host_hint([100000] * 17, [2] + [1] * 16) == (100000, 16 + 3, 1)
    assert lib.host_hint([100000] * 15 + [1 << 20], [2] + [1] * 14 + [0]) == (1 << 20, 3 + 14 + 18, 1)          # (a larger frame already says so)


def _record():
    """writes the fixture from ZHIP_PLAN_SO: a library with the same entry that holds the PARENT commit's lines, never the plan's"""
    assert os.environ.get("ZHIP_PLAN_SO"), "the fixture is recorded from the parent commit's decisions: name that library in ZHIP_PLAN_SO"
    lib = PlanLib()
    rows = [lib.row(**c) for c in spelled_cases()]
    digests = {name: digest(lib, cases) for name, cases in product_slices()}
    with open(FIXTURE, "w") as f:
        f.write('{"fields": %s,\n "product_sha256": %s,\n "expected": [\n%s\n]}\n' % (json.dumps(ALL_FIELDS), json.dumps(digests, indent=1), ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows)))
    print("%d cases spelled out, %d slices, %d bytes" % (len(rows), len(digests), os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        _record()
