"""The launch plan of device compress (python-zstandard_amd/csrc/zhip_encode_plan.hpp) on the CPU: every decision zhip_compress_batch_device reads -- flags, strides,
chunk, grids, reservations, launch numbers, the match-stage kernel of a chunk -- at both sides of every switch point.

Two checks. (1) Equality with tests/golden/encode_plan.json, which was recorded from the decisions of the commit BEFORE the plan existed (that commit's lines of
zhip_compress_batch_device pasted verbatim into a function of the same inputs), not from the plan's code: a SHA-256 of the rows of the WHOLE cross product of the axes below
(62 208 cases, one digest per level row and dictionary -- the rows themselves would be 10 MB), and some 290 cases around each switch spelled out, which say WHAT differs where a
digest does. (2) The switch points the project documents (tests/test_gpu_launch_shapes.py's docstring, the knobs' comments) asserted directly, so that a fixture regenerated
from wrong code cannot hide them.

The device shape is an input: 256 CUs, and for the per-CU wave counts the fallbacks zhip_ctx_create uses when its occupancy query fails (4, 4, 4). No real occupancy is claimed.
ZHIP_PLAN_SO names another library with the same entry (how the fixture was recorded: python -m tests.test_emu_encode_plan --record)."""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

import pytest

from tests import emulib

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "encode_plan.json")

FIELDS = ["greedy", "anyDfast", "mbcWanted", "flatDict", "flatFast", "flat", "allDfast", "fastWide", "mbc",
          "tableStride", "arenaStride", "arenaLit", "slotSrcMax", "e1Lanes", "chunk", "g1", "g2", "gBig",
          "metaBytes", "arenaBytes", "tablesBytes", "workspaceBytes", "bigListBytes", "e1ListBytes", "flatTablesBytes", "bigWsBytes",
          "mbBlocksBytes", "mbCountBytes", "mbSeqsBytes", "mbMaxBlocks", "mbSeqCap", "mbLanes", "epochShift", "epochKeyLayout", "flatMaxOpen", "flatMaxNeed"]
CHUNK_FIELDS = ["kernel", "shape", "probes", "fastPairs", "grid", "mbProbes"]          # kernel: 0 none, 1 LDS, 2 LDS fast, 3 flat, 4 flat fast
ALL_FIELDS = FIELDS + ["first." + f for f in CHUNK_FIELDS] + ["last." + f for f in CHUNK_FIELDS]
ROW_FIELDS = ["flags"] + [f for f in ALL_FIELDS[9:] if f != "flatMaxNeed"]          # a fixture row: the nine flags as one number (greedy = bit 0), then the rest
# (flatMaxNeed is stated by a test below instead: the parent computed it only on a context's first question)
K_NONE, K_LDS, K_LDS_FAST, K_FLAT, K_FLAT_FAST = range(5)

ZE_MB_POS_BITS = 22
ZE_ARENA_LIT = 8 * (43704 + 8)          # 8 x (ZE_SEQ_CAP + 8), zhip_format.hpp
NUM_CU = 256
DEV = (NUM_CU, 4, 4, 4)
SWITCHES = (1, 1, 4)                    # ZHIP_FAST_WIDE, ZHIP_TABLE_EPOCHS, ZHIP_E1LDS_PER_CU as the product builds
KNOB_NAMES = ["echunk", "echunkMax", "mbcMin", "mbcLanes", "flat4Max", "flat3Max", "flat3", "fast2Max", "fastPairs", "e1LdsMax", "e1LdsRounds"]
KNOB_DEFAULT = dict(echunk=0, echunkMax=0, mbcMin=4096, mbcLanes=32, flat4Max=32768, flat3Max=65536, flat3=1, fast2Max=32768, fastPairs=0, e1LdsMax=-1, e1LdsRounds=2)

NS = [1, 1024, 1025, 16383, 16384, 32768, 32769, 65536, 65537, 131072, 262144, 262145]
# (level, the seven explicit fields): levels -5, 1, 2, 3, 4, 5, 7 (a row the match kernels decline), explicit strategy 1 and 2 with window_log 17
ROWS = [(-5, (0,) * 7), (1, (0,) * 7), (2, (0,) * 7), (3, (0,) * 7), (4, (0,) * 7), (5, (0,) * 7), (7, (0,) * 7), (3, (17, 0, 0, 0, 0, 0, 1)), (3, (17, 0, 0, 0, 0, 0, 2))]
MB_EDGE = (1 << ZE_MB_POS_BITS) - 8
HINTS = [0, 4096, 4097, 16384, 65536, 131072, 131073, 256 << 10, 512 << 10, 1 << 20, MB_EDGE - 1, MB_EDGE]
# present, hlog, clog, strat, attachMax, contentSize: none; a double-fast dictionary with content; a fast one; one without content
DICTS = [(0, 0, 0, 2, 16384, 0), (1, 17, 16, 2, 16384, 110000), (1, 14, 13, 1, 8192, 30000), (1, 17, 16, 2, 16384, 0)]
KNOB_VARIANTS = [dict(echunk=1000), dict(echunkMax=4096), dict(fastPairs=1), dict(fastPairs=2), dict(e1LdsMax=0)]
KNOBS = [{}] + KNOB_VARIANTS


def case(n, row, hint, d=DICTS[0], flatMax=65536, knobs=None, host=1):
    return dict(n=n, level=row[0], ov=row[1], hint=hint, host=host, dict=d, flatMax=flatMax, knobs=knobs or {})


def product_slices():
    """the whole cross product, a slice per (level row, dictionary); the size hint is the batch's largest source, as from the host-buffer API"""
    for ri, row in enumerate(ROWS):
        for di, d in enumerate(DICTS):
            yield "rows%d.dict%d" % (ri, di), (case(n, row, hint, d, fm, kv) for n, hint, fm, kv in itertools.product(NS, HINTS, (65536, 131072), KNOBS))


def spelled_cases():
    """the cases whose rows the fixture spells out: each axis swept around the points where the others' switches lie"""
    L1, L3, L4, S2 = ROWS[1], ROWS[3], ROWS[4], ROWS[8]
    out = [case(n, row, 0) for n in NS for row in ROWS]                                                         # sources x levels, no hint
    out += [case(16384, row, hint) for hint in HINTS for row in (L1, L3, L4)] + [case(n, L3, hint) for hint in HINTS for n in (1024, 65537)]      # the size hint
    out += [case(n, row, 0, flatMax=131072) for n in NS[8:] for row in (L1, L3, S2)] + [case(65537, L3, hint, flatMax=131072) for hint in (131072, 256 << 10)]
    out += [case(16384, row, hint, host=0) for row in (L1, L3) for hint in (4096, 4097, 65536, 131073, 512 << 10)]                             # the caller's word alone: no LDS shape from it
    out += [case(n, L3, hint, d) for d in DICTS[1:] for n in (1, 1025, 65537, 262144, 262145) for hint in (0, 4096, 4097, 16384)]             # dictionaries
    out += [case(n, row, 0, knobs=kv) for kv in KNOB_VARIANTS for n in (1024, 32769, 65537) for row in (L1, L3)] + [case(16384, L3, 256 << 10, knobs=kv) for kv in KNOB_VARIANTS]
    return out


def fixture_row(p):
    return [sum(p[f] << i for i, f in enumerate(FIELDS[:9]))] + [p[f] for f in ROW_FIELDS[1:]]


def digest(lib, cases):
    h = hashlib.sha256()
    for c in cases:
        h.update((",".join(map(str, fixture_row(lib.plan(**c)))) + "\n").encode())
    return h.hexdigest()


class PlanLib:
    def __init__(self, path=None):
        path = path or os.environ.get("ZHIP_PLAN_SO") or emulib.EMU_SO
        if not os.path.exists(path):
            emulib.build()
        self.lib = C.CDLL(path)
        self.lib.emu_encode_plan.restype = C.c_int

    def plan(self, n, level=3, ov=(0,) * 7, hint=0, host=1, dict=DICTS[0], flatMax=65536, knobs=None, dev=DEV, switches=SWITCHES, **_):
        kn = KNOB_DEFAULT.copy(); kn.update(knobs or {})
        out = (C.c_uint64 * 64)()
        cnt = self.lib.emu_encode_plan(C.c_int(level), (C.c_int32 * 7)(*ov), C.c_uint64(n), C.c_uint64(hint), C.c_uint64(hint if host else 0), (C.c_int64 * 6)(*dict),
                                       (C.c_int64 * 4)(*dev), (C.c_int64 * 11)(*[kn[k] for k in KNOB_NAMES]), (C.c_int64 * 3)(*switches), C.c_uint64(flatMax), out)
        assert cnt == len(ALL_FIELDS), cnt
        return {f: int(out[i]) for i, f in enumerate(ALL_FIELDS)}


@pytest.fixture(scope="module")
def lib():
    return PlanLib()


def test_plan_is_the_parent_commits_decisions(lib):
    fx = json.load(open(FIXTURE))
    assert fx["fields"] == ROW_FIELDS
    spelled = spelled_cases()
    assert len(spelled) == len(fx["expected"]) and len(spelled) > 250
    bad = []
    for c, want in zip(spelled, fx["expected"]):
        got = fixture_row(lib.plan(**c))
        if got != want:
            bad.append((c, {f: (w, g) for f, w, g in zip(ROW_FIELDS, want, got) if w != g}))
    assert not bad, "%d of %d cases differ from the recorded decisions (field: (recorded, plan)); the first: %r" % (len(bad), len(spelled), bad[:3])
    got = {name: digest(lib, cases) for name, cases in product_slices()}
    assert len(got) == 36 and got == fx["product_sha256"], "slices of the whole cross product that differ from the recorded decisions: %r" % sorted(k for k in got if got[k] != fx["product_sha256"].get(k))


# ---- the documented switch points, stated directly
def test_lds_kernel_up_to_four_sources_per_cu(lib):
    """no size hint: the LDS-source kernel up to numCU x ZHIP_E1LDS_PER_CU sources, the flat kernel from one more"""
    for level, lds, flat in ((3, K_LDS, K_FLAT), (1, K_LDS_FAST, K_FLAT_FAST)):
        assert lib.plan(NUM_CU * 4, level=level)["first.kernel"] == lds
        assert lib.plan(NUM_CU * 4, level=level)["first.grid"] == NUM_CU * 4
        assert lib.plan(NUM_CU * 4 + 1, level=level)["first.kernel"] == flat
        assert lib.plan(NUM_CU * 4 + 1, level=level)["first.grid"] == (NUM_CU * 4 + 1 + 63) // 64
        assert lib.plan(NUM_CU * 4, level=level, knobs=dict(e1LdsMax=0))["first.kernel"] == flat


def test_probes_per_trip_by_launch_size(lib):
    """four probes up to 32 768 sources, three up to 65 536, two above"""
    for n, probes in ((1025, 4), (32768, 4), (32769, 3), (65536, 3)):
        p = lib.plan(n, level=3)
        assert (p["first.kernel"], p["first.probes"]) == (K_FLAT, probes), n
    p = lib.plan(131072, level=3, flatMax=131072)
    assert (p["chunk"], p["first.kernel"], p["first.probes"]) == (131072, K_FLAT, 2)
    # the fast form: two pairs up to fast2Max, one above, unless ZHIP_FAST_PAIRS forces either
    assert lib.plan(32768, level=1)["first.fastPairs"] == 2 and lib.plan(32769, level=1)["first.fastPairs"] == 1
    assert lib.plan(32768, level=1, knobs=dict(fastPairs=1))["first.fastPairs"] == 1 and lib.plan(32769, level=1, knobs=dict(fastPairs=2))["first.fastPairs"] == 2


def test_launches_for_65537_sources(lib):
    """one launch for 65 537 when flatMax is 131 072, two when it is 65 536; the question is open only above 65 536 sources and without ZHIP_ECHUNK_MAX"""
    for level in (1, 3):
        one, two = lib.plan(65537, level=level, flatMax=131072), lib.plan(65537, level=level, flatMax=65536)
        assert one["chunk"] == 65537 and two["chunk"] == 65536 and one["flatMaxOpen"] == two["flatMaxOpen"] == 1
        assert (two["first.grid"], two["last.grid"]) == (1024, 1)
        assert one["flatMaxNeed"] == two["flatMaxNeed"] == 131072 * (one["tableStride"] + one["arenaStride"]) // 8 * 9 + (4 << 30)
        assert lib.plan(65536, level=level, flatMax=131072)["flatMaxOpen"] == 0
        assert lib.plan(65537, level=level, flatMax=131072, knobs=dict(echunkMax=4096))["flatMaxOpen"] == 0
        assert lib.plan(65537, level=level, flatMax=131072, knobs=dict(echunkMax=4096))["chunk"] == 4096
    assert lib.plan(65537, level=5, flatMax=131072)["flatMaxOpen"] == 0          # (no flat search at level 5)


def test_dictionary_chunks(lib):
    """dictionary batches: chunks of 262 144 where the caller says its documents are small (4 KiB documents: 48 KiB of tables) -- one launch for 262 144 of them; at the
    attach cutoff's 192 KiB of tables a double-fast dictionary's 262 144 are two launches (32 GiB of tables at most), a fast dictionary's 64 KiB still one. Whatever flatMax."""
    for d in DICTS[1:]:
        for fm in (65536, 131072):
            p = lib.plan(262144, dict=d, flatMax=fm, hint=4096)
            assert p["chunk"] == 262144 and p["slotSrcMax"] == 4096 and p["flatMaxOpen"] == 0 and p["tableStride"] == ((48 << 10) if d[3] == 2 else (32 << 10))
            assert lib.plan(262145, dict=d, flatMax=fm, hint=4096)["chunk"] == 262144
            q = lib.plan(262144, dict=d, flatMax=fm)
            assert q["slotSrcMax"] == 0 and q["flatMaxOpen"] == 0
            if d[3] == 2:
                assert q["tableStride"] == 192 << 10 and q["chunk"] == (32 << 30) // (192 << 10) and 131072 <= q["chunk"] < 262144
            else:
                assert q["tableStride"] == 64 << 10 and q["chunk"] == 262144          # (hashLog 14 under the 8 KiB cutoff: 4 << 14)


def test_arena_stride_rule_and_table_stride_bounds(lib):
    """arenaStride == ZE_ARENA_LIT + 512 exactly when every row is fast or double-fast, there is no dictionary, and a flat form runs; tableStride within 4 KiB ... 12 << 17"""
    strat = {-5: (1, 1, 1, 1), 1: (1, 1, 1, 1), 2: (1, 2, 1, 1), 3: (2, 2, 2, 2), 4: (2, 3, 2, 3), 5: (3, 3, 3, 4), 7: (4, 4, 5, 5)}      # zh_levelTable's strategy column per size class
    seen = set()
    for case in itertools.chain(spelled_cases(), *(cases for _, cases in product_slices())):
        p = lib.plan(**case)
        assert (4 << 10) <= p["tableStride"] <= (12 << 17), case
        rows = (case["ov"][6],) * 4 if case["ov"][6] else strat[case["level"]]
        small = all(s in (1, 2) for s in rows) and not case["dict"][0] and p["flat"] == 1
        assert (p["arenaStride"] == ZE_ARENA_LIT + 512) == small, case
        if not case["dict"][0]:
            assert p["arenaLit"] == ZE_ARENA_LIT
        seen.add(small)
    assert seen == {True, False}


def _record():
    """writes the fixture from ZHIP_PLAN_SO: a library with the same entry that holds the PARENT commit's lines, never the plan's"""
    assert os.environ.get("ZHIP_PLAN_SO"), "the fixture is recorded from the parent commit's decisions: name that library in ZHIP_PLAN_SO"
    lib = PlanLib()
    rows = [fixture_row(lib.plan(**c)) for c in spelled_cases()]
    digests = {name: digest(lib, cases) for name, cases in product_slices()}
    with open(FIXTURE, "w") as f:
        f.write('{"fields": %s,\n "product_sha256": %s,\n "expected": [\n%s\n]}\n' % (json.dumps(ROW_FIELDS), json.dumps(digests, indent=1), ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows)))
    print("%d cases spelled out, %d slices, %d bytes" % (len(rows), len(digests), os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        _record()
