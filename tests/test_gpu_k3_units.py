"""K3's long-item units and its global addressing on the MI355X: tests/k3units.py's cases through the device API, as tests/test_gpu_sequences.py runs
its families -- (a) frames of one block, (b) a raw block in front under the hint of 131 073 (the several-block mode), (c) the same without a hint (the
generic kernel, for comparison) --, the frames of several blocks under a hint of their own size, the raw-content dictionary cases for the dictionary
instantiations. libzstd 1.5.7 judges every frame first; the route is proved by DeviceBatchContext.decode_fallbacks; layout with gaps and canaries,
every frame answered (test_gpu_launch_shapes.py's _decode / _check_decode through test_gpu_sequences.py's _run).

Two layouts of their own: slots that start at every alignment 0 ... 15 (the flush stores whole 16-byte units from the slot's first byte on), and one
batch whose slots lie behind the 4 GiB mark of a destination buffer of a little over 4 GiB -- a 32-bit lane offset must count from the frame's slot,
never from the buffer. That buffer is torch.empty: only the slots are touched and compared. A few hundred frames in all, the largest of 1 MiB."""
import numpy as np
import pytest

from tests import k3units as U
from tests.seqmodel import K3
from tests.test_gpu_launch_shapes import CANARY, SIZE_SENTINEL, _context, _dev, _outside_slots_untouched, _segs, _t, zstd  # noqa: F401  (zstd: the module fixture)
from tests.test_gpu_sequences import HINT, ROUTES, _handed_on, _judged, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def unit_sets(ref, oracle):
    cases = U.one_block_cases(K3)
    return {"one_block": _judged(cases, ref, oracle), "led": _judged([c.with_lead() for c in cases], ref, oracle)}


@pytest.mark.parametrize("route", list(ROUTES))
def test_unit_cases_on_three_routes(zstd, unit_sets, route):
    """unit counts, item shapes, the record's fields, the history and the small slots with raw, Huffman-coded and RLE literals, one batch per route"""
    which, hint = ROUTES[route]
    cases = unit_sets[which]
    modes = {m for c in cases for m in U.block_modes(c)}
    assert modes >= {"raw", "huf1", "huf4", "rle"}
    ran = [b for c in cases if c.content is not None for b in U.all_batches(c)]
    assert {b["U"] for b in ran} >= {2, 63, 64, 65, 127, 128, 129, 239, 256}
    assert any(i["kind"] == "lit" and i["src"] > 65535 for b in ran for i in b["items"])
    assert {i["where"] for b in ran if b["after_slide"] for i in b["items"] if i["kind"] == "far"} >= {"inside", "one before", "straddles", "below"}
    if hint: assert sum(len(c.blocks) for c in cases) <= 6 * len(cases)
    _run("units, " + route, cases, hint, 1, seed=len(cases) + hint, fallbacks=_handed_on(route, len(cases)))


def test_sources_above_2_17_and_2_20_under_their_own_hint(zstd, ref, oracle):
    """far matches in units whose sources lie above 2^17 and 2^20 of the frame, in the several-block mode and in the generic kernel"""
    cases = _judged([U.in_mode(c, m) for c in U.distant_sources(K3) for m in U.MODES], ref, oracle)
    for c, lowest in zip(cases[::3], (1 << 17, 1 << 20)):
        assert sum(i["src"] >= lowest for b in U.all_batches(c) for i in b["items"] if i["kind"] == "far") >= 5, c.name
    for hint in (max(len(c.want) for c in cases), 0):
        _run("distant sources, hint %d" % hint, cases, hint, 1, seed=11, fallbacks=0 if hint else len(cases))


@pytest.mark.parametrize("route", list(ROUTES))
def test_long_items_from_a_dictionary(zstd, ref, oracle, route):
    """the dictionary instantiations: long far matches wholly inside a raw-content dictionary (a negative source through the hand-off), a straddler beside them"""
    which, hint = ROUTES[route]
    cases = [U.in_mode(c, m) for c in U.dictionary_cases(K3) for m in U.MODES]
    if which == "led": cases = [c.with_lead() for c in cases]
    cases = _judged(cases, ref, oracle)
    assert sum(i.get("where") == "dictionary" for c in cases for b in U.all_batches(c) for i in b["items"]) >= 12
    _run("units from a dictionary, " + route, cases, hint, 1, seed=hint + 13, fallbacks=_handed_on(route, len(cases)), dict_data=cases[0].dict_data, dict_type=1)


def _decode_at(ctx, cases, doffs, dst):
    """one decompress of `cases` into the slots at `doffs` of `dst`; returns (status, sizes)"""
    import torch
    n = len(cases)
    flens = np.fromiter((len(c.frame) for c in cases), dtype=np.int64, count=n)
    soffs = np.zeros(n, dtype=np.int64); soffs[1:] = np.cumsum(flens + 3)[:-1]
    src_np = np.full(int(soffs[-1] + flens[-1] + 8), 0x3C, dtype=np.uint8)
    for c, o in zip(cases, soffs): src_np[o:o + len(c.frame)] = np.frombuffer(c.frame, dtype=np.uint8)
    out_sizes = torch.full((n,), SIZE_SENTINEL, dtype=torch.int64, device=_dev())
    status = torch.full((n,), -1, dtype=torch.int32, device=_dev())
    ctx.decompress(_t(src_np), _segs(soffs, flens), dst, _segs(doffs, [c.cap for c in cases]), out_sizes, status)
    torch.cuda.synchronize()
    return status.cpu().numpy(), out_sizes.cpu().numpy()


def _aimed(ref, oracle, led):
    """a small set that reaches every kind of global address of the batch loop: units of both kinds, short items, pre-batch parts, the history and a
    slide, whole-wave near matches, big items, small slots"""
    from tests import seqfamilies as F
    base = U.item_shapes(K3) + U.history(K3) + U.unit_counts(K3)[3:5] + U.small_slots(K3)[::5] + F.near_matches(K3)[:3] + F.batch_shapes(K3)[:3] + F.slot_edges(K3)
    cases = [U.in_mode(c, U.MODES[i % 3]) for i, c in enumerate(base)]
    return _judged([c.with_lead() for c in cases] if led else cases, ref, oracle)


@pytest.mark.parametrize("route", ["a: one block", "b: several-block mode"])
def test_slots_at_every_alignment(zstd, ref, oracle, route):
    """every frame of the aimed set in sixteen slots, one at each alignment of the slot's first byte; canaries between the slots"""
    import torch
    which, hint = ROUTES[route]
    cases = [c for c in _aimed(ref, oracle, which == "led") for _ in range(16)]
    doffs, pos = np.zeros(len(cases), dtype=np.int64), 64
    for i, c in enumerate(cases):
        pos = (pos + 15) // 16 * 16 + 16 + i % 16                      # (16 bytes of canary at least in front of every slot)
        doffs[i] = pos; pos += c.cap
    assert {int(o) % 16 for o in doffs[:16]} == set(range(16))
    dst = torch.full((pos + 64,), CANARY, dtype=torch.uint8, device=_dev())
    ctx = _context(hint=hint)
    try:
        st, sz = _decode_at(ctx, cases, doffs, dst)
        handed_on = ctx.decode_fallbacks()
    finally:
        ctx.close()
    got = dst.cpu().numpy()
    bad = [(c.name, int(o) % 16, int(s)) for c, o, s, z in zip(cases, doffs, st, sz)
           if (s != 0 or got[o:o + z].tobytes() != c.want) if c.want is not None] + [(c.name, "accepted") for c, s in zip(cases, st) if c.want is None and s == 0]
    assert not bad, (route, len(bad), bad[:6])
    ok, where = _outside_slots_untouched(got, doffs, [c.cap for c in cases])
    assert ok, (route, "bytes outside the slots changed at", where)
    assert handed_on == 0


def test_slots_behind_the_4_gib_mark(zstd, ref, oracle):
    """the destination buffer is a little over 4 GiB and every slot lies behind its 4 GiB mark: an address formed from a 32-bit offset into the
    BUFFER wraps to its front, one formed from the frame's slot does not. Only the slots are initialised, read back and compared (routes a and b)."""
    import torch
    mark = 1 << 32
    dst = torch.empty(mark + (4 << 20), dtype=torch.uint8, device=_dev())
    for route in ("a: one block", "b: several-block mode"):
        which, hint = ROUTES[route]
        cases = _aimed(ref, oracle, which == "led")
        doffs, pos = np.zeros(len(cases), dtype=np.int64), mark + 1
        for i, c in enumerate(cases):
            doffs[i] = pos; pos += c.cap + 1 + i % 7
        assert pos < dst.numel() and int(doffs.min()) > mark
        dst[mark:pos + 16].fill_(CANARY)
        ctx = _context(hint=hint)
        try:
            st, sz = _decode_at(ctx, cases, doffs, dst)
            handed_on = ctx.decode_fallbacks()
        finally:
            ctx.close()
        got = dst[mark:pos + 16].cpu().numpy()
        rel = doffs - mark
        bad = [(c.name, int(s)) for c, o, s, z in zip(cases, rel, st, sz) if c.want is not None and (s != 0 or got[o:o + z].tobytes() != c.want)]
        assert not bad, (route, len(bad), bad[:6])
        ok, where = _outside_slots_untouched(got, rel, [c.cap for c in cases])
        assert ok, (route, "bytes between the slots changed at", where)
        assert handed_on == 0
