"""The entropy kernel on the MI355X, driven by explicit sequences: tests/test_emu_entropy_sequences.py's families through zhip_compress_sequences_device.

Every list is described in tests/entropy_families.py; the expected frame is libzstd 1.5.7's ZSTD_compressSequences on the same list (reflib.checker()),
computed -- and held against libzstd's own decoder -- before the call, and every frame of every batch is compared with it byte for byte, none sampled. Both
offset forms (canonical repeat codes / plain offsets) and both loader routes (the entropy kernel gathers the literals / the loader copies them) run.

  1. each family as its own small batches, one context per configuration;
  2. every default-configuration case, shuffled and replicated to more frames than the entropy kernel's resident grid (the library's own occupancy figure,
     DeviceBatchContext.entropy_grid), 4 096 at least, in ONE call: the work-stealing loop takes several frames per wave, sizes from 8 bytes to a full block
     follow each other in one wave, refused lists sit among the good ones; every fifth frame of the draw goes through a second, checksumming context (the
     trailer kernel);
  3. the dictionary families on dictionary contexts;
  4. compress and compress_sequences alternately on one context, both against libzstd: the shared setup serves either call after the other.

Layout and checks are test_gpu_launch_shapes.py's: sources and slots at odd offsets with gaps, slots of exactly zhip_compress_bound, canaries around every
slot, status -1 and a size sentinel before the call, so a frame no kernel answered fails."""
import collections
import time

import numpy as np
import pytest

from tests import entropy_families as E
from tests.test_emu_entropy_sequences import FORMS, ROOT, reference_frames
from tests.test_gpu_launch_shapes import CANARY, _bound, _dev, _odd_layout, _outside_slots_untouched, _segs, _t, zstd  # noqa: F401  (zstd: the module fixture)

pytestmark = pytest.mark.gpu

SIZE_SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def ref():
    from tests import reflib
    return reflib.checker()


@pytest.fixture(scope="module")
def dicts():
    return E.load_dicts(ROOT)


@pytest.fixture(scope="module")
def plain_cases(ref, dicts):
    return reference_frames(ref, E.plain_families(), dicts)


@pytest.fixture(scope="module")
def dict_cases(ref, dicts):
    return reference_frames(ref, E.dictionary_families(dicts), dicts)


def _ctx(cfg, dicts):
    from zstandard_amd.device import DeviceBatchContext
    d, raw = (dicts[cfg.dict_name][0], dicts[cfg.dict_name][3]) if cfg.dict_name else (None, False)
    return DeviceBatchContext(dict_data=d, dict_type=1 if raw else 0, level=cfg.level, write_checksum=cfg.checksum, write_content_size=cfg.content_size,
                              format=1 if cfg.magicless else 0, **cfg.params)


def _call(ctx, items, route, rng):
    """items = [(source, packed list)] through compress_sequences in the odd layout; returns (status, sizes, destination arena, slot offsets, slot capacities, ms)"""
    import torch
    n = len(items)
    uniq, index = {}, []
    for s, _ in items: index.append(uniq.setdefault(s, len(uniq)))
    srcs = list(uniq)
    slens = np.array([len(s) for s in srcs], dtype=np.int64)
    soffs, sarena = _odd_layout(rng, slens, rng.permutation(len(srcs)))
    src_np = np.full(sarena, 0x3C, dtype=np.uint8)
    for s, o in zip(srcs, soffs):
        src_np[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    index = np.array(index)
    caps = np.array([_bound(len(s)) for s, _ in items], dtype=np.int64)
    doffs, darena = _odd_layout(rng, caps, rng.permutation(n))
    # the lists in shuffled order too, with a gap of unrelated words between them
    order = rng.permutation(n)
    qoffs, pos, parts = np.zeros(n, dtype=np.int64), 0, []
    for i in order:
        gap = int(rng.integers(0, 4)); parts.append(np.full(gap, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)); pos += gap
        qoffs[i] = pos; parts.append(items[i][1]); pos += len(items[i][1])
    seqs = np.concatenate(parts + [np.zeros(1, dtype=np.uint64)]).view(np.int64)
    dev = _dev()
    dst = torch.full((darena,), CANARY, dtype=torch.uint8, device=dev)
    out_sizes = torch.full((n,), SIZE_SENTINEL, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    args = (_t(src_np), _segs(soffs[index], slens[index]), _t(seqs), _segs(qoffs, [len(q) for _, q in items]), dst, _segs(doffs, caps), out_sizes, status)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.compress_sequences(*args, copy_literals=bool(route))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return status.cpu().numpy(), out_sizes.cpu().numpy(), dst.cpu().numpy(), doffs, caps, ms, args


def _check(label, cases_forms, st, sz, got, doffs, caps):
    """cases_forms = [(case, form)]: every good frame is libzstd's, every refused list has its status and size 0, nothing outside the slots changed"""
    bad = []
    for i, (c, form) in enumerate(cases_forms):
        if c.refused is not None:
            if st[i] != c.refused or sz[i] != 0: bad.append((i, c.family, c.name, "not refused as it must be", int(st[i]), int(sz[i])))
        elif st[i] != 0: bad.append((i, c.family, c.name, form, "status", int(st[i])))
        elif got[doffs[i]: doffs[i] + sz[i]].tobytes() != c.want[form]: bad.append((i, c.family, c.name, form, "differs from libzstd's frame", int(sz[i]), len(c.want[form])))
    assert not bad, (label, len(bad), bad[:8])
    for i, (c, _) in enumerate(cases_forms):
        if c.refused is not None:
            assert (got[doffs[i]: doffs[i] + caps[i]] == CANARY).all(), (label, "a refused list's slot was written", c.name)
    ok, where = _outside_slots_untouched(got, doffs, caps)
    assert ok, (label, "bytes outside the slots changed at", where)


def _run_groups(label, cases, dicts, seed):
    groups = collections.OrderedDict()
    for c in cases: groups.setdefault(c.cfg.key(), []).append(c)
    rng = np.random.default_rng(seed)
    compared = 0
    for cs in groups.values():
        ctx = _ctx(cs[0].cfg, dicts)
        try:
            for form in FORMS:
                for route in (0, 1):
                    st, sz, got, doffs, caps, _, _ = _call(ctx, [(c.source, c.packed(form)) for c in cs], route, rng)
                    _check("%s, %r, %s, route %d" % (label, cs[0].cfg, form, route), [(c, form) for c in cs], st, sz, got, doffs, caps)
                    compared += len(cs)
        finally:
            ctx.close()
    return compared


@pytest.mark.parametrize("family", list(E.PLAIN))
def test_family_against_libzstd(zstd, plain_cases, dicts, family):
    cases = [c for c in plain_cases if c.family == family]
    if family == "refused lists": cases = cases + [c for c in plain_cases if c.family == "sequence counts"][:12]
    assert _run_groups(family, cases, dicts, 11) == 4 * len(cases)


def _big_draw(pool, grid, rng):
    """(main, fifth): every case of `pool` in both forms once, then small ones over and over and a large one now and then, shuffled; four of every five places
    form `main` -- cut at more frames than the resident grid, 4 096 at least --, the fifth places go to the checksumming context"""
    n_main = max(4096, grid + 1024)
    small = [c for c in pool if len(c.source) <= 20000]
    large = [c for c in pool if len(c.source) > 20000]
    draw = [(c, f) for c in pool for f in FORMS]
    while len(draw) < n_main * 5 // 4:
        src = large if large and rng.random() < 0.01 else small
        draw.append((src[int(rng.integers(0, len(src)))], FORMS[int(rng.integers(0, 2))]))
    draw = [draw[i] for i in rng.permutation(len(draw))]
    return [cf for i, cf in enumerate(draw) if i % 5 != 4][:n_main], [cf for i, cf in enumerate(draw) if i % 5 == 4]


def test_more_frames_than_the_resident_grid_in_one_call(zstd, plain_cases, dicts, ref):
    import torch
    pool = [c for c in plain_cases if c.cfg.key() == E.DEFAULT.key()]
    rng = np.random.default_rng(5)
    ctx, ctx_ck = _ctx(E.DEFAULT, dicts), _ctx(E.DEFAULT.with_checksum(), dicts)
    try:
        grid = ctx.entropy_grid()
        assert grid >= 64
        main, fifth = _big_draw(pool, grid, rng)
        n_main = len(main)
        assert len(main) == n_main > grid and any(c.refused is not None for c, _ in main)
        sizes = [len(c.source) for c, _ in main if c.refused is None]
        assert min(sizes) <= 8 and max(sizes) >= 131000, "sizes from 8 bytes to a full block in the one call"
        # the checksummed frames' expected bytes: the same lists with the checksum flag, from libzstd, before the call
        ck_want = {}
        for c, f in fifth:
            if c.refused is None and (id(c), f) not in ck_want:
                ck_want[(id(c), f)] = ref.compress_sequences(c.source, c.seqs, c.tail, level=3, flags=E.DEFAULT.with_checksum().flags(), rep_search=f == "canonical")
        for route in (0, 1):
            st, sz, got, doffs, caps, ms, args = _call(ctx, [(c.source, c.packed(f)) for c, f in main], route, rng)
            _check("one call of %d frames on a grid of %d, route %d" % (n_main, grid, route), main, st, sz, got, doffs, caps)
            # context only, no assertion: the same sources through the searching call on the same context
            st2 = torch.full((n_main,), -1, dtype=torch.int32, device=_dev()); sz2 = torch.zeros(n_main, dtype=torch.int64, device=_dev())
            dst2 = torch.empty_like(args[4])
            torch.cuda.synchronize(); t0 = time.perf_counter()
            ctx.compress(args[0], args[1], dst2, args[5], sz2, st2)
            torch.cuda.synchronize()
            print("\n[entropy sequences] %d frames (%.1f MB of sources), entropy grid %d: compress_sequences route %d %.1f ms; compress over the same sources %.1f ms"
                  % (n_main, sum(len(c.source) for c, _ in main) / 1e6, grid, route, ms, (time.perf_counter() - t0) * 1e3))
            st, sz, got, doffs, caps, _, _ = _call(ctx_ck, [(c.source, c.packed(f)) for c, f in fifth], route, rng)

            class _W:                      # the checksummed expectation in _check's shape
                def __init__(self, c, f): self.family, self.name, self.refused, self.want = c.family, c.name, c.refused, {f: ck_want.get((id(c), f))}
            _check("every fifth frame, checksummed, route %d" % route, [(_W(c, f), f) for c, f in fifth], st, sz, got, doffs, caps)
    finally:
        ctx.close(); ctx_ck.close()


def test_dictionary_families_against_libzstd(zstd, dict_cases, dicts):
    assert _run_groups("dictionary", dict_cases, dicts, 13) == 4 * len(dict_cases)


def test_compress_and_compress_sequences_alternate_on_one_context(zstd, plain_cases, dicts, ref):
    """the two calls share their setup and the context's scratch: each must serve after the other, several times over, with libzstd's frames"""
    import torch
    from tests.corpus import Corpus
    corpus = Corpus()
    raws = [corpus.frame_bytes(i)[: 131072 >> (i % 4)] for i in range(12)] + [b"", b"abc", b"z" * 5000]
    want = [ref.compress(r, level=3) for r in raws]
    cases = [c for c in plain_cases if c.cfg.key() == E.DEFAULT.key() and c.family in ("sequence counts", "lengths", "refused lists")]
    rng = np.random.default_rng(17)
    ctx = _ctx(E.DEFAULT, dicts)
    try:
        for turn in range(3):
            lens = np.array([len(r) for r in raws], dtype=np.int64)
            soffs, sarena = _odd_layout(rng, lens, rng.permutation(len(raws)))
            src_np = np.full(sarena, 0x3C, dtype=np.uint8)
            for r, o in zip(raws, soffs): src_np[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
            caps = np.array([_bound(len(r)) for r in raws], dtype=np.int64)
            doffs, darena = _odd_layout(rng, caps, rng.permutation(len(raws)))
            dst = torch.full((darena,), CANARY, dtype=torch.uint8, device=_dev())
            sz = torch.full((len(raws),), SIZE_SENTINEL, dtype=torch.int64, device=_dev()); st = torch.full((len(raws),), -1, dtype=torch.int32, device=_dev())
            ctx.compress(_t(src_np), _segs(soffs, lens), dst, _segs(doffs, caps), sz, st)
            torch.cuda.synchronize()
            got, stn, szn = dst.cpu().numpy(), st.cpu().numpy(), sz.cpu().numpy()
            for i in range(len(raws)):
                assert stn[i] == 0 and got[doffs[i]: doffs[i] + szn[i]].tobytes() == want[i], ("compress, turn %d" % turn, i, int(stn[i]))
            ok, where = _outside_slots_untouched(got, doffs, caps)
            assert ok, ("compress, turn %d" % turn, where)
            form = FORMS[turn % 2]
            st, sz, got, doffs, caps, _, _ = _call(ctx, [(c.source, c.packed(form)) for c in cases], turn % 2, rng)
            _check("compress_sequences, turn %d" % turn, [(c, form) for c in cases], st, sz, got, doffs, caps)
    finally:
        ctx.close()
