"""The many-ranges read of a seekable stream (zhip_seekable_decompress_ranges_device) without a GPU: the library's plan (zsk_gather_plan) against a brute-force
model, and the plan plus the three gather kernels on the host wave emulator with the decoder replaced by a copy -- bytes, guards, segments, statuses, rejected
calls -- and the same run as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

import numpy as np
import pytest

from tests import seekable_cases as sc
from tests import seekable_range_cases as rc_


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return rc_.emu(tmp_path_factory.mktemp("emu_seekable_ranges"))


# ---------------------------------------------------------------------------------------------------- 1. the plan against a brute-force model
@pytest.mark.parametrize("limit", rc_.LIMITS)
def test_plan_matches_model(lib, limit):
    for c in rc_.cases(lib):
        rc, stats, segs, jobs, passes, frames_of = rc_.plan(lib, c.stream, c.ranges, c.capacity, limit)
        assert rc == 0, c.name
        items, in_place, scratch_bytes, n_jobs, n_passes = stats[:5]
        d, sizes = c.d_off, np.diff(c.d_off)
        touch, want_in_place = rc_.model(d, c.ranges)
        assert items == int((touch > 0).sum()), c.name
        assert in_place == int(want_in_place.sum()), c.name
        for (o, l, _), (f0, f1) in zip(c.ranges, frames_of):
            if l:
                assert d[f0] <= o < d[f0 + 1] and d[f1] < o + l <= d[f1 + 1], c.name
        # every touched frame with content is in exactly one segment, in place exactly where the model says; items count up with frames
        seen, next_item, scratch_sum = np.zeros(len(sizes), dtype=np.int64), 0, 0
        used = {}                                                           # pass -> scratch bytes handed out so far
        largest = {}
        for first, count, item, home, inpl, p in segs:
            assert item == next_item, c.name
            if not inpl:
                assert home == used.get(p, 0), "scratch slots ascend with frames, back to back (%s)" % c.name
            for f in range(first, first + count):
                if not sizes[f]:
                    continue
                assert touch[f] > 0 and bool(inpl) == bool(want_in_place[f]), (c.name, f)
                seen[f] += 1; next_item += 1
                if not inpl:
                    used[p] = used.get(p, 0) + int(sizes[f]); largest[p] = max(largest.get(p, 0), int(sizes[f]))
        assert next_item == items and (seen == (touch > 0)).all(), c.name
        assert [s[5] for s in segs] == sorted(s[5] for s in segs) and [s[0] for s in segs] == sorted(s[0] for s in segs), c.name
        assert n_passes == len(passes) and (n_passes == 0) == (items == 0)
        lim = limit or rc_.DEFAULT_LIMIT
        for p, (scratch, item0, item1, _) in enumerate(passes):
            assert scratch == used.get(p, 0) and scratch <= max(lim, largest.get(p, 0)), (c.name, p)
            assert item0 == (passes[p - 1][2] if p else 0) and item1 >= item0
            scratch_sum += scratch
        assert scratch_sum == scratch_bytes == int(sizes[(touch > 0) & ~want_in_place].sum()), c.name
        if limit == 0:
            assert n_passes <= 1
        for p, src, dst, n in jobs:
            assert n > 0 and src + n <= passes[p][0] and dst + n <= c.capacity, c.name
        assert [j[0] for j in jobs] == sorted(j[0] for j in jobs)
        # the plan replayed: decode pass by pass into d_dst and the scratch, then the pass's copies
        content = np.frombuffer(c.content, dtype=np.uint8) if c.total else np.zeros(0, dtype=np.uint8)
        out = np.full(c.capacity, rc_.GUARD_BYTE, dtype=np.uint8)
        written = np.zeros(c.capacity, dtype=bool)
        for p in range(n_passes):
            scratch = np.zeros(passes[p][0], dtype=np.uint8)
            for first, count, item, home, inpl, sp in segs:
                if sp != p:
                    continue
                a, b = int(d[first]), int(d[first + count])
                if inpl:
                    out[home:home + b - a] = content[a:b]; written[home:home + b - a] = True
                else:
                    scratch[home:home + b - a] = content[a:b]
            for jp, src, dst, n in jobs:
                if jp == p:
                    out[dst:dst + n] = scratch[src:src + n]; written[dst:dst + n] = True
        for o, l, at in c.ranges:
            assert out[at:at + l].tobytes() == c.content[o:o + l], c.name
        assert not written[rc_.untouched_mask(c.ranges, c.capacity)].any(), c.name


def test_plan_small_examples(lib):
    """the counts the issue names for the 6-frame stream: sharing, in place, copies"""
    total, fs = sc.RANGE_CASE
    rng = np.random.default_rng(1)
    content = sc.source(total)
    stream = rc_.stream_for(lib, [len(p) for p in sc.chunks(content, fs)], content, False, rng)

    def stats(ranges):
        placed, at = [], 0
        for o, l in ranges:
            placed.append((o, l, at)); at += l
        rc, st, _, _, _, _ = rc_.plan(lib, stream, placed, at, 0)
        assert rc == 0
        return dict(items=st[0], in_place=st[1], scratch=st[2], jobs=st[3], passes=st[4])

    assert stats([(0, 100), (100, 4096), (4196, 8000)])["items"] == 3
    s = stats([(3 * 4096 + 100 * k, 100) for k in range(31)] + [(3 * 4096, 100)])
    assert (s["items"], s["in_place"], s["jobs"], s["scratch"]) == (1, 0, 32, 4096)
    s = stats([(0, total), (0, total)])
    assert (s["items"], s["in_place"], s["jobs"], s["scratch"]) == (6, 0, 2, total), "consecutive scratch frames are one copy per range"
    s = stats([(0, total)])
    assert (s["items"], s["in_place"], s["jobs"], s["scratch"], s["passes"]) == (6, 6, 0, 0, 1)
    s = stats([(4095, 2)])
    assert (s["items"], s["in_place"], s["jobs"], s["scratch"]) == (2, 0, 1, 8192)
    s = stats(sc.ranges_of(total))
    assert s["items"] == 6 and s["in_place"] == 2, "frames 3 and 4: only the whole-content range touches them"
    assert stats([(0, 0), (total, 0)]) == dict(items=0, in_place=0, scratch=0, jobs=0, passes=0)


# ---------------------------------------------------------------------------------------------------- 2. the whole path under emulation
@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("limit", rc_.LIMITS)
def test_emulated_path(lib, limit, checksum):
    for c in rc_.cases(lib, checksum):
        rc, status, dst, stats, items = rc_.run(lib, c.stream, c.content, c.ranges, c.capacity, limit)
        assert rc == 0, c.name
        assert status == [0] * (2 + 2 * len(c.ranges)), c.name
        for o, l, at in c.ranges:
            assert dst[at:at + l].tobytes() == c.content[o:o + l], c.name
        assert (dst[rc_.untouched_mask(c.ranges, c.capacity)] == rc_.GUARD_BYTE).all(), "guard bytes between and around the destinations (%s)" % c.name
        touch, want_in_place = rc_.model(c.d_off, c.ranges)
        assert stats[0] == len(items) == int((touch > 0).sum()) and stats[1] == int(want_in_place.sum()), c.name
        # the decoder's segments: every touched frame once, inside d_dst or the pass's scratch, none overlapping another
        assert [i[0] for i in items] == [int(f) for f in np.nonzero(touch > 0)[0]], c.name
        lim = limit or rc_.DEFAULT_LIMIT
        for kind in (0, 1):
            for p in sorted(set(i[4] for i in items)) if kind else [None]:
                spans = sorted((i[2], i[2] + i[3]) for i in items if i[1] == kind and (p is None or i[4] == p))
                assert all(a1 >= b0 for (_, b0), (a1, _) in zip(spans, spans[1:])), c.name
                if spans and kind == 0:
                    assert spans[-1][1] <= c.capacity
                if spans and kind == 1:
                    assert spans[-1][1] <= max(lim, max(b - a for a, b in spans)), c.name
        for f, kind, _, _, _ in items:
            assert (kind == 0) == bool(want_in_place[f]), (c.name, f)


# ---------------------------------------------------------------------------------------------------- 3. status
def _six(lib, checksum):
    total, fs = sc.RANGE_CASE
    content = sc.source(total)
    rng = np.random.default_rng(3)
    return content, rc_.stream_for(lib, [len(p) for p in sc.chunks(content, fs)], content, checksum, rng), total


@pytest.mark.parametrize("limit", [0, 4096])
def test_status(lib, limit):
    content, stream, total = _six(lib, True)
    listed = [(0, 100), (5000, 10), (2 * 4096 - 5, 4096), (0, total), (3 * 4096, 4096), (4 * 4096 + 7, 0), (3 * 4096 + 1, 5), (4 * 4096, 4096 + 17)]
    ranges, cap = rc_.place_destinations(np.random.default_rng(11), listed)
    needs = lambda f: [bool(l) and o < (f + 1) * 4096 and o + l > f * 4096 for o, l, _ in ranges]

    def check(status, dst, frame, code):
        want, first = [], None
        for r, hit in enumerate(needs(frame)):
            want += [code, frame] if hit else [0, 0]
            if hit and first is None:
                first = r
        assert status[2:] == want
        assert status[:2] == [code, first]
        for (o, l, at), hit in zip(ranges, needs(frame)):
            if not hit:
                assert dst[at:at + l].tobytes() == content[o:o + l]
        assert (dst[rc_.untouched_mask(ranges, cap)] == rc_.GUARD_BYTE).all()

    rc, status, dst, _, _ = rc_.run(lib, stream, content, ranges, cap, limit, short_frame=3)
    assert rc == 0
    check(status, dst, 3, 20)
    rc, status, dst, _, _ = rc_.run(lib, stream, content, ranges, cap, limit, code_frame=2, code=64)
    assert rc == 0
    check(status, dst, 2, 64)
    # both: every range reports the lowest failing frame among ITS frames
    rc, status, dst, _, _ = rc_.run(lib, stream, content, ranges, cap, limit, short_frame=3, code_frame=2, code=64)
    assert rc == 0
    want = []
    for n2, n3 in zip(needs(2), needs(3)):
        want += [64, 2] if n2 else [20, 3] if n3 else [0, 0]
    assert status[2:] == want and status[:2] == [64, 2], "range 2 is the lowest that fails"
    # what the entries were made of differs from what frames 1 and 4 "decode" to: checksum_wrong, the lowest frame per range
    wrong = bytearray(content); wrong[4096 + 9] ^= 1; wrong[4 * 4096 + 1] ^= 0x80
    rc, status, dst, _, _ = rc_.run(lib, stream, bytes(wrong), ranges, cap, limit)
    assert rc == 0
    want = []
    for n1, n4 in zip(needs(1), needs(4)):
        want += [22, 1] if n1 else [22, 4] if n4 else [0, 0]
    assert status[2:] == want and status[:2] == [22, 1]
    # a clean run of the same list
    rc, status, dst, _, _ = rc_.run(lib, stream, content, ranges, cap, limit)
    assert rc == 0 and status == [0] * (2 + 2 * len(ranges))


# ---------------------------------------------------------------------------------------------------- 4. rejected calls
def test_rejected_calls(lib):
    content, stream, total = _six(lib, False)
    good = [(0, 100, 0), (4000, 200, 100), (total - 1, 1, 300)]
    cap = 301
    rc, status, dst, _, _ = rc_.run(lib, stream, content, good, cap)
    assert rc == 0 and status == [0] * 8
    for bad, want, index in [
            (good + [(total, 1, 400)], sc.SIZE_MISMATCH, 3),                               # beyond the content
            (good + [(1 << 63, 1 << 63, 400)], sc.SIZE_MISMATCH, 3),                       # offset + length wraps
            ([(0, 0, 0), (0, total + 1, 0)], sc.SIZE_MISMATCH, 1),
            (good[:2] + [(total - 1, 2, 299)], sc.SIZE_MISMATCH, 2),
            ([(0, 100, 0), (0, 100, cap - 99)], sc.SIZE_MISMATCH, 1),                      # the destination ends beyond the capacity
            ([(0, 100, (1 << 64) - 50)], sc.SIZE_MISMATCH, 0),                             # dstOffset + length wraps
            ([(0, 100, 0), (200, 50, 150), (4000, 100, 99)], sc.UNSUPPORTED, 2),         # destinations overlap by one byte
            ([(0, 100, 20), (0, 100, 20)], sc.UNSUPPORTED, 1),
            ([(0, 100, 0), (0, 10, 50)], sc.UNSUPPORTED, 1)]:                            # one inside the other
        rc, status, dst, stats, _ = rc_.run(lib, stream, content, bad, cap)
        assert rc == want and stats[7] == index, bad
        assert (dst == rc_.GUARD_BYTE).all() and status == [-1] * (2 + 2 * len(bad)), "a rejected call writes nothing"
    # what is allowed: zero-length ranges anywhere (also at a taken destination and at the capacity), touching destinations, no ranges at all
    ok = [(0, 100, 0), (50, 100, 100), (total, 0, 50), (0, 0, cap), (7, 0, 0)]
    rc, status, dst, _, _ = rc_.run(lib, stream, content, ok, cap)
    assert rc == 0 and status == [0] * 12 and dst[:200].tobytes() == content[:100] + content[50:150]
    rc, status, dst, _, _ = rc_.run(lib, stream, content, [], cap)
    assert rc == 0 and status == [0, 0] and (dst == rc_.GUARD_BYTE).all()
    rc, status, dst, _, _ = rc_.run(lib, stream, content, [(5, 0, 3)], cap)
    assert rc == 0 and status == [0, 0, 0, 0] and (dst == rc_.GUARD_BYTE).all()


# ---------------------------------------------------------------------------------------------------- 5. the sanitizer run
def test_sanitizer_run(lib, tmp_path):
    """the plan and the emulated kernels over the seeds of test 1, as a stand-alone program built with -fsanitize=address,undefined, in a child process"""
    prog = rc_.sanitizer_program(tmp_path)
    path = os.path.join(str(tmp_path), "cases.bin")
    listed = rc_.cases(lib, True)
    # every seed at the default limit and at 20 000; the limits that make a pass of every frame or two where that stays a few hundred launches: each launch
    # under the sanitizer allocates the emulator's 64 lane stacks anew
    n = rc_.write_case_file(path, listed, (0, 20000)) + rc_.write_case_file(path, [c for c in listed if len(c.sizes) <= 65], (1, 4096), append=True)
    done = subprocess.run([prog, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode(errors="replace")[-4000:]
    assert done.stdout.decode().strip().endswith("%d cases" % n)
