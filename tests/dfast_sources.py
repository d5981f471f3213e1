"""Sources aimed at the decision points of the double-fast search (ZSTD_compressBlock_doubleFast_noDict_generic; here ze_dfast / ze_dfast_g, ze_dfast_flat_np with two, three
and four probes a trip, its block form, and the dictionary forms), shared by the host test of the searches (test_emu_dfast.py), the mutants test (test_emu_dfast_mutants.py),
the stand-alone sanitizer program (emu/emu_dfast.cpp with -DEMU_DFAST_MAIN, through golden/dfast_sources.bin) and the GPU test of level 3 (test_gpu_dfast.py).

Every generator is seeded and returns `Case`s: the source, and what libzstd 1.5.7's parse (ZSTD_generateSequences) must show for it -- `expect`, a list of
(position, matchLength, offset) sequences that must be in libzstd's list, `absent`, positions at which no sequence may start, `last`, the literals behind the last sequence.
A source whose property libzstd does not show is a mistake of the SOURCE, and the tests say so before any search of the project's is looked at.

How the sources are built: `_B` writes literal runs of random bytes and copies at an offset, and keeps a copy from growing at either end (the literal behind it differs from
the byte that would extend it, the literal before it from the byte before its origin), so a copy is one match of exactly its length wherever libzstd finds it."""
import numpy as np

STRATEGY_DFAST = 2
# level 3's rows, level 4's where libzstd resolves it to double-fast (16 385 ... 131 072 bytes; below that its row is greedy and the set is passed over) and that row's fields
# given explicitly for the smaller sources; then explicit double-fast parameters laid over level 3
PARAM_SETS = [dict(level=3), dict(level=4), dict(strategy=STRATEGY_DFAST, hash_log=17, chain_log=17, min_match=4)] + [dict(strategy=STRATEGY_DFAST, min_match=m) for m in (4, 5, 6, 7)] + [
    dict(strategy=STRATEGY_DFAST, hash_log=h, chain_log=c, min_match=m) for h, c, m in ((12, 10, 4), (17, 16, 5), (10, 12, 6), (14, 14, 7))]
BLOCK = 131072


class Case:
    def __init__(self, name, raw, expect=(), absent=(), last=None, params=None, dict_data=None):
        self.name, self.raw, self.expect, self.absent, self.last, self.params = name, bytes(raw), list(expect), list(absent), last, params or PARAM_SETS
        self.dict_data = dict_data          # a raw-content dictionary: the case is for the table-copy mode's search (ze_dfast_ext) alone

    def __repr__(self):
        return "<%s: %d bytes>" % (self.name, len(self.raw))


class _Retry(Exception):
    pass


class _B:
    """a source under construction"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.buf = bytearray()
        self.cont = None          # the byte that would extend the copy just written
        self.tail_is_lit = False

    def __len__(self):
        return len(self.buf)

    def lit(self, n, avoid=None):
        """n random bytes; the first is neither the byte that would extend the copy before it nor `avoid`"""
        if n <= 0: return self
        b = bytearray(self.rng.bytes(n))
        while b[0] == self.cont or b[0] == avoid: b[0] = (b[0] + 1) & 255
        self.buf += b; self.cont = None; self.tail_is_lit = True
        return self

    def put(self, data):
        if len(data) and data[0] == self.cont: raise _Retry()
        self.buf += data; self.cont = None; self.tail_is_lit = False
        return self

    def copy(self, off, n, back=True):
        """n bytes from `off` back, one match of exactly n bytes: the literal before it is made to differ from the byte before the origin (back=False: left as it is)"""
        assert 0 < off <= len(self.buf)
        if back and len(self.buf) > off and self.buf[-1] == self.buf[-off - 1]:
            if not self.tail_is_lit: raise _Retry()
            self.buf[-1] = (self.buf[-1] + 1) & 255
        if self.cont is not None and self.buf[-off] == self.cont: raise _Retry()
        for _ in range(n): self.buf.append(self.buf[-off])
        self.cont = self.buf[-off]; self.tail_is_lit = False
        return self


# Seeds to pass over, by case name: the tables of a small source are small (hashLog <= 11 below 1 KiB), so now and then a cell a case depends on is taken by other bytes, under
# one parameter set or another, and libzstd's parse does not show the property. Such a draw is no use; the next seed is taken. choose_seeds() recomputes the table from libzstd.
SEED_SKIP = {'catch-up of 10': 1, 'end 24 rep -7': 1, 'end 24 rep -8': 1, 'end 24 rep -9': 3, 'end 25 match -9': 2, 'end 26 late -10': 1, 'end 29 chain -7': 1, 'end 30 chain -8': 1, 
             'end 30 chain -9': 1, 'end 33 late -9': 1, 'end 35 late -9': 1, 'end 37 rep -7': 1, 'end 41 late -9': 1, 'end 44 rep -7': 1, 'end 44 rep -8': 1, 'end 44 rep -9': 1, 
             'end 47 late -9': 1, 'end 54 late -9': 1, 'end 56 late -9': 1, 'end 58 late -9': 1, 'end 62 rep -8': 1, 'end 63 chain -7': 1, 'end 64 rep -7': 1, 'end 64 rep -8': 1, 
             'end 64 rep -9': 1, 'end 66 late -9': 2, 'end 70 late -9': 1, 'end 71 chain -8': 2, 'end 71 match -7': 1, 'end 72 chain -8': 1, 'end 73 late -9': 3, 'end 76 chain -7': 1, 
             'end 76 chain -8': 1, 'end 76 chain -9': 1, 'end 76 late -9': 1, 'end 78 late -9': 1, 'end 79 late -9': 3, 'end 79 rep -8': 1, 'end 80 chain -7': 1, 'end 80 rep -8': 1, 
             'short 10 then long 9 pad 1': 1, 'short 10 then long 9 pad 2': 1, 'step 4 lead 3 inner from pad + 0': 1, 'step 4 lead 3 inner from pad + 151': 1}


def _mk(name, fn, seed, *args, **extra):
    """the Case that fn(_B, *args) builds with the first usable seed of seed, seed + 1000, ...: one at which no copy runs into its neighbour, past SEED_SKIP[name] of them"""
    skip = SEED_SKIP.get(name, 0)
    for k in range(skip, skip + 50):
        try:
            b = _B(seed + 1000 * k)
            kw = fn(b, *args)
            kw.update(extra)
            return Case(name, b.buf, **kw)
        except _Retry:
            continue
    raise AssertionError("no seed builds %s%r" % (fn.__name__, args))


FAMILIES = ("step_sources", "end_sources", "candidate_sources", "lowest_index_sources", "equal_cell_sources", "catch_up_sources", "repeat_offset_sources", "insertion_sources", "block_sources", "ext_sources")


def choose_seeds():
    """prints SEED_SKIP: for every case the number of seeds to pass over until libzstd shows its property under all its parameter sets (python -m tests.dfast_sources)"""
    from tests.dfast_check import Lz, param_sets, property_failures
    lz = Lz()
    SEED_SKIP.clear()
    for fam in FAMILIES:
        for _ in range(40):
            bad = [c.name for c in globals()[fam]() if any(property_failures(c, lz(c.raw, **p)) for p, _ in param_sets(c, lz))]
            if not bad: break
            for name in bad: SEED_SKIP[name] = SEED_SKIP.get(name, 0) + 1
        else:
            print("# no seed found for", bad)
    print("SEED_SKIP = {%s}" % ", ".join("%r: %d" % kv for kv in sorted(SEED_SKIP.items())))


PAD = 3000


def _pad(b):
    """300 random bytes and their period up to 3 000: ONE match, a few hundred insertions -- but a source of 3 KiB and more, whose tables (sized by libzstd for the source: hashLog
    <= log2(size) + 1) then hold the construction behind it without a cell being taken twice. The search is fresh behind it, at step 1; the repeat offsets are 300 and 1."""
    b.lit(300); b.copy(300, PAD - 300)
    return len(b)


def visits(start, end):
    """[(position, step)] of the probes a stretch without a match makes from a fresh start at `start` (after a match, or 1 at the source's first byte) up to `end`: the step at a
    position is the one a match found THERE sees (ip1 = position + step), raised by one whenever ip1 reaches nextStep (`>=`), which starts 256 behind the fresh start"""
    ip, step, nxt = start, 1, start + 256
    out = []
    while ip < end:
        out.append((ip, step))
        ip1 = ip + step
        if ip1 >= nxt: step += 1; nxt += 256
        ip = ip1
    return out


# ------------------------------------------------------------------------------------------------------------ step growth
def _step_case(b, step, lead, first_of_step, fresh_at):
    """A = 64 random bytes right behind the pad (every position of the 256 behind a match is inserted); a stretch of random bytes; C = A[0:40] placed so that the first probe at or behind its start is `lead`
    bytes inside it and has `step`; then 8-byte copies of A[k:k + 8]. The match is found at v = start + lead with ip1 = v + step: the long cell of ip1 is written while step < 4,
    and then the copy of A[lead + step: +8] is found in C (offset to v + step); from step 4 on it is found in A. fresh_at > 0: a 40-byte match ends that far behind the pad first, so the stretch
    starts at another residue."""
    start = _pad(b)
    b.lit(8)
    a0 = len(b); b.lit(64)
    if fresh_at:
        b.lit(start + fresh_at - 40 - len(b)); b.copy(len(b) - a0 - 20, 40); start = len(b)        # (A[20:60], found by the long hash: all of A is inserted)
    vs = [(p, s) for p, s in visits(start, start + 256 * step + 64) if s == step and p > len(b) + 16]
    v = vs[0][0] if first_of_step else vs[7][0]
    pc = v - lead
    b.lit(pc - len(b))
    b.copy(pc - a0, 40)
    k = lead + step
    b.lit(11)
    q = len(b); b.copy(q - (a0 + k), 8)                                                   # the probe: A[k:k + 8]
    b.lit(13)
    q0 = len(b); b.copy(q0 - (a0 + lead + 12), 8)                                         # a control inside C that no rule inserts: always found in A
    b.lit(20)
    written = step < 4
    return dict(expect=[(pc, 40, pc - a0), (q, 8, q - (pc + k) if written else q - (a0 + k)), (q0, 8, q0 - (a0 + lead + 12))])


def step_sources():
    """The step grows by one per 256 bytes without a match, and a match found with step < 4 writes the long cell of ip + step (zstd's `if (step < 4)`), one found later does not:
    stretches that make the finding probe's step 1 ... 5, the probe landing on the copy's first byte and inside it, at the first position of a step (where ip1 landed on nextStep,
    `>=`) and further in; from the source's first byte and from the end of a match at another residue."""
    out = []
    for step in (1, 2, 3, 4, 5):
        for first in (True, False):
            if step == 1 and first: continue                                           # (the first probe of a stretch: nothing before it)
            for lead in sorted({0, step - 2 if first else step - 1}):                  # (the probe before the first of a step was one step shorter)
                for fresh_at in (0, 151):
                    out.append(_mk("step %d lead %d %s from pad + %d" % (step, lead, "first" if first else "inner", fresh_at), _step_case, 100 + step, step, lead, first, fresh_at))
    return out


# ------------------------------------------------------------------------------------------------------------ end of source
def _prefix(b, n, room):
    """fills up to n - room: short sources with random bytes, long ones with a period of 300 (one match up to there: the search is fresh and step 1 at its end). Returns the second
    repeat offset a match right behind it will see, and the position the cases copy from (inserted, and its bytes nowhere else in the tables)."""
    if n - room <= 40 + 300:
        b.lit(n - room)
        return 1, 2
    b.lit(300)
    b.copy(300, n - room - 300)
    return 300, 10


def _end_match(b, n, t):
    """a 12-byte match that ends t bytes before the end: ip + mLength = ilimit + 8 - t"""
    _, o = _prefix(b, n, 12 + 4 + t)
    b.lit(4)
    p = len(b); b.copy(p - o, 12)
    b.lit(t)
    assert len(b) == n
    return dict(expect=[(p, 12, p - o)], last=t)


def _end_rep(b, n, t, r):
    """... and right behind it r bytes at the second repeat offset, beginning at ilimit + 8 - t: taken while that is <= ilimit"""
    assert 4 <= r <= t
    off2, o = _prefix(b, n, 12 + 4 + t)
    b.lit(4)
    p = len(b); b.copy(p - o, 12)
    b.copy(off2, r)
    b.lit(t - r)
    assert len(b) == n
    if t >= 8: return dict(expect=[(p, 12, p - o), (p + 12, r, off2)], last=t - r)
    return dict(expect=[(p, 12, p - o)], absent=[p + 12], last=t)


def _end_chain(b, n, t):
    """a match, a repeat-offset match of 6 that ends t bytes before the end, and 5 bytes at the other repeat offset behind it: taken while n - t <= ilimit"""
    off2, o = _prefix(b, n, 12 + 4 + 6 + t)
    b.lit(4)
    p = len(b); b.copy(p - o, 12)
    b.copy(off2, 6)
    b.copy(p - o, 5)
    b.lit(t - 5)
    assert len(b) == n
    if t >= 8: return dict(expect=[(p, 12, p - o), (p + 12, 6, off2), (p + 18, 5, p - o)], last=t - 5)
    return dict(expect=[(p, 12, p - o), (p + 12, 6, off2)], absent=[p + 18], last=t)


def _end_late(b, n, t):
    """a copy that BEGINS t bytes before the end and runs into it: the last probe is the one with ip1 == ilimit, so one that begins at ilimit - 1 (t = 9) is found and one at ilimit (t = 8) is not"""
    _, o = _prefix(b, n, 4 + t)
    b.lit(4)
    p = len(b); b.copy(p - o, t)
    assert len(b) == n
    if t >= 9: return dict(expect=[(p, t, p - o)], last=0)
    return dict(absent=[p], last=None)


END_SIZES = tuple(range(8, 81)) + (4095, 4096, 4097, BLOCK - 1, BLOCK)
MIN_MATCH_4 = [dict(level=3), dict(strategy=STRATEGY_DFAST, min_match=4), dict(strategy=STRATEGY_DFAST, hash_log=12, chain_log=10, min_match=4)]      # (level 3's row has minMatch 4 up to 16 KiB)


def _end_small(b, n, t, kind, m):
    """the constructions above at their smallest: random bytes, then a copy of m bytes from position 1 (position 0 is never inserted), then what the kind wants, then the
    literals that make the size n. The repeat offsets behind the first match are its own and 1."""
    extra = {"match": 0, "rep": 0, "chain": 4}[kind]
    pre = n - m - extra - t
    assert pre >= m + 2                                            # a first byte, the origin, one byte between the origin and its copy
    b.lit(pre)
    p = len(b); d = p - 1; b.copy(d, m)
    if kind == "match":
        b.lit(t)
        return dict(expect=[(p, m, d)], last=t)
    if kind == "rep":
        r = 4 if t == 7 else 5
        b.copy(1, r); b.lit(t - r)
        if t >= 8: return dict(expect=[(p, m, d), (p + m, r, 1)], last=t - r)
        return dict(expect=[(p, m, d)], absent=[p + m], last=t)
    b.copy(1, 4); b.copy(d, 4); b.lit(t - 4)
    if t >= 8: return dict(expect=[(p, m, d), (p + m, 4, 1), (p + m + 4, 4, d)], last=t - 4)
    return dict(expect=[(p, m, d), (p + m, 4, 1)], absent=[p + m + 4], last=t)


def _end_late_small(b, n, t):
    b.lit(n - t)
    p = len(b); b.copy(p - 1, t)
    if t >= 9: return dict(expect=[(p, t, p - 1)], last=0)
    return dict(absent=[p], last=None)


def end_small_copy(n, t, kind):
    """the copy length the smallest construction uses at size n, or 0 where the size cannot hold the property: n = pre + m + extra + t with pre >= m + 2 (a first byte that is
    never inserted, the origin, a byte between), extra = 5 for the chain (the first repeat-offset match of 4, and a second byte between: with one, the third match's origin is
    the run the second one made), so n >= 2 m + 2 + extra + t. m = 8 is found through the long hash
    under every parameter set: n >= 25 + extra for t = 7. m = 4 is libzstd's smallest match and a short match under minMatch 4 only: n >= 17 + extra for t = 7, one more per
    t. Below 17 (18, 19 for t = 8, 9) no source has a match that ends there: two occurrences of four bytes, one byte before and one between, and t behind do not fit."""
    extra = 5 if kind == "chain" else 0
    for m in (8, 4):
        if n >= 2 * m + 2 + extra + t: return m
    return 0


def end_sources():
    """ilimit = n - 8. For every size 8 ... 80, around 4 096 and at 131 071 / 131 072: a match that ends at ilimit - 1, ilimit, ilimit + 1 (`if (ip <= ilimit)` in front of the
    insertions and the repeat-offset loop); a repeat-offset match that begins there (taken at <= ilimit only) and one chained behind another that ends there (`while (ip <= ilimit`);
    a match that begins at the last probe (ip1 == ilimit) and one position later (ip1 == ilimit + 1: the loop has ended) -- each kind at all three ends at every size that can
    hold it (end_small_copy gives the arithmetic: from 17 bytes on under minMatch 4, from 25 on under every parameter set; the late match from 18 / 20 / 22 on). Every size below
    25 also gets compressible bytes with no property but libzstd's parse -- below 16 bytes the lane-serial search only, 63 / 64 is where the product hands over to it."""
    out = []
    for n in END_SIZES:
        if n < 25:
            rng = np.random.default_rng(200 + n)
            out.append(Case("end %d period 3" % n, (rng.bytes(3) * n)[:n]))
            out.append(Case("end %d half" % n, (lambda h: (h + h + h)[:n])(rng.bytes(max(4, n // 2 - 1)))))
            out.append(Case("end %d two symbols" % n, bytes(rng.integers(0, 2, n, dtype=np.uint8))))
        big = n > 80
        for t in (7, 8, 9):
            for kind, fn, seed in (("match", _end_match, 300), ("rep", _end_rep, 400), ("chain", _end_chain, 500)):
                name = "end %d %s -%d" % (n, kind, t)
                if big:
                    out.append(_mk(name, fn, seed + n % 97, n, t, *((4 if t == 7 else 5,) if kind == "rep" else ())))
                    continue
                m = end_small_copy(n, t, kind)
                if m: out.append(_mk(name, _end_small, seed + n, n, t, kind, m, params=None if m == 8 else MIN_MATCH_4))
        for t in (8, 9, 10):
            if big: out.append(_mk("end %d late -%d" % (n, t), _end_late, 600 + n % 97, n, t))
            elif n >= 2 * t + 2: out.append(_mk("end %d late -%d" % (n, t), _end_late_small, 600 + n, n, t))
    return out


# ------------------------------------------------------------------------------------------------------------ which candidate wins
def _rep_beats_long(b):
    """at p a long match (12 bytes, L at 8) and at p + 1 four bytes at the first repeat offset: the repeat offset is examined first and wins"""
    _pad(b)
    b.lit(8)
    a = len(b); b.lit(12); L = bytes(b.buf[a:a + 12])
    b.lit(6)
    y = len(b) + 1; b.put(bytes([L[0] ^ 0x33]) + L[1:5] + bytes([L[5] ^ 0x44]))
    b.lit(9)
    m = len(b); p = m + 10 + 5; d = p + 1 - y
    b.copy(d, 10)                                               # the match that makes d the first repeat offset
    b.lit(5)
    assert len(b) == p
    b.copy(p - a, 12, back=False)
    b.lit(30)
    return dict(expect=[(m, 10, d), (p + 1, 4, d)], absent=[p])


def _long_beats_short(b):
    """at p the short cell points at a newer occurrence of the first 4 ... 7 bytes, the long cell at the older 12: the long match is taken"""
    _pad(b)
    b.lit(8)
    a = len(b); b.lit(12); L = bytes(b.buf[a:a + 12])
    b.lit(9)
    s = len(b); b.put(L[:7] + bytes([L[7] ^ 0x21]))
    b.lit(9)
    p = len(b); b.copy(p - a, 12)
    b.lit(30)
    return dict(expect=[(s, 7, s - a), (p, 12, p - a)])


def _short_then_long(b, ms, l1, pad=0, low_pad=None):
    """a short match of ms bytes at p and a long match of l1 bytes at p + 1: the long one is taken only if LONGER (l1 > ms). S = c0 + lam[0:ms - 1] where c0 is the last byte of a
    match -- a position that enters the short table only --, then lam[0:l1] further on (found as a match of ms - 1, its long cell written), then c0 + lam[0:l1] at p"""
    _pad(b)
    b.lit(8 + pad)
    x = len(b); b.lit(14)
    b.lit(7)
    b.copy(len(b) - x, 10)                                       # ends with c0
    s = len(b) - 1; c0 = b.buf[s]
    lam = bytearray(b.rng.bytes(max(l1, ms) + 1))
    while lam[0] == b.cont: lam[0] = (lam[0] + 1) & 255
    b.put(bytes(lam[:ms - 1]) + bytes([lam[ms - 1] ^ 0x5a]))
    b.lit(9, avoid=c0)
    if b.buf[-1] == c0: b.buf[-1] ^= 1
    l = len(b); b.put(bytes(lam[:l1]) + bytes([lam[l1] ^ 0x3c]))
    b.lit(9)
    if b.buf[-1] == b.buf[s - 1]: b.buf[-1] ^= 1
    p = len(b); b.put(bytes([c0]) + bytes(lam[:l1]) + bytes([lam[l1] ^ 0x77]))
    b.lit(30)
    if l1 > ms: return dict(expect=[(p + 1, l1, p + 1 - l)], absent=[p])
    return dict(expect=[(p, ms, p - s)], absent=[p + 1])


def candidate_sources():
    """The order of the candidates at one position: the first repeat offset at ip + 1, then the long match at ip, then the short one -- and behind a short match the long candidate
    of ip + 1, taken if longer (11 against 10), not if equal (10) or shorter by one (9)."""
    out = []
    out.append(_mk("repeat offset at ip + 1 beats long at ip", _rep_beats_long, 700))
    out.append(_mk("long beats short", _long_beats_short, 701))
    for l1 in (11, 10, 9):
        for pad in (0, 1, 2):
            out.append(_mk("short 10 then long %d pad %d" % (l1, pad), _short_then_long, 702 + l1, 10, l1, pad))
    return out


def _lowest_long(b, at_low, kind="ahead"):
    """a frame of 131 072 + 70 000 bytes under window_log 17: in the second block the lowest valid index is position 70 000. There lam (12 bytes) starts (at_low) or one byte
    later; in the second block S = c0 + lam[0:6] (7 bytes: a short match under every minMatch, no long one) and then c0 + lam at p: the long candidate of p + 1 is valid only ABOVE the lowest
    index (`idxl1 > LOW`), so at_low the short match of 7 at p is taken and otherwise the long one of 12 at p + 1"""
    low = 70000
    b.lit(300); b.copy(300, low - 10 - 300)
    b.lit(10 if at_low else 11)
    l = len(b); b.lit(12); lam = bytes(b.buf[l:l + 12])
    b.lit(5)
    b.copy(300, BLOCK + 20 - len(b))
    b.lit(9)
    if kind != "ahead":                                             # lam's first 8 bytes (the long candidate at ip) or 7 (the short one): valid AT the lowest index (`>=`)
        n = 8 if kind == "long" else 7                              # (8 and no more: nine would be a long match one step ahead too, caught up to the same sequence)
        if kind == "long": b.put(lam[:7] + bytes([lam[7] ^ 0x29])); b.lit(9)          # (a newer owner of the short cell: only the long candidate leads to lam itself)
        q = len(b); b.copy(q - l, n)
        b.lit(20)
        b.copy(300, BLOCK + low - len(b))
        return dict(expect=[(q, n, q - l)])
    c0 = lam[0] ^ 0x11
    if b.buf[-1] == b.buf[l - 1]: b.buf[-1] ^= 1
    s = len(b); b.put(bytes([c0]) + lam[:6] + bytes([lam[6] ^ 0x42]))
    b.lit(9)
    p = len(b); b.put(bytes([c0]) + lam + bytes([b.buf[l + 12] ^ 0x18]))
    b.lit(20)
    b.copy(300, BLOCK + low - len(b))
    assert len(b) == BLOCK + low and l == (low if at_low else low + 1)
    if at_low: return dict(expect=[(p, 7, p - s)], absent=[p + 1])
    return dict(expect=[(p + 1, 12, p + 1 - l)], absent=[p])


def lowest_index_sources():
    """`idxl1 > LOW` against `>=`: only a form whose lowest index is above 2 AND was inserted can tell them apart -- ze_dfast_g (the generic kernel's search of sources above one
    block) under a window shorter than the frame. In the one-block forms and the flat block form LOW is the frame's first byte, which no search ever inserts."""
    out = []
    par = [dict(strategy=STRATEGY_DFAST, window_log=17, hash_log=17, chain_log=16, min_match=m) for m in (4, 5, 7)]
    for at_low in (True, False):
        out.append(_mk("long candidate one step ahead %s the lowest index" % ("at" if at_low else "above"), _lowest_long, 720, at_low, params=par))
    for kind in ("long", "short"):
        out.append(_mk("%s candidate at the lowest index" % kind, _lowest_long, 721, True, kind, params=par))
    return out


# ------------------------------------------------------------------------------------------------------------ equal cells inside a trip
def equal_cell_sources():
    """Alphabets of 2 and 3 symbols and periods 1 ... 9: the probes of one trip share long and short cells all the time, so every read depends on the forwarding of the trip's
    earlier writes -- and the long candidate carried from the trip before (cellL0) on a write of that trip. No property but libzstd's parse."""
    out = []
    rng = np.random.default_rng(800)
    for syms in (2, 3):
        for n in (64, 200, 777, 3001):
            out.append(Case("alphabet of %d, %d" % (syms, n), bytes(rng.integers(0, syms, n, dtype=np.uint8))))
    for period in range(1, 10):
        unit = bytes(rng.integers(0, 3, period, dtype=np.uint8)) if period > 2 else bytes(rng.bytes(period))
        for n in (70, 1000):
            raw = bytearray((unit * (n // period + 1))[:n])
            out.append(Case("period %d, %d" % (period, n), raw))
            for k in range(n // 3, n, n // 3 + 1): raw[k] ^= 1                              # the period broken now and then: matches end, the search goes on inside the period
            out.append(Case("period %d broken, %d" % (period, n), raw))
    # a period of 2 ... 9 in a random stretch at a step above 1: the probes of one trip are `step` apart and land on equal bytes when the step divides the period
    for period in (2, 3, 4, 6, 8):
        b = _B(810 + period)
        b.lit(300 * (period % 4 + 1))
        unit = b.rng.bytes(period)
        b.put(unit * (40 // period + 3)); b.lit(300); b.put(unit * 6); b.lit(40)
        out.append(Case("period %d behind %d random bytes" % (period, 300 * (period % 4 + 1)), b.buf))
    return out


# ------------------------------------------------------------------------------------------------------------ catch-up backwards
def _catch_up(b, back, stop):
    """20 bytes Q; the copy of Q[0:20] is found at its byte `back` (the bytes before it were never inserted: a stretch at step `back + 1`) and caught up `back` bytes, until
    stop = "diff": the byte before differs; "anchor": a match ended there; "zero": the origin is the source's first byte"""
    if stop == "zero":
        q = 0; b.lit(20)
        b.lit(30)
        p = len(b); b.copy(p, 20, back=False)                       # position 0 is never inserted: found at p + 1 against 1, caught up to 0
        b.lit(20)
        return dict(expect=[(p, 20, p)])
    base = _pad(b)
    b.lit(8)
    q = len(b); b.lit(24)
    step = back + 1
    vs = [(p, s) for p, s in visits(base, base + 256 * step + 300) if s == step and p > len(b) + 40]
    v = vs[3][0]
    p = v - back
    if stop == "anchor":
        # Q's first byte is a position the stretch (step 3 by then) passes over, so its copy is found one byte in, at p + 1, right behind a match that ends at p: the byte
        # before Q is made the last byte of that match, so the bytes go on agreeing and only the anchor stops the catch-up
        del b.buf[base:]; b.lit(700)
        q = [p for p, s in visits(base, base + 700) if s == 3][5] - 1
        o1 = base + 10
        b.buf[q - 1] = b.buf[o1 + 11]
        b.lit(9)
        m = len(b); b.copy(m - o1, 12)
        p = len(b); b.copy(p - q, 20, back=False)
        b.lit(20)
        return dict(expect=[(m, 12, m - o1), (p, 20, p - q)])
    b.lit(p - len(b))
    b.copy(p - q, 20)
    b.lit(20)
    return dict(expect=[(p, 20, p - q)])


def catch_up_sources():
    """The catch-up backwards, 8 bytes a round in the flat form: a difference 1 ... 10 bytes back (7, 8, 9 around the round's width), the anchor, position 0 (and with it the
    byte-wise path for origins below 8)."""
    out = []
    for back in (1, 2, 3, 6, 7, 8, 9, 10):
        out.append(_mk("catch-up of %d" % back, _catch_up, 900 + back, back, "diff"))
    out.append(_mk("catch-up stopped by the anchor", _catch_up, 920, 0, "anchor"))
    out.append(_mk("catch-up to position 0", _catch_up, 921, 1, "zero"))
    # origins below 8: Q at 1 ... 7, found `back` bytes in
    for q in (1, 2, 5, 7):
        def low(b, q=q):
            b.lit(q); b.lit(20); b.lit(600)
            v = [p for p, s in visits(1, 900) if s == 3 and p > 400][2]
            p = v - 2
            del b.buf[p:]; b.tail_is_lit = True
            b.copy(p - q, 20); b.lit(20)
            return dict(expect=[(p, 20, p - q)])
        out.append(_mk("catch-up of 2 to origin %d" % q, low, 930 + q))
    return out


# ------------------------------------------------------------------------------------------------------------ repeat offsets
def _alternating(b, n_rounds):
    """records from two sources at two distances, each cut short by a literal: match, then right behind it the OTHER offset (the second repeat offset, swapped in), round after round"""
    _pad(b)
    b.lit(8)
    x = len(b); b.lit(40)
    y = len(b); b.lit(40)
    b.lit(5)
    p1 = len(b); b.copy(p1 - x, 10); d1 = p1 - x
    b.lit(3)
    p2 = len(b); b.copy(p2 - y - 3, 10); d2 = p2 - y - 3
    exp = [(p1, 10, d1), (p2, 10, d2)]
    for k in range(n_rounds):
        p = len(b); b.copy(d1 if k % 2 == 0 else d2, 5 + k % 3); exp.append((p, 5 + k % 3, d1 if k % 2 == 0 else d2))
    b.lit(20)
    return dict(expect=exp)


def _off2_zero(b):
    """the second repeat offset is 0 until the first match: four equal bytes right behind the first match are no repeat-offset match at offset 4 (libzstd's {1, 4} start, the 4 parked at entry) ..."""
    b.lit(4)
    b.put(bytes([b.buf[0] ^ 1, b.buf[1], b.buf[2], b.buf[3]]) + b.buf[1:4])        # bytes 5 ... 7 = bytes 1 ... 3: offset 4, three bytes and no more
    b.lit(20)
    x = 8; p = len(b); b.copy(p - x, 9)
    b.copy(1, 4)                                                    # ... but at offset 1, the first one moved down, they are
    b.lit(20)
    return dict(expect=[(p, 9, p - x), (p + 9, 4, 1)])


def repeat_offset_sources():
    """The repeat-offset loop behind a match (`while (off2 > 0 && ...)`, the two offsets swapped at every hit): both offsets alternating for 2 and 7 rounds -- and the state it
    starts from: libzstd's {1, 4} with the 4 parked, so that behind the first match the second offset is the old first one, 1, and not 4."""
    out = []
    for rounds in (2, 7):
        out.append(_mk("both offsets alternating, %d rounds" % rounds, _alternating, 1000 + rounds, rounds))
    out.append(_mk("second offset empty at the start", _off2_zero, 1010))
    return out


def _two_blocks(b, first, both):
    """The first block leaves no match ("none": 128 KiB of random bytes), one ("one": a period of 300) or two ("two": and a 12-byte match into its first bytes, at offset d) -- so it hands on the repeat
    offsets {1, 4} (the 4, larger than position 1, was parked at its entry and is restored at its end: `saved2`), {300, 1} or {d, 300}. The second block opens with 9 bytes at
    the first of them from its second byte on (the repeat-offset check at ip + 1) and, `both`, 6 bytes at the second right behind (the repeat-offset loop behind that match)."""
    if first == "none": b.lit(BLOCK); r0, r1 = 1, 4
    else:
        b.lit(300); b.copy(300, BLOCK - 300 - (20 if first == "one" else 70)); r0, r1 = 300, 1
        exp = [(300, len(b) - 300, 300)]
        if first == "two":
            b.lit(38); p = len(b); b.copy(p - 40, 12); exp.append((p, 12, p - 40)); r0, r1 = p - 40, 300
        b.lit(BLOCK - len(b))
    exp = [] if first == "none" else exp
    b.lit(1)
    p = len(b); b.copy(r0, 9, back=False); exp.append((p, 9, r0))
    if both: b.copy(r1, 6); exp.append((p + 9, 6, r1))
    b.lit(3000)
    return dict(expect=exp)


def block_sources():
    """Sources of two and three blocks for the block form (tables and repeat offsets carried, zstd.c:31091-31098 / :31252-31258). An incoming offset larger than the position
    is parked and restored: that can only happen in a frame's FIRST block (the 4 of the {1, 4} start), so what is checked is what the first block leaves after no, one and two
    matches (`saved1` / `saved2`) -- read back by the second block through its first two sequences, and compared as numbers by the test --, and matches across the block
    boundary into the first block's tables."""
    out = []
    for first in ("none", "one", "two"):
        for both in (False, True):
            if first == "none" and both: continue                  # ({1, 4}: nine equal bytes at offset 1 are at offset 4 too)
            out.append(_mk("first block with %s match, second opens with %s" % (first, "both offsets" if both else "the first offset"), _two_blocks, 1100, first, both))
    rng = np.random.default_rng(1150)
    unit = rng.bytes(5000)
    out.append(Case("three blocks, period 5000 with breaks", b"".join(unit[:4000 + 37 * k] + rng.bytes(50) for k in range(64))[:2 * BLOCK + 4321]))
    return out


# ------------------------------------------------------------------------------------------------------------ insertions behind a match
def _insertion(b, which):
    """a 30-byte match M found at p0 (curr = p0) that ends at e, then further on 8 bytes that only one of the insertions behind a match makes findable THERE: "curr+2 long" /
    "curr+2 short" (position p0 + 2, inside M), "end-2" (long, e - 2), "end-1" (short, e - 1), and the two inside the repeat-offset loop ("rep long", "rep short": the position
    the repeat-offset match began at). The same bytes are also at M's origin, further back: the offset tells which was found. The short ones share 7 bytes and differ in the eighth."""
    _pad(b)
    b.lit(8)
    a = len(b); b.lit(40)
    b.lit(20)
    p0 = len(b); b.copy(p0 - a, 30); e = p0 + 30
    exp = [(p0, 30, p0 - a)]
    if which.startswith("rep"):
        b.copy(300, 6)                                              # a repeat-offset match (the second offset is the pad's 300) right behind M: inserted at e. The same
        exp.append((e, 6, 300))                                     # six bytes are in the pad's first 300, all inserted: an offset to there says that e was not
        b.put(bytes([b.cont ^ 0x41]) + bytes(b.rng.bytes(6)))
        pos = e
    else:
        b.lit(12)
        pos = {"curr+2 long": p0 + 2, "curr+2 short": p0 + 2, "end-2": e - 2, "end-1": e - 1}[which]
    if which in ("end-2", "rep long"):
        # a decoy. Without it the 8 bytes are found all the same when the long insertion is missing: through the SHORT cell of the same position (rep long) or of the next one
        # (end-2: ip - 1, caught up one byte), as the same sequence. The decoy repeats the 7 bytes that short cell stands for and then differs, so it takes the cell over:
        # only the long cell still leads to the 8 bytes
        k = pos + 1 if which == "end-2" else pos
        b.lit(9); b.put(bytes(b.buf[k:k + 7]) + bytes([b.buf[k + 7] ^ 0x55]))
    b.lit(25)
    q = len(b)
    long_kind = which in ("curr+2 long", "end-2", "rep long")
    if long_kind:
        b.copy(q - pos, 8)
        exp.append((q, 8, q - pos))
    else:
        b.copy(q - pos, 7)
        exp.append((q, 7, q - pos))
    b.lit(30)
    return dict(expect=exp)


INSERTIONS = ("curr+2 long", "curr+2 short", "end-2", "end-1", "rep long", "rep short")


def insertion_sources():
    """Later matches that can only be found through each of the insertions behind a match and each of the two inside the repeat-offset loop."""
    out = []
    for which in INSERTIONS:
        out.append(_mk("insertion %s" % which, _insertion, 1200 + INSERTIONS.index(which), which))
    return out


# ------------------------------------------------------------------------------------------------------------ all of them
def one_block_sources():
    return step_sources() + end_sources() + candidate_sources() + equal_cell_sources() + catch_up_sources() + repeat_offset_sources() + insertion_sources()


EXT_HEAD = 17000


def ext_sources():
    """Sources for ze_dfast_ext (ZSTD_compressBlock_doubleFast_extDict_generic): a raw-content dictionary and a source above the attach cutoff of 16 KiB, or of several blocks, so
    that libzstd copies the dictionary's tables and searches with the dictionary as an external segment. Every source opens with 17 000 bytes of the dictionary's first 300 in a
    period (one match that begins in the dictionary and runs on through the source: the two-segment count), then a one-block case of the families above -- whole, or cut a little
    before its aimed matches with what lay before the cut moved to the dictionary's end, so that the matches, their catch-up and the repeat offsets cross the segment boundary.
    That search has its own step rule (((ip - anchor) >> 8) + 1), writes the long cell of ip + 1 behind every short match and has no parked offsets, so the one-block cases'
    properties do not carry over: these cases assert parity with libzstd only, and what they are aimed at is shown by the mutants of ze_dfast_ext they kill."""
    return [c for _, cases in _ext_groups(1) for c in cases]


def _ext_groups(group):
    """[(dictionary, [cases])]: the whole cases and the two-block ones share ONE dictionary; the cut cases come `group` to a dictionary, which holds all their cut-off parts"""
    rng = np.random.default_rng(1400)
    blob = rng.bytes(300)
    head = (blob * (EXT_HEAD // 300 + 1))[:EXT_HEAD]
    unit = rng.bytes(5000)
    shared = blob + unit[:3000] + bytes(rng.integers(0, 3, 700, dtype=np.uint8))
    whole = step_sources() + candidate_sources() + [c for c in catch_up_sources() if len(c.raw) > PAD] + repeat_offset_sources()[:2] + insertion_sources() + [
        c for c in end_sources() if 4095 <= len(c.raw) <= 4097] + [c for c in equal_cell_sources() if len(c.raw) >= 700]
    first = [Case("ext: " + c.name, head + c.raw, dict_data=shared) for c in whole]
    # of several blocks: from the second block on the tables hold the source's own cells too, and the repeat offsets are the previous block's
    body = b"".join(unit[:4000 + 37 * k] + rng.bytes(50) for k in range(40))
    first.append(Case("ext: two blocks, period 5000 with breaks", (head + body)[:BLOCK + 30000], dict_data=shared))
    first.append(Case("ext: two blocks, alphabet of 3", head + bytes(rng.integers(0, 3, BLOCK, dtype=np.uint8)), dict_data=shared))
    out = [(shared, first)]
    parts = []
    for c in step_sources() + insertion_sources() + candidate_sources():
        cut = max(16, c.expect[1 if c.name.startswith("step") else 0][0] - 24)
        parts.append((c.name, c.raw[max(0, cut - 4096):cut], head + c.raw[cut:]))
    for k in range(0, len(parts), group):
        d = blob + b"".join(x for _, x, _ in parts[k:k + group])
        out.append((d, [Case("ext, cut: " + name, raw, dict_data=d) for name, _, raw in parts[k:k + group]]))
    return out


def ext_batches(group=24):
    """the same sources as a few batches with a dictionary each, for the whole-frame tests: [(dictionary, [sources])]"""
    return [(d, [c.raw for c in cases]) for d, cases in _ext_groups(group)]


DICT_END_SIZES = (64, 65, 72, 80)


def dictionary_batches(group=8):
    """The step family and the end-of-source family (at 64, 65, 72 and 80 bytes) with their match targets moved into a raw-content dictionary: [(dictionary, [sources])]. A case is
    cut a little before its first aimed match: what lies before the cut (at most its last 4 KiB) goes into the dictionary -- behind 300 random bytes and the like of `group` - 1
    other cases --, and the source is 200 of those random bytes (one long match into the dictionary, so that the frame is worth compressing and its sequences are written out)
    and then the case from the cut on."""
    blob = np.random.default_rng(1300).bytes(300)
    parts = []
    for c in step_sources() + [c for c in end_sources() if c.expect and len(c.raw) in DICT_END_SIZES]:
        first = c.expect[1][0] if c.name.startswith("step") else c.expect[0][0]
        cut = max(16, first - 24) if len(c.raw) > 200 else 20
        parts.append((c.raw[max(0, cut - 4096):cut], blob[50:250] + c.raw[cut:]))
    return [(blob + b"".join(d for d, _ in parts[k:k + group]), [r for _, r in parts[k:k + group]]) for k in range(0, len(parts), group)]



FIXTURE = "golden/dfast_sources.bin"


def fixture_cases():
    """what the sanitizer program runs: every one-block aimed source up to 4 200 bytes and one source of two blocks (the sources of a whole block and the windowed ones would
    make the committed file several MiB)"""
    return [c for c in one_block_sources() if len(c.raw) <= 4200] + block_sources()[4:5]


def write_fixture(path):
    """tests/golden/dfast_sources.bin, the input of the stand-alone sanitizer program (emu/build_asan.sh): "DFS1", count, then per source n, windowLog, hashLog, chainLog,
    minMatch (level 3's row as libzstd resolves it for the source), block count, block ends (libzstd's), n bytes"""
    import struct
    from tests.dfast_check import Lz
    lz = Lz()
    cases = fixture_cases()
    with open(path, "wb") as f:
        f.write(b"DFS1" + struct.pack("<I", len(cases)))
        for c in cases:
            cp = lz.cparams(len(c.raw)); ends = [b[2] for b in lz(c.raw)]
            f.write(struct.pack("<6I", len(c.raw), cp["window_log"], cp["hash_log"], cp["chain_log"], cp["min_match"], len(ends)) + struct.pack("<%dI" % len(ends), *ends) + c.raw)
    return len(cases)


if __name__ == "__main__":
    import os
    import sys
    if "--write-fixture" in sys.argv: print(write_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), FIXTURE)), "sources written")
    else: choose_seeds()
