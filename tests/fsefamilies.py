"""Seeded families of frames whose three sequence tables are EXPLICIT choices (test infrastructure for tests/test_emu_sequence_tables.py,
tests/test_gpu_sequence_tables.py and the stand-alone parser program tests/emu/ncount_bounds_main.cpp).

The suite's other frames carry predefined and RLE tables (tests/craft.py before this file) or whatever distributions libzstd's encoder emitted for a
corpus. Here a table is a distribution and an accuracy log (craft.described: mode 2) or a "repeat" of a chosen predecessor (mode 3), and every family
sits on both sides of its limit. plan() draws sequences over the symbols the block's tables hold -- tracking what a "repeat" inherits --, and
FseCase.build() writes the frame and asks tests/fsemodel.py what it decodes to, or why it is refused. Which limits a family reaches is asserted with
fsemodel.census (REQUIRED below) by the tests, never assumed here.

`python -m tests.fsefamilies --write-fixture` writes tests/golden/fse_descriptions.bin: every description of the families (kind, alphabet limit,
length, bytes), the input of the sanitizer program."""
import os
import struct

import numpy as np

from tests import craft, fsemodel, hufmodel, seqmodel
from tests.hufmodel import Refused
from tests.seqfamilies import Case

LL, OF, ML = 0, 1, 2
K3N = fsemodel.KINDS
MAXS, MAXLOG = fsemodel.MAX_SYMBOL, fsemodel.MAX_LOG
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fse_descriptions.bin")


class FseCase(Case):
    """a Case whose expected value comes from fsemodel: the frame's own bytes decoded (tables, states, sequences), then seqmodel.execute"""
    align = None                                               # the offset mod 16 the harness should place the block's bit stream at (16 stands for 0: a true value)

    def __init__(self, family, name, blocks, **kw):
        header = dict(kw.pop("header", None) or {"window_log": 17})
        if "claims" not in header:
            header["claims"] = sum(len(b[1]) if b[0] == "raw" else b[2] if b[0] == "rle" else len(b[1]) + sum(q[1] for q in b[2]) for b in blocks)
        Case.__init__(self, family, name, blocks, header=header, **kw)

    def model_dict(self):
        return self.dict_data if self.dict_data and not self.raw_dict else None

    def build(self, xxh64=None):
        Case.build(self, xxh64)
        self.infos = []
        try:
            content = fsemodel.decode(self.frame, self.model_dict(), self.dict_content(), self.start_reps, self.infos)
            # (a case whose bytes are not the writer's plain output -- a damaged section, raw description bytes, a stream that walks another table -- decodes
            # to what the model reads from the bytes; for every other case the model must read back exactly what the writer was given)
            if self.want is not None and content != self.content:
                assert self.loose(), (self.family, self.name, "the model reads other sequences than the writer was given")
                if len(content) == len(self.content): self.want = self.content = content
                else: self.want, self.why = None, "content size differs from the header's"
            elif self.want is None and self.content is None and len(content) == self.cap: self.want = self.content = content
        except (Refused, seqmodel.Invalid) as e:
            self.want, self.why = None, e.reason
        self.stream_at = [i["stream_at"] for i in self.infos if "stream_at" in i]
        return self

    def loose(self):
        for b in self.blocks:
            o = b[3] if b[0] == "seq" and len(b) > 3 else {}
            if "seq_mangle" in o or any(isinstance(m, dict) and (m["desc"] is not None or m["walk"]) for m in o.get("modes", ())): return True
        return False

    def pad_for(self, arena_pos):
        if self.align is None or not self.stream_at: return 0
        return (self.align - arena_pos - self.stream_at[-1]) % 16

    def with_lead(self):
        h = dict(self.header); h["claims"] += 1
        c = FseCase(self.family, self.name + " [after a raw block]", [("raw", b"L")] + list(self.blocks), dict_data=self.dict_data, raw_dict=self.raw_dict,
                    checksum=self.checksum, start_reps=self.start_reps, header=h)
        if self.dict_data and not self.raw_dict: c.content_off = self.content_off
        c.align = self.align
        return c

    def fse_census(self, base=0):
        return fsemodel.census(self.frame, self.model_dict(), base)


# ------------------------------------------------------------------------------------------------ distributions
def dist(counts, top=None):
    """{symbol: count} -> a count list up to the highest symbol named (or `top`)"""
    n = (max(counts) if top is None else top) + 1
    return [counts.get(s, 0) for s in range(n)]


def even(symbols, log, lows=()):
    """2^log cells shared evenly by `symbols` (the first takes the remainder), `lows` at "less than one" """
    size = (1 << log) - len(lows)
    symbols = [s for s in symbols if s not in lows]
    d = {s: size // len(symbols) for s in symbols}
    d[symbols[0]] += size - sum(d.values())
    assert all(v > 0 for v in d.values()), "more symbols than cells"
    d.update({s: -1 for s in lows})
    return dist(d)


def random_norm(rng, symbols, log):
    size = 1 << log
    cut = sorted(rng.choice(np.arange(1, size), len(symbols) - 1, replace=False).tolist()) if len(symbols) > 1 else []
    counts = [b - a for a, b in zip([0] + cut, cut + [size])]
    d = {}
    for s, c in zip(symbols, counts):
        if c == 1 and rng.integers(0, 2): c = -1
        d[s] = c
    return dist(d)


def bits(*fields):
    """(value, width) fields packed LSB first, as a description's bytes"""
    acc = n = 0
    for v, w in fields: acc |= (v & ((1 << w) - 1)) << n; n += w
    return acc.to_bytes((n + 7) // 8, "little")


_DEFN = {}


def defnorm(kind):
    if kind not in _DEFN: _DEFN[kind] = craft._defnorm(*(("zo_ll_defnorm", 36), ("zo_of_defnorm", 29), ("zo_ml_defnorm", 53))[kind])
    return _DEFN[kind]


SMALL = (list(range(0, 16)), list(range(0, 9)), list(range(0, 32)))          # codes whose sequences stay small: LL up to 15, offsets below 512, ML up to 34


# ------------------------------------------------------------------------------------------------ sequences over chosen tables
class Fse:
    """one table of a block's plan: mode 2 on `norm` at `log`; desc / walk as craft.described; use = the symbols sequences may take (default: all present)"""
    def __init__(self, norm, log, desc=None, walk=None, use=None):
        self.norm, self.log, self.desc, self.walk, self.use = list(norm), log, desc, walk, use


class Rle:
    def __init__(self, sym): self.sym = sym


class Pre:
    """the predefined table, sequences on the symbols `use` only"""
    def __init__(self, use): self.use = use


def _symbols(spec, kind, inherited):
    """(symbols a sequence may take, their weights, what a later repeat inherits) for one table of a plan"""
    if isinstance(spec, Fse):
        norm = spec.walk[0] if spec.walk else spec.norm
        syms = spec.use if spec.use is not None else [s for s, c in enumerate(norm) if c]
        return syms, [max(abs(norm[s]), 1) for s in syms], spec
    if isinstance(spec, Rle): return [spec.sym], [1], spec
    if spec == 3 and inherited is not None: return _symbols(inherited, kind, None)[:2] + (inherited,)
    norm = defnorm(kind)
    syms = spec.use if isinstance(spec, Pre) else [s for s in SMALL[kind] if s < len(norm)]
    return syms, [abs(norm[s]) for s in syms], 0


class Infeasible(Exception):
    pass


def cover(rng, norm, log, n):
    """n codes or more (as many as the visit takes), and the state the LAST of them takes, that lead the decoder through every cell of the table of `norm`: walking backwards from a state,
    each symbol has exactly one cell whose range holds it, and the walk takes a symbol whose such cell is still unvisited while there is one"""
    cells, _, by = craft.fse_table(norm, log)
    hold = {s: [None] * len(cells) for s in by}
    for s, xs in by.items():
        for x in xs:
            for y in range(cells[x][2], cells[x][2] + (1 << cells[x][1])): hold[s][y] = x
    syms = sorted(by)
    cur = last = int(rng.integers(0, len(cells)))
    seen, codes = {cur}, [cells[cur][0]]
    while len(codes) < n or (len(seen) < len(cells) and len(codes) < 40 * len(cells)):
        fresh = [hold[s][cur] for s in syms if hold[s][cur] not in seen]
        cur = fresh[int(rng.integers(0, len(fresh)))] if fresh else hold[syms[int(rng.integers(0, len(syms)))]][cur]
        seen.add(cur); codes.append(cells[cur][0])
    return codes[::-1], last


def draw(rng, tabs, n, have, reps, room=120000, forced=None):
    """n sequences whose codes are drawn over tabs = three (symbols, weights); every offset lies inside the `have` bytes in front and what the
    sequences add (an offset code no history admits yet is not drawn; with none left: Infeasible). Returns (seqs, literal count, new have, new reps)."""
    pick = [np.asarray(t[0])[rng.choice(len(t[0]), n, p=np.asarray(t[1], dtype=float) / sum(t[1]))] for t in (tabs[0], tabs[2])]
    osyms, ow = tabs[1]
    seqs, nlit, made = [], 0, 0
    forced = forced or {}
    for i in range(n):
        lc, mc = int(pick[0][i]), int(pick[1][i])
        if have == 0 and i == 0: lc = max(tabs[0][0])                                   # nothing in front: the longest literal run the table has
        if LL in forced: lc = forced[LL][i]
        if ML in forced: mc = forced[ML][i]
        ll = craft._LL_BASE[lc] + int(rng.integers(0, 1 << min(craft._LL_BITS[lc], 3)))
        ml = craft._ML_BASE[mc] + int(rng.integers(0, 1 << min(craft._ML_BITS[mc], 3)))
        pos = have + ll
        ok = []                                                                          # (code, weight, the offset values that stay inside the history)
        for oc, w in zip(osyms, ow) if OF not in forced else [(forced[OF][i], 1)]:
            if oc >= 2: vals = (1 << oc, min((2 << oc) - 1, pos + 3)) if (1 << oc) - 3 <= pos else None
            else: vals = [v for v in range(1 << oc, 2 << oc) if 0 < seqmodel.next_reps(reps, ll, v)[0] <= pos] or None
            if vals: ok.append((oc, w, vals))
        if not ok: raise Infeasible("no offset code of the table reaches into %d bytes" % pos)
        oc, _, vals = ok[int(rng.choice(len(ok), p=np.asarray([x[1] for x in ok], dtype=float) / sum(x[1] for x in ok)))]
        ofv = int(rng.integers(vals[0], vals[1] + 1)) if oc >= 2 else int(vals[int(rng.integers(0, len(vals)))])
        _, reps = seqmodel.next_reps(reps, ll, ofv)
        seqs.append((ll, ml, ofv)); nlit += ll; have = pos + ml; made += ll + ml
    assert made <= room, "a block of %d bytes" % made
    return seqs, nlit, have, reps


def plan(rng, spec, dict_tabs=None, have=0, reps=(1, 4, 8), opts=None):
    """spec = [("seq", (LL, OF, ML) table specs, n) | ("raw", n) | ("rle", n) | ("noseq", n)] -> the block list of a Case. A table spec is 0
    (predefined: small codes only), Rle(sym), Fse(...) or 3 (repeat: the symbols of what the last block with sequences used)."""
    blocks, inherited = [], dict_tabs
    for b in spec:
        if b[0] == "raw": blocks.append(("raw", bytes(rng.integers(0, 256, b[1], dtype=np.uint8)))); have += b[1]; continue
        if b[0] == "rle": blocks.append(("rle", int(rng.integers(0, 256)), b[1])); have += b[1]; continue
        if b[0] == "noseq": blocks.append(("seq", bytes(rng.integers(0, 256, b[1], dtype=np.uint8)), [], {})); have += b[1]; continue
        got = [_symbols(s, k, inherited[k] if inherited else None) for k, s in enumerate(b[1])]
        extra = dict(b[3]) if len(b) > 3 else {}
        seqs, nlit, have, reps = draw(rng, [g[:2] for g in got], b[2], have, reps, forced=extra.pop("forced", None))
        rest = int(rng.integers(0, 5)); have += rest
        o = {"modes": craft_modes(b[1])}
        o.update(extra); o.update(opts or {})
        blocks.append(("seq", bytes(rng.integers(0, 256, nlit + rest, dtype=np.uint8)), seqs, o))
        inherited = [g[2] for g in got]
    return blocks


def one(family, name, rng, tables, n=24, lead=0, **kw):
    """a frame of one block on `tables` -- behind a raw block of `lead` bytes (600 where the tables' offset codes reach no further than the block's own output)"""
    opts = kw.pop("opts", None)
    try: blocks = plan(rng, ([("raw", lead)] if lead else []) + [("seq", tables, n)], opts=opts)
    except Infeasible: blocks = plan(rng, [("raw", lead or 600), ("seq", tables, n)], opts=opts)
    return FseCase(family, name, blocks, **kw)


def only(kind, t):
    """the table `t` for `kind`, the two others predefined"""
    return tuple(t if k == kind else 0 for k in range(3))


# ------------------------------------------------------------------------------------------------ accuracy logs
def accuracy_logs(seed=1):
    rng = np.random.default_rng(seed)
    cases = []
    for kind in range(3):
        K = fsemodel.KINDS[kind]
        for log in range(5, MAXLOG[kind] + 1):
            cases.append(one("accuracy logs", "%s at log %d" % (K, log), rng, only(kind, Fse(even(SMALL[kind][:8], log), log))))
        over = MAXLOG[kind] + 1
        cases.append(one("accuracy logs", "%s at log %d" % (K, over), rng, only(kind, Fse(even(SMALL[kind][:8], over), over))))
        for nib in (11, 15):                                    # logs 16 and 20: above what any distribution may have
            cases.append(one("accuracy logs", "%s: accuracy-log nibble %d" % (K, nib), rng, only(kind, Fse(defnorm(kind), fsemodel.DEF_LOG[kind], desc=bits((nib, 4), (0x155, 12)), use=SMALL[kind][:8]))))
    top = tuple(Fse(even(SMALL[k][:9], MAXLOG[k]), MAXLOG[k]) for k in range(3))
    cases.append(one("accuracy logs", "all three tables at their highest logs", rng, top, n=60))
    return cases


# ------------------------------------------------------------------------------------------------ alphabets
def alphabets(seed=2):
    rng = np.random.default_rng(seed)
    cases = []

    def fam(name, blocks, **kw): cases.append(FseCase("alphabets", name, blocks, **kw))
    # the top codes in use, with their 16 extra bits: one long sequence each (a block's output stays below 128 KiB, so each in a frame of its own)
    t = Fse(even([3, 35], 6), 6)
    fam("LL code 35 in use", [("raw", b"h" * 40), ("seq", bytes(rng.integers(0, 256, 65536 + 77 + 3, dtype=np.uint8)), [(3, 5, 7), (65536 + 77, 4, 12)], {"modes": craft_modes(only(LL, t))})])
    t = Fse(even([2, 52], 7), 7)
    fam("ML code 52 in use", [("raw", b"h" * 40), ("seq", b"abcdef", [(3, 5, 7), (2, 65539 + 1234, 12)], {"modes": craft_modes(only(ML, t))})])
    t = Fse(even([4, 16], 6), 6)
    fam("offset code 16 in use: the highest the history of a 128 KiB frame admits", [("rle", 7, 70000), ("seq", b"abcdef", [(3, 5, 17), (2, 9, 65536 + 3000)], {"modes": craft_modes(only(OF, t))})])
    for kind, over in ((LL, 36), (OF, 32), (ML, 53)):
        K = fsemodel.KINDS[kind]
        n = even([0, 1, 2, over], 6)
        cases.append(one("alphabets", "a distribution naming %s symbol %d" % (K, over), rng, only(kind, Fse(n, 6, use=[0, 1, 2]))))
        n = even([0, 1, 2, over - 1], 6)
        cases.append(one("alphabets", "a distribution naming %s symbol %d, unused" % (K, over - 1), rng, only(kind, Fse(n, 6, use=[0, 1, 2]))))
    for oc in (29, 30, 31):
        n = even([0, 1, 2, oc], 5)
        cases.append(one("alphabets", "offset code %d named, never used" % oc, rng, only(OF, Fse(n, 5, use=[0, 1, 2]))))
        t = Fse(n, 5)
        fam("offset code %d used: an offset beyond any history" % oc, [("raw", b"h" * 40), ("seq", b"abcdef", [(3, 5, 7), (2, 9, (1 << oc) + 5)], {"modes": craft_modes(only(OF, t))})], header={"window_log": 17, "claims": 60})
    # where the total is reached: at symbol 0 (the single-symbol family's), at symbol 1, at the alphabet's last symbol
    for kind in range(3):
        K = fsemodel.KINDS[kind]
        cases.append(one("alphabets", "%s: the total is reached at symbol 1" % K, rng, only(kind, Fse([40, 24], 6))))
        lastsym = MAXS[kind]
        cases.append(one("alphabets", "%s: the total is reached at the last symbol" % K, rng, only(kind, Fse(even([0, 1, 2, lastsym], 6), 6, use=[0, 1, 2]))))
        for present in (2, 3):
            cases.append(one("alphabets", "%s: %d symbols present" % (K, present), rng, only(kind, Fse(even(SMALL[kind][1:1 + present], 5), 5))))
        every = list(range(lastsym + 1))
        cases.append(one("alphabets", "%s: every symbol present" % K, rng, only(kind, Fse(even(every, 7), 7, use=SMALL[kind]))))
    return cases


def craft_modes(tables):
    return tuple(craft.described(s.norm, s.log, s.desc, s.walk) if isinstance(s, Fse) else 1 if isinstance(s, Rle) else 0 if isinstance(s, Pre) else s for s in tables)


# ------------------------------------------------------------------------------------------------ "less than one" counts
def low_counts(seed=3):
    rng = np.random.default_rng(seed)
    cases = []
    for kind in range(3):
        K = fsemodel.KINDS[kind]
        syms = SMALL[kind][:9]
        for name, lows in (("none", []), ("one", syms[4:5]), ("every symbol but one", syms[1:]), ("the lowest symbols", syms[:3]), ("the highest symbols", syms[-3:])):
            cases.append(one("less than one", "%s: 'less than one': %s" % (K, name), rng, only(kind, Fse(even(syms, 6, lows), 6)), n=40))
    # every cell "less than one": 2^log symbols, which the alphabets hold at log 5 only, and only LL (36 symbols) and ML (53): offsets have 32 symbols
    # but their codes 29 .. 31 reach no history, so the sequences keep to the others
    for kind, use in ((LL, list(range(16))), (ML, list(range(32))), (OF, list(range(9)))):
        cases.append(one("less than one", "%s: all 32 cells 'less than one' at log 5" % fsemodel.KINDS[kind], rng, only(kind, Fse([-1] * 32, 5, use=use)), n=50))
    # as many as an alphabet holds at logs 7 .. 9. (`high` cannot fall below a 64-cell boundary of the table: that takes 64 "less than one" symbols and the
    # largest alphabet has 53. With 52 of them the walk skips positions in EVERY 64-lane trip of zd_build_fse's spread, which is what the ballot numbering feels.)
    for kind in range(3):
        for log in range(7, MAXLOG[kind] + 1):
            every = list(range(MAXS[kind] + 1))
            lows = every[1:]
            cases.append(one("less than one", "%s log %d: %d 'less than one' symbols" % (fsemodel.KINDS[kind], log, len(lows)), rng,
                             only(kind, Fse(even(every, log, lows), log, use=[s for s in SMALL[kind]])), n=50))
    return cases


# ------------------------------------------------------------------------------------------------ one symbol owning the whole table
def single_symbol(seed=4):
    """norm[s] = 2^log: libzstd 1.5.7 reads and builds such a table (every state reads no bits); its encoder would write RLE mode instead"""
    rng = np.random.default_rng(seed)
    cases = []
    for kind in range(3):
        K = fsemodel.KINDS[kind]
        for log in range(5, MAXLOG[kind] + 1):
            for s in (0, MAXS[kind]):
                if kind == OF and s: s = 16                     # (the highest offset code a frame of 128 KiB has the history for)
                name = "%s: symbol %d owns all of log %d" % (K, s, log)
                t = Fse(dist({s: 1 << log}), log)
                if s == 35: blocks = [("raw", b"h" * 40), ("seq", bytes(rng.integers(0, 256, 65536 + 9, dtype=np.uint8)), [(65536 + 9, 4, 12)], {"modes": craft_modes(only(LL, t))})]
                elif s == 52: blocks = [("raw", b"h" * 40), ("seq", b"abc", [(1, 65539 + 9, 12)], {"modes": craft_modes(only(ML, t))})]
                elif s == 16: blocks = plan(rng, [("rle", 66000), ("seq", only(kind, t), 12)])
                else: blocks = plan(rng, [("raw", 600), ("seq", only(kind, t), 12)])
                cases.append(FseCase("single symbol", name, blocks))
                t = Fse(dist({s: (1 << log) - 1, (1 if s == 0 else 0): -1}), log, use=[s] if s in (35, 52) else None)
                if s not in (35, 52, 16): cases.append(one("single symbol", "%s: symbol %d with 2^%d - 1 cells and one 'less than one'" % (K, s, log), rng, only(kind, t), n=12))
    three = (Fse(dist({4: 512}), 9), Fse(dist({5: 256}), 8), Fse(dist({6: 512}), 9))
    cases.append(one("single symbol", "all three tables owned by one symbol at 9 / 8 / 9", rng, three, n=30))
    return cases


# ------------------------------------------------------------------------------------------------ spread and numbering
def spread(seed=5):
    rng = np.random.default_rng(seed)
    cases = []

    def add(name, kind, norm, log, n=None):
        cells = 1 << log
        # (the codes of the aimed table come from cover(): every cell visited, which the census asserts; the two others keep to their smallest codes)
        codes, last = cover(rng, norm, log, n or 2 * cells)
        n = len(codes)
        tabs = tuple(Fse(norm, log) if k == kind else Pre([1, 2, 3]) for k in range(3))
        o = {"forced": {kind: codes}, "seq_last": tuple(last if k == kind else "first" for k in range(3))}
        spec = [("seq", tabs, n, o)]
        try: blocks = plan(rng, spec)
        except Infeasible: blocks = plan(rng, [("raw", 600)] + spec)
        cases.append(FseCase("spread", "%s: %s" % (fsemodel.KINDS[kind], name), blocks))
    for kind in range(3):
        s = SMALL[kind]
        for b in (63, 64, 65):
            add("a symbol boundary at cell %d of the walk" % b, kind, dist({s[0]: b, s[1]: 128 - b - 2, s[2]: 1, s[3]: 1}), 7)
        add("one symbol with 2^log - (n - 1) cells", kind, dist({s[0]: 64 - 7, **{x: 1 for x in s[1:8]}}), 6)
        add("all symbols equal", kind, even(s[:8], 6), 6)
        add("every count a power of two", kind, dist({s[0]: 32, s[1]: 16, s[2]: 8, s[3]: 4, s[4]: 2, s[5]: 1, s[6]: 1}), 6)
        add("powers of two, one off", kind, dist({s[0]: 31, s[1]: 17, s[2]: 8, s[3]: 3, s[4]: 3, s[5]: 1, s[6]: 1}), 6)
        for log in range(5, MAXLOG[kind] + 1):
            add("a random distribution at log %d" % log, kind, random_norm(rng, s[:min(len(s), 5 + log)], log), log)
    return cases


# ------------------------------------------------------------------------------------------------ zero runs
def zero_runs(seed=6):
    rng = np.random.default_rng(seed)
    cases = []
    for run in (0, 1, 2, 3, 4, 6, 9, 12, 27):
        for kind in (LL, ML) if run > 4 else (LL, OF, ML):
            if run + 3 > MAXS[kind]: continue
            norm = dist({0: 20, 1: 0, 2 + run: 30, 3 + run: 14}) if run else dist({0: 20, 1: 0, 2: 30, 3: 14})
            cases.append(one("zero runs", "%s: %d zeros behind a zero count" % (fsemodel.KINDS[kind], run), rng, only(kind, Fse(norm, 6, use=[0] if 2 + run >= len(SMALL[kind]) else [0, 2 + run])), n=16))
    for kind in range(3):
        K, m = fsemodel.KINDS[kind], MAXS[kind]
        # symbols 0 (count), 1 (zero), then a run over 2 .. m - 1 and the rest at the alphabet's last symbol; and the run one longer: past the alphabet
        run = m - 2
        flags = [(3, 2)] * (run // 3) + [(run % 3, 2)]
        good = bits((1, 4), (41, 6), (1, 4), *flags, (31, 5))            # log 6: count 40 in the short form (6 bits), a zero in 4 bits, the run, count 24 in the long form (25 + 6 in 5 bits)
        cases.append(one("zero runs", "%s: a run that ends at the alphabet's last symbol" % K, rng, only(kind, Fse(dist({0: 40, m: 24}), 6, desc=good, use=[0])), n=10))
        run += 1
        flags = [(3, 2)] * (run // 3) + [(run % 3, 2)]
        bad = bits((1, 4), (41, 6), (1, 4), *flags, (31, 5))
        cases.append(one("zero runs", "%s: a run one past the alphabet's last symbol" % K, rng, only(kind, Fse(dist({0: 40, m: 24}), 6, desc=bad, use=[0])), n=10))
    # a chain of 3s that runs past the block's end: the description is the block's last bytes (written behind the stream by the mangle)
    # (LL: 32 flags name 96 symbols, past the alphabet AND past the block; ML: 12 flags name 36, inside the alphabet, and the block ends)
    for kind, ff in ((LL, 8), (ML, 3)):
        chain = bits((1, 4), (41, 6), (1, 4), (3, 2)) + b"\xff" * ff
        c = one("zero runs", "%s: a chain of 3s past the block's end" % fsemodel.KINDS[kind], rng, (0, 0, 0), n=6, opts={"seq_mangle": _replace_modes(kind, chain)})
        cases.append(c)
    return cases


def _replace_modes(kind, tail):
    """a sequences section whose table `kind` turns 'described' and whose bytes behind the modes byte are `tail`, to the block's end"""
    def f(sec):
        m = sec[1] | (2 << (6 - 2 * kind))
        return sec[:1] + bytes([m]) + tail
    return f


# ------------------------------------------------------------------------------------------------ width of a count
def count_widths(seed=7):
    rng = np.random.default_rng(seed)
    cases = []
    for kind in range(3):
        K, s = fsemodel.KINDS[kind], SMALL[kind]
        for log in range(5, MAXLOG[kind] + 1):
            size = 1 << log
            for c in (size - 4, size - 3):                      # the first symbol's count in the short form (value below 2^log - 2) and in the long one
                cases.append(one("count widths", "%s log %d: first count %d" % (K, log, c), rng, only(kind, Fse(dist({s[0]: c, **{x: 1 for x in s[1:1 + size - c]}}), log)), n=20))
            cases.append(one("count widths", "%s log %d: the largest count beside another symbol" % (K, log), rng, only(kind, Fse(dist({s[0]: 1, s[1]: size - 1}), log)), n=20))
        # after the threshold has shrunk: remaining 21 -> threshold 16, 5 bits; max = 31 - 21 = 10: counts 8 (value 9: short) and 9 (value 10: long)
        for c in (8, 9):
            cases.append(one("count widths", "%s: count %d where ten values take the short form" % (K, c), rng, only(kind, Fse(dist({s[0]: 44, s[1]: c, s[2]: 20 - c}), 6)), n=20))
        # (a count above what is left cannot be written: the long form's largest value, 2 * threshold - 1, stands for exactly `remaining`; so zd_read_ncount_to's
        # `remaining < 1` never holds, and the nearest case is the field at its largest value, which completes the total)
        most = bits((1, 4), (41, 6), (31, 5))                   # log 6: count 40, then the 5-bit field at 31 = count 24, all that is left
        cases.append(one("count widths", "%s: a count field at its largest value" % K, rng, only(kind, Fse(dist({0: 40, 1: 24}), 6, desc=most)), n=8))
        short = [1] * (MAXS[kind] + 1)                          # every symbol of the alphabet present once at log 6: the total stays below 64
        if sum(short) < 64: cases.append(one("count widths", "%s: a total below 2^log at the alphabet's last symbol" % K, rng, only(kind, Fse(defnorm(kind), fsemodel.DEF_LOG[kind], desc=craft.ncount(short, 6), use=SMALL[kind][:8])), n=8))
    return cases


# ------------------------------------------------------------------------------------------------ where a description ends
def spelled_zeros(norm, log):
    """the description of `norm` with every zero count written on its own, each behind a zero-run flag of 0: legal, and what no encoder writes"""
    f = [(log - 5, 4)]
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    prev0 = False
    for c in norm:
        if prev0: f.append((0, 2))
        v, mx = c + 1, 2 * threshold - 1 - remaining
        f.append((v, nb - 1) if v < mx else (v, nb) if v < threshold else (v + mx, nb))
        remaining -= abs(c); prev0 = c == 0
        while 1 <= remaining < threshold: nb -= 1; threshold >>= 1
    assert remaining == 1
    return bits(*f)


def longest_description(kind):
    """(norm, log, bytes): the longest description found for `kind` -- one cell for symbol 1, the rest of the table for the alphabet's last symbol, and every
    zero between them spelled out: a count at the full width and a flag each. (A search over the counts -1, 0, 1, 2, 3 and "all that is left" per symbol
    finds nothing longer than 399 / 323 / 586 bits; this one is a few bits below, with symbols a small sequence can use.)"""
    log, m = MAXLOG[kind], MAXS[kind]
    norm = dist({1: 1, m: (1 << log) - 1})
    return norm, log, spelled_zeros(norm, log)


def description_ends(seed=8):
    rng = np.random.default_rng(seed)
    cases = []
    # the last bit of the third description in every bit of its byte: ML distributions of growing length behind fixed LL and OF ones
    seen = set()
    for extra in range(0, 40):
        s = SMALL[ML][:4 + extra % 20]
        norm = even(s, 6 + extra // 20)
        _, endbit = fsemodel.zero_chains(craft.ncount(norm, 6 + extra // 20) + bytes(8))
        if (endbit - 1) % 8 in seen: continue
        seen.add((endbit - 1) % 8)
        t = (Fse(even(SMALL[LL][:5], 5), 5), Fse(even(SMALL[OF][:5], 5), 5), Fse(norm, 6 + extra // 20))
        cases.append(one("description ends", "the third description's last bit in bit %d of its byte" % ((endbit - 1) % 8), rng, t, n=20))
    assert len(seen) == 8, seen
    # one sequence on single-symbol tables: no state bits, no extra bits -- the bit stream is its end mark alone, one byte right behind the descriptions
    # (a described table of log 5 asks five bits for its initial state; the two others in RLE mode ask none)
    t = (Rle(3), Rle(0), Fse(dist({2: 32}), 5))
    cases.append(FseCase("description ends", "a bit stream of one byte behind the third description", [("raw", b"h" * 40), ("seq", b"abcd", [(3, 5, 1)], {"modes": craft_modes(t)})]))
    cases.append(FseCase("description ends", "the third description's last byte is the block's last", [("raw", b"h" * 40), ("seq", b"abcd", [(3, 5, 1)], {"modes": craft_modes(t), "seq_mangle": lambda sec: sec[:-1]})]))
    for k in range(3):                                          # a block cut inside each description: one and two bytes of it left
        full = (Fse(even(SMALL[LL][:9], 7), 7), Fse(even(SMALL[OF][:9], 7), 7), Fse(even(SMALL[ML][:9], 7), 7))
        lens = [len(craft.ncount(f.norm, f.log)) for f in full]
        for keep in (1, lens[k] - 1):
            cut = 2 + sum(lens[:k]) + keep
            cases.append(one("description ends", "a block cut inside the %s description, %d bytes of it left" % (fsemodel.KINDS[k], keep), rng, full, n=12, opts={"seq_mangle": lambda sec, cut=cut: sec[:cut]}))
    # the three longest descriptions in one block
    big = tuple(Fse(n, log, desc=d, use=[1]) for n, log, d in (longest_description(k) for k in range(3)))
    cases.append(one("description ends", "the three longest descriptions in one block", rng, big, n=30))
    return cases


# ------------------------------------------------------------------------------------------------ mixed modes
def _mode_spec(rng, mode, kind, log=6):
    if mode == 0: return 0
    if mode == 1: return Rle(SMALL[kind][int(rng.integers(1, 6))])
    if mode == 2: return Fse(random_norm(rng, SMALL[kind][:7], log), log)
    return 3


def mixed_modes(seed=9):
    rng = np.random.default_rng(seed)
    cases = []
    for first in (0, 1, 2):
        for a in range(4):
            for b in range(4):
                for c in range(4):
                    spec = [("raw", 300), ("seq", tuple(_mode_spec(rng, first, k, 7) for k in range(3)), 10), ("seq", tuple(_mode_spec(rng, m, k) for k, m in enumerate((a, b, c))), 10)]
                    cases.append(FseCase("mixed modes", "modes %d %d %d behind a block of mode %d" % (a, b, c, first), plan(rng, spec)))
    for a, b, c in [(a, b, c) for a in range(4) for b in range(4) for c in range(4) if 3 in (a, b, c)]:       # the 37 combinations with a "repeat" and nothing to repeat
        spec = [("seq", tuple(_mode_spec(rng, m, k) for k, m in enumerate((a, b, c))), 10)]
        cases.append(FseCase("mixed modes", "modes %d %d %d in a frame's first block" % (a, b, c), plan(rng, [("raw", 300)] + spec)))
    return cases


# ------------------------------------------------------------------------------------------------ repeat chains
def repeat_chains(seed=10):
    rng = np.random.default_rng(seed)
    cases = []

    def D(log=6, n=7): return tuple(Fse(random_norm(rng, SMALL[k][:n], min(log, MAXLOG[k])), min(log, MAXLOG[k])) for k in range(3))

    def fam(name, spec): cases.append(FseCase("repeat chains", name, plan(rng, [("raw", 300)] + spec)))
    R = (3, 3, 3)
    fam("described, repeat, repeat", [("seq", D(), 10), ("seq", R, 10), ("seq", R, 10)])
    fam("described at log 9, RLE, repeat: the one-cell table", [("seq", D(9), 10), ("seq", tuple(Rle(SMALL[k][2]) for k in range(3)), 10), ("seq", R, 10)])
    fam("predefined, repeat", [("seq", (0, 0, 0), 10), ("seq", R, 10)])
    fam("repeat across a block without sequences", [("seq", D(), 10), ("noseq", 20), ("seq", R, 10)])
    fam("repeat across a raw block", [("seq", D(), 10), ("raw", 20), ("seq", R, 10)])
    fam("repeat across an RLE block", [("seq", D(), 10), ("rle", 20), ("seq", R, 10)])
    fam("repeat in block 2 when block 1 had no sequences", [("noseq", 20), ("seq", R, 10)])
    fam("repeat behind a raw block only", [("seq", R, 10)])
    for k in range(3):
        other = D(5 + k)
        fam("a repeat of %s alone, the others described anew at log %d" % (fsemodel.KINDS[k], 5 + k), [("seq", D(8), 10), ("seq", tuple(3 if j == k else other[j] for j in range(3)), 10)])
    return cases


# ------------------------------------------------------------------------------------------------ dictionaries
def dictionary_frames(trained, content_off, reps=(1, 4, 8), seed=11):
    """(name, cases) with the trained dictionary of tests/golden, and with its bytes as a raw-content dictionary for contrast"""
    rng = np.random.default_rng(seed)
    dt = fsemodel.dictionary_tables(trained)
    # what a "repeat" of the dictionary's tables draws from: its distributions, the small codes only
    inh = [Fse(t.norm, t.log, use=[s for s in SMALL[k] if s < len(t.norm) and t.norm[s]]) for k, t in enumerate(dt)]
    writer_tabs = [craft.fse_table(t.norm, t.log) for t in dt]
    dict_id = struct.unpack("<I", trained[4:8])[0]
    have = len(trained) - content_off
    R = (3, 3, 3)

    def D(log=6): return tuple(Fse(random_norm(rng, SMALL[k][:7], log), log) for k in range(3))
    specs = [("every table repeat in the first block", [("seq", R, 12)]),
             ("block 1 described, block 2 repeat: block 1's tables", [("seq", D(), 12), ("seq", R, 12)]),
             ("block 1 all repeat, block 2 described, block 3 repeat", [("seq", R, 12), ("seq", D(7), 12), ("seq", R, 12)])]
    for k in range(3):
        for others, what in ((0, "predefined"), (1, "RLE"), (2, "described")):
            tabs = tuple(3 if j == k else _mode_spec(rng, others, j) for j in range(3))
            specs.append(("%s repeat, the others %s" % (fsemodel.KINDS[k], what), [("seq", tabs, 12)]))
            tabs = tuple(_mode_spec(rng, others, j) if j == k else 3 for j in range(3))
            specs.append(("%s %s, the others repeat" % (fsemodel.KINDS[k], what), [("seq", tabs, 12)]))
    out = []
    for raw in (False, True):
        cases = []
        for name, spec in specs:
            blocks = plan(rng, spec, dict_tabs=inh, have=have, reps=reps)
            header = {"window_log": 17, "dict_tables": writer_tabs}
            if not raw: header["dict_id"] = dict_id
            c = FseCase("dictionaries", name + (" [raw-content dictionary]" if raw else ""), blocks, dict_data=trained[content_off:] if raw else trained, raw_dict=raw, start_reps=reps, header=header)
            if not raw: c.content_off = content_off
            cases.append(c)
        out.append(("raw content" if raw else "trained", cases))
    return out


# ------------------------------------------------------------------------------------------------ bit rate
def _rate_tables():
    """logs 9 / 8 / 9 with every symbol but the last at "less than one": a sequence on those symbols reads 9 + 8 + 9 state bits"""
    return (Fse(dist({**{s: -1 for s in range(35)}, 35: 512 - 35}), 9, use=[16, 20, 24]),          # LL 16 .. 63: 1, 2, 4 extra bits
            Fse(dist({**{s: -1 for s in range(31)}, 31: 256 - 31}), 8, use=[16]),                  # offsets of 64 KiB and up: the largest code a frame of 128 KiB has the history for
            Fse(dist({**{s: -1 for s in range(52)}, 52: 512 - 52}), 9, use=[36, 40, 42]))          # ML 43 .. 130: 2, 4, 5 extra bits


def heaviest_window(content=131072):
    """(bits, [(LL extra bits, ML extra bits, offset code)] x 4): the four consecutive steps that read the most bits in a frame of at most `content` bytes --
    26 state bits, the offset code the bytes in front admit, and the largest code of each extra-bit count for both lengths, by exhaustive search over the
    length codes of four sequences and the bytes in front of them (a fifth, small sequence follows: the fourth step's state update needs one)"""
    llb = {craft._LL_BITS[c]: craft._LL_BASE[c] for c in range(36)}
    mlb = {craft._ML_BITS[c]: craft._ML_BASE[c] for c in range(53)}
    best = (0, None, None)
    for lead in sorted({0} | {max(0, 65533 - v) for v in llb.values()}):
        layer = {lead: (0, [])}
        for _ in range(4):
            nxt = {}
            for have, (got, path) in layer.items():
                for a in range(9, 17):
                    for m in range(9, 17):
                        pos = have + llb[a]; end = pos + mlb[m]
                        if end + 4 > content: continue
                        oc = min(16, (pos + 3).bit_length() - 1)
                        if end not in nxt or nxt[end][0] < got + 26 + oc + a + m: nxt[end] = (got + 26 + oc + a + m, path + [(a, m, oc)])
            layer = nxt
        for got, path in layer.values():
            if got > best[0]: best = (got, path, lead)
    return best


HEAVIEST = [(15, 14, 15), (14, 13, 16), (13, 13, 16), (14, 14, 16)]       # heaviest_window()'s answer, in front of nothing: 277 bits (pinned by the tests)


def _burst(rng, steps, lead=0, tail=1, tables=None):
    """blocks: `lead` bytes of an RLE block, then one block whose sequences take `steps` = [(LL extra bits, ML extra bits, offset code)] on the all-low
    tables of logs 9 / 8 / 9 (the largest code of each width, small extra values so that the sizes stay at the codes' bases) and `tail` small sequences"""
    llc = {craft._LL_BITS[c]: c for c in range(36)}; mlc = {craft._ML_BITS[c]: c for c in range(53)}
    seqs, have = [], lead
    for a, m, oc in list(steps) + [(0, 0, 16)] * tail:
        ll = craft._LL_BASE[llc[a]] + (int(rng.integers(0, 200)) if a >= 8 else 3 if a == 0 else 0)
        ml = craft._ML_BASE[mlc[m]] + (int(rng.integers(0, 200)) if m >= 8 else 0)
        pos = have + ll
        ofv = int(rng.integers(1 << oc, min((2 << oc) - 1, pos + 3) + 1))
        assert ofv - 3 <= pos
        seqs.append((ll, ml, ofv)); have = pos + ml
    assert have <= 131072, have
    blocks = [("rle", 7, lead)] if lead else []
    return blocks + [("seq", bytes(rng.integers(0, 256, sum(q[0] for q in seqs) + 2, dtype=np.uint8)), seqs, {"modes": craft_modes(tables or _rate_tables())})]


def bit_rate(seed=12):
    rng = np.random.default_rng(seed)
    cases = []
    zero = (Fse(dist({9: 512}), 9), Fse(dist({8: 256}), 8), Fse(dist({7: 512}), 9))
    n, lead = 400, 66000
    light = (Fse(_rate_tables()[0].norm, 9, use=SMALL[LL]), Fse(_rate_tables()[1].norm, 8, use=SMALL[OF]), Fse(_rate_tables()[2].norm, 9, use=SMALL[ML]))

    def fam(name, blocks, align=None):
        c = FseCase("bit rate", name, blocks, header={"window_log": 21})
        c.align = align
        cases.append(c)
    # The most a valid frame of 128 KiB asks of K2's bit ring. One step: 26 state bits, offset code 16 and LL 35 + ML 51 (16 + 15 extra bits) -- 73 bits; LL 35 + ML 52 is
    # three bytes above 128 KiB, and LL 34 + ML 52 behind the 32 765 bytes its offset code needs fills the frame to its last byte: no sequence could follow. Four consecutive steps (the ring is fed one burst of four ahead): 277 bits,
    # heaviest_window()'s search. Both at every offset mod 16 of the stream's first byte.
    for a in range(16):
        fam("the heaviest four steps a frame of 128 KiB holds, the stream's first byte at %d mod 16" % a, _burst(rng, HEAVIEST), align=a or 16)
    top = (Fse(dist({0: 512 - 35, **{x: -1 for x in range(1, 36)}}), 9),) + _rate_tables()[1:]          # (LL code 35 among the "less than one" symbols: symbol 0 takes the rest)
    fam("the heaviest step: LL code 35 and ML code 51", _burst(rng, [(16, 15, 16)], tables=top))
    fam("seven steps on LL code 31, ML code 48 and offset code 16", _burst(rng, [(12, 12, 16)] * 7, lead=65533))
    fam("26 state bits a step over 400 sequences with 16 offset bits", plan(rng, [("rle", lead), ("seq", _rate_tables(), n)]))
    fam("26 state bits a step, 3 000 sequences on small codes", plan(rng, [("rle", 4000), ("seq", light, 3000)]))
    fam("no state bits in any step", plan(rng, [("rle", 4000), ("seq", zero, 2000)]))
    fam("the two alternating", plan(rng, [("rle", lead)] + [("seq", _rate_tables() if i % 2 == 0 else zero, 60) for i in range(6)]))
    return cases


# ------------------------------------------------------------------------------------------------ initial states and the last sequence
def initial_states(seed=13):
    rng = np.random.default_rng(seed)
    cases = []
    for kind in range(3):
        K, s = fsemodel.KINDS[kind], SMALL[kind]
        norm = even(s[1:8], 6)
        cells = craft.fse_table(norm, 6)[0]
        for st, what in ((0, "0"), (63, "2^log - 1")):
            # one sequence only: its three states are the initial states, chosen freely
            seq = {LL: (cells[st][0], 5, 7), OF: (3, 5, 1 << cells[st][0]), ML: (3, craft._ML_BASE[cells[st][0]], 7)}[kind]
            first = tuple(st if k == kind else None for k in range(3))
            cases.append(FseCase("initial states", "%s: initial state %s, one sequence" % (K, what), [("raw", b"h" * 600), ("seq", b"abcdefghijklmnop"[:seq[0] + 1], [seq], {"modes": craft_modes(only(kind, Fse(norm, 6))), "seq_last": first, "seq_first": first})]))
    blocks = plan(rng, [("raw", 300), ("seq", tuple(Fse(even(SMALL[k][:6], 6), 6) for k in range(3)), 9)])
    cases.append(FseCase("initial states", "a stream with eight bits left over", blocks[:1] + [blocks[1][:3] + (dict(blocks[1][3], seq_mangle=lambda sec: sec[:-1] + bytes([0, sec[-1]])),)]))
    cases.append(FseCase("initial states", "a stream one bit short", blocks[:1] + [blocks[1][:3] + (dict(blocks[1][3], seq_mangle=_drop_top_bit),)]))
    cases.append(FseCase("initial states", "the same stream as written", blocks))
    for choice in ("most", "least"):                            # the last sequence on the state of its symbols that reads the most / the fewest bits when it is reached
        cases.append(FseCase("initial states", "the last sequence on the state with the %s bits" % choice, blocks[:1] + [blocks[1][:3] + (dict(blocks[1][3], seq_last=choice),)]))
    # descriptions the stream does not follow: the states walk another distribution over the same symbols (libzstd's verdict decides: other sequences of the
    # same total, or a refusal)
    for k in range(3):
        told, walked = even(SMALL[k][1:7], 6), even(SMALL[k][1:7][::-1], 6, lows=SMALL[k][1:2])
        tabs = only(k, Fse(told, 6, walk=(walked, 6)))
        cases.append(FseCase("initial states", "a %s description the stream does not follow" % K3N[k], plan(rng, [("raw", 300), ("seq", tabs, 9)])))
    return cases


def _drop_top_bit(sec):
    """the end mark moved one bit down: the first field read loses its top bit and everything behind it shifts"""
    v = int.from_bytes(sec[-2:], "little")
    top = v.bit_length() - 1
    v = (v & ((1 << (top - 1)) - 1)) | (1 << (top - 1))
    return sec[:-2] + (v.to_bytes(2, "little") if v >> 8 else bytes([v & 255]))


# ------------------------------------------------------------------------------------------------ K2 groups
def k2_groups(seed=14):
    """(name, cases): batches of 1 / 14 / 15 / 16 / 31 frames with different logs per frame (5 / 5 / 5 beside 9 / 8 / 9, single-symbol tables, predefined),
    refused members among them"""
    rng = np.random.default_rng(seed)

    def member(i):
        w = i % 5
        if w == 0: t = tuple(Fse(even(SMALL[k][:6], 5), 5) for k in range(3))
        elif w == 1: t = tuple(Fse(random_norm(rng, SMALL[k][:9], MAXLOG[k]), MAXLOG[k]) for k in range(3))
        elif w == 2: t = (0, 0, 0)
        elif w == 3: t = (Fse(dist({15: 512}), 9), Fse(dist({3: 256}), 8), Fse(dist({6: 512}), 9))      # (15 literals in front of every match: offsets of 5 .. 12 reach no further)
        else: t = tuple(Fse(even(SMALL[k][:8], 10), 10) if k == i % 3 else Fse(even(SMALL[k][:8], 7), 7) for k in range(3))      # refused: a log above the kind's maximum
        return FseCase("K2 groups", "member %d (kind %d)" % (i, w), plan(rng, [("seq", t, 30 + i)]))
    return [("%d frames" % n, [member(i) for i in range(n)]) for n in (1, 14, 15, 16, 31)]


def k2_dictionary_groups(trained, content_off, reps=(1, 4, 8), seed=15):
    """(name, cases) under the trained dictionary: 1 / 14 / 15 / 16 / 31 frames of one block whose tables are all the dictionary's (the shared copy) beside
    frames that describe their own at logs 5 and 9 / 8 / 9, one and two of three "repeat", and refused ones"""
    rng = np.random.default_rng(seed)
    dt = fsemodel.dictionary_tables(trained)
    inh = [Fse(t.norm, t.log, use=[x for x in SMALL[k] if x < len(t.norm) and t.norm[x]]) for k, t in enumerate(dt)]
    header = {"window_log": 17, "dict_tables": [craft.fse_table(t.norm, t.log) for t in dt], "dict_id": struct.unpack("<I", trained[4:8])[0]}

    def member(i):
        w = i % 5
        if w in (0, 2): t = (3, 3, 3)
        elif w == 1: t = tuple(Fse(random_norm(rng, SMALL[k][:9], MAXLOG[k]), MAXLOG[k]) for k in range(3))
        elif w == 3: t = tuple(3 if k == i % 3 else Fse(even(SMALL[k][:6], 5), 5) for k in range(3))
        else: t = tuple(Fse(even(SMALL[k][:8], 10), 10) if k == i % 3 else 3 for k in range(3))              # refused: a log above the kind's maximum
        c = FseCase("K2 groups", "dictionary member %d (kind %d)" % (i, w), plan(rng, [("seq", t, 20 + i)], dict_tabs=inh, have=len(trained) - content_off, reps=reps),
                    dict_data=trained, raw_dict=False, start_reps=reps, header=dict(header))
        c.content_off = content_off
        return c
    return [("%d frames" % n, [member(i) for i in range(n)]) for n in (1, 14, 15, 16, 31)]


MOST_BITS = 26 + 16 + 16 + 15        # one step: the state bits of logs 9 / 8 / 9, offset code 16, LL code 35 and ML code 51: what a frame of 128 KiB can hold
MOST_WINDOW = 277                    # four consecutive steps: heaviest_window()


FAMILIES = {
    "accuracy logs": accuracy_logs, "alphabets": alphabets, "less than one": low_counts, "single symbol": single_symbol, "spread": spread, "zero runs": zero_runs,
    "count widths": count_widths, "description ends": description_ends, "mixed modes": mixed_modes, "repeat chains": repeat_chains, "bit rate": bit_rate,
    "initial states": initial_states,
}

REQUIRED = {
    "accuracy logs": ["%s log %d" % (fsemodel.KINDS[k], log) for k in range(3) for log in range(5, MAXLOG[k] + 1)] + ["K2 slot filled: 512 + 512 + 256 cells"],
    "alphabets": ["LL top code in use", "ML top code in use", "LL highest symbol 35", "OF highest symbol 31", "ML highest symbol 52", "OF highest symbol 1",
                  "LL symbols present: 2", "OF symbols present: 3", "ML symbols present: all", "LL symbols present: all", "OF symbols present: all"],
    "less than one": ["%s 'less than one' symbols: %s" % (K, n) for K in fsemodel.KINDS for n in ("none", "one", "all but one symbol", "several")] + [
        "LL 'less than one' symbols: all cells", "ML 'less than one' symbols: all cells", "'less than one' at the lowest symbols", "'less than one' at the highest symbols",
        "LL log 9: 35 'less than one' symbols", "ML log 9: 52 'less than one' symbols", "OF log 8: 31 'less than one' symbols", "ML log 7: 52 'less than one' symbols"],
    "single symbol": ["K2 cell with x = 1023 beside symbol 52", "a step that reads no state bits", "LL single-symbol table of log 9, symbol 35", "LL single-symbol table of log 5, symbol 0",
                      "OF single-symbol table of log 8, symbol 0", "ML single-symbol table of log 9, symbol 0", "K2 slot filled: 512 + 512 + 256 cells"],
    "spread": ["every cell of a %s log-%d table visited" % (fsemodel.KINDS[k], log) for k in range(3) for log in range(5, MAXLOG[k] + 1)],
    "zero runs": ["zero-run flags %s" % f for f in ("0", "1", "2", "3,0", "3,1", "3,3,0", "3,3,3,0", "3,3,3,3,0")],
    "count widths": ["%s %s count in the %s form" % (K, w, f) for K in fsemodel.KINDS for w in ("first", "later") for f in ("short", "long")],
    "description ends": ["bit stream of one byte", "description bytes in a block: 100 and up", "description bytes in a block: 1..31"],
    "mixed modes": ["modes %d %d %d" % (a, b, c) for a in range(4) for b in range(4) for c in range(4)] + ["repeat of a predefined table", "repeat of a RLE table", "repeat of a described table"],
    "repeat chains": ["repeat of a predefined table", "repeat of a RLE table", "repeat of a described table"],
    "bit rate": ["state bits in a step: 26", "a step that reads no state bits", "K2 slot filled: 512 + 512 + 256 cells", "bits in a step, extra bits included: %d" % MOST_BITS] + [
        "bits in four consecutive steps: %d, the stream's first byte at %d mod 16" % (MOST_WINDOW, a) for a in range(16)],
    "initial states": ["%s initial state %s" % (K, w) for K in fsemodel.KINDS for w in ("0", "the last", "inside")] + ["one sequence"],
    "dictionaries": ["repeat of a dictionary table", "repeat of a described table"],
    "K2 groups": ["K2 group of %d frames" % n for n in (1, 14, 15, 16, 31)] + ["K2 group: logs 5 5 5 beside 9 8 9", "K2 group: a refused frame among the others"],
    "K2 dictionary groups": ["K2 group of %d frames" % n for n in (1, 14, 15, 16, 31)] + ["K2 group: shared dictionary tables beside described ones", "K2 group: a refused frame among the others"],
}
# the reasons each family's refused frames must be refused for (every one of them libzstd's verdict too: the tests hold the model against it first)
REFUSALS = {
    "accuracy logs": {"LL table: accuracy log 10 above 9", "OF table: accuracy log 9 above 8", "ML table: accuracy log 10 above 9"} | {"%s table: distribution: accuracy log above 15" % K for K in fsemodel.KINDS},
    "alphabets": {"LL table: distribution: a symbol above the alphabet", "offset beyond the history"},
    "zero runs": {"%s table: distribution: a symbol above the alphabet" % K for K in fsemodel.KINDS} | {"ML table: distribution: runs past the description"},
    "count widths": {"LL table: distribution: does not total 2^log", "OF table: distribution: does not total 2^log", "ML table: distribution: does not total 2^log"},
    "description ends": {"sequences: no bit stream behind the tables"},
    "mixed modes": {"%s table: repeat with nothing to repeat" % K for K in fsemodel.KINDS},
    "repeat chains": {"LL table: repeat with nothing to repeat"},
    "initial states": {"sequences: bits left over"},
}


def all_descriptions():
    """every mode-2 description the families write, as (kind, bytes from its first byte to the block's end, at most the 256 staged): the sanitizer program's input"""
    out, seen = [], set()
    for gen in FAMILIES.values():
        for c in gen():
            c.build(lambda b: 0)
            for t, pos, size, _ in hufmodel.walk(c.frame):
                if t != 2: continue
                buf = c.frame[pos:pos + size]
                try: _, used, _ = hufmodel.literals_section(buf, None)
                except Refused: continue
                sec = buf[used:]
                if len(sec) < 3 or sec[0] == 0 or sec[0] > 127: continue
                at, modes = 2, sec[1]
                for kind, sh in enumerate((6, 4, 2)):
                    m = (modes >> sh) & 3
                    if m == 1: at += 1
                    if m == 2:
                        rest = sec[at:at + fsemodel.STAGED]
                        if (kind, rest) not in seen: seen.add((kind, rest)); out.append((kind, rest))
                        try: at += fsemodel.read_table(sec[at:], kind).used
                        except Refused: break
    return out


def write_fixture(path=FIXTURE):
    """count, then per description: kind, alphabet limit, length (2 bytes), the bytes"""
    ds = sorted(set(all_descriptions()))                       # (each with what follows it in its block, up to the 256 bytes K0 and K1 stage)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(ds)))
        for k, d in ds: f.write(struct.pack("<BBH", k, MAXS[k], len(d)) + d)
    return len(ds)


if __name__ == "__main__":
    import sys
    if "--write-fixture" in sys.argv: print(write_fixture(), "descriptions ->", FIXTURE)
