"""Sequence lists that aim at the decisions of the ENTROPY kernel (ze_entropy_body / ze_frame<false> / ze_compress_block<false>, and the trailer kernel behind
it), for tests/test_emu_entropy_sequences.py, tests/test_gpu_entropy_sequences.py and tests/stress_emu_entropy_sequences.py (test infrastructure).

Every generator is deterministic (seeded) and returns Cases: ONE block described by explicit sequences (litLength, matchLength, raw offset) and its literal
bytes. The source is what the list decodes to (seqmodel.execute), so the list always reproduces it; the expected frame is libzstd's ZSTD_compressSequences
on the same list (reflib.RefZstd.compress_sequences), never a normal compress call. A case is handed to the kernels in two forms (Case.form): "canonical" --
seqmodel.canonical, the reference runs with ZSTD_c_searchForExternalRepcodes enabled -- and "plain" -- every offset as offset + 3, the reference runs with
it disabled.

Each family names the limit it straddles and has cases on both sides; where a decision cannot be read back from a frame (which normalisation path ran) the
family sweeps instead. What the families reach together is asserted by the tests from frame_census() over the REFERENCE's frames.

libzstd's own bounds on a list, which a generator must respect because a case the reference refuses is a generator bug: fewer than srcSize / 4 sequences
(srcSize / 3 where the level's minMatch is 3: its sequence store is sized from the block), lengths that sum to the source, at most one length above 65 535
per block (the one-long-length flag)."""
import struct

import numpy as np

from tests import seqmodel

BLOCK_MAX = seqmodel.BLOCK_MAX
# the format's length code tables (RFC 8878 3.1.1.3.2.1.1): the smallest length of every code
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
SEQ_CAPACITY = 43704          # sequences a one-block arena slot holds (ZE_SEQ_CAP; pinned against the header by the emulator test)
INVALID = 107                 # externalSequences_invalid
UNSUPPORTED = 40


class Config:
    """what a context is set up with: one Config = one batch (one zhip_ctx_set_cparams state)"""
    def __init__(self, level=3, content_size=True, checksum=False, magicless=False, dict_name=None, **params):
        self.level, self.content_size, self.checksum, self.magicless, self.dict_name, self.params = level, content_size, checksum, magicless, dict_name, dict(params)

    def key(self):
        return (self.level, self.content_size, self.checksum, self.magicless, self.dict_name, tuple(sorted(self.params.items())))

    def flags(self):
        return (1 if self.content_size else 0) | (2 if self.checksum else 0) | 4

    def with_checksum(self):
        return Config(self.level, self.content_size, True, self.magicless, self.dict_name, **self.params)

    def __repr__(self):
        return "level %d%s%s%s%s%s" % (self.level, "" if self.content_size else ", no content size", ", checksum" if self.checksum else "", ", magicless" if self.magicless else "",
                                       ", dictionary %s" % self.dict_name if self.dict_name else "", "".join(", %s=%d" % kv for kv in sorted(self.params.items())))


DEFAULT = Config()


class Case:
    def __init__(self, family, name, seqs, lits, cfg=DEFAULT, refused=None, route=None, ref_refuses=False):
        """seqs: [(ll, ml, raw offset)]; lits: all literal bytes, the last run included; refused: None or the status the LOADER must give (the list is then handed
        over as it is, and `source` says which bytes go with it); route: None = both loader routes, 0 / 1 = that one only (the near-full-block cases)"""
        self.family, self.name, self.seqs, self.lits, self.cfg, self.refused, self.route = family, name, list(seqs), bytes(lits), cfg, refused, route
        self.source, self.ref_refuses = None, ref_refuses            # ref_refuses: libzstd checks the same thing and must refuse the list too

    def build(self, dicts):
        """.source, .tail, and the two forms' code lists; dicts: {name: (bytes, content offset, repeat offsets, raw)}"""
        if self.refused is not None:
            if self.source is None: self.source = self.lits
            return self
        content, reps = b"", (1, 4, 8)
        if self.cfg.dict_name:
            d, off, reps, _ = dicts[self.cfg.dict_name]
            content = d[off:]
        blk = [("seq", self.lits, [(ll, ml, o + 3) for ll, ml, o in self.seqs], {})]
        try:
            self.source = seqmodel.execute(blk, content, reps)
        except seqmodel.Invalid as e:
            raise AssertionError("GENERATOR BUG, not a kernel: %s / %s: %s" % (self.family, self.name, e.reason))
        assert len(self.source) <= BLOCK_MAX, (self.family, self.name, "more than one block")
        self.tail = len(self.lits) - sum(q[0] for q in self.seqs)
        self._forms = {"plain": seqmodel.plain(blk, reps)[0][2], "canonical": seqmodel.canonical(blk, reps)[0][2]}
        for form, codes in self._forms.items():
            assert seqmodel.execute([("seq", self.lits, codes, {})], content, reps) == self.source, ("TEST MODEL, not a kernel", self.family, self.name, form)
        return self

    def form(self, form):
        """the list as the kernel takes it: [(offBase, litLength, matchLength)]"""
        if self.refused is not None: return [(o, ll, ml) for ll, ml, o in self.seqs]              # handed over verbatim (o is an offBase here)
        return [(c, ll, ml) for ll, ml, c in self._forms[form]]

    def packed(self, form):
        q = self.form(form)
        if not q: return np.zeros(0, dtype=np.uint64)
        a = np.array(q, dtype=np.uint64)
        return a[:, 0] | (a[:, 1] << np.uint64(28)) | (a[:, 2] << np.uint64(46))


# ------------------------------------------------------------------------------------------------------------------ literal bytes
_TEXT = None


def set_text_source(sample):
    """literal bytes of kind "text" are drawn from `sample` (a dictionary's own content: literals whose statistics are close to its Huffman table's)"""
    global _TEXT
    _TEXT = np.frombuffer(sample, dtype=np.uint8)


def lit_bytes(rng, n, kind="skew"):
    """n literal bytes: "rle" one value; "two" two values; "uniform" all 256 (not compressible); "skew" values 0..100, low ones likelier (a Huffman table fits);
    "geom" geometric over 256 values; "text" drawn byte by byte from set_text_source's sample, "slice" a contiguous stretch of it; ("alphabet", k) k values, near uniform; ("fib", k) k values with
    Fibonacci-like counts (code lengths above 11 before limiting), n is then ignored"""
    if kind == "slice":                                                          # a contiguous stretch of the sample: its statistics as they are
        if n == 0: return b""
        assert _TEXT is not None and len(_TEXT) > n + 64, "set_text_source first"
        at = int(rng.integers(0, len(_TEXT) - n))
        return bytes(_TEXT[at:at + n])
    if kind == "text":
        if n == 0: return b""
        assert _TEXT is not None and len(_TEXT) > 64, "set_text_source first"
        return bytes(_TEXT[rng.integers(0, len(_TEXT), n)])
    if isinstance(kind, tuple) and kind[0] == "fib":
        c, a, b = [], 1, 1
        for _ in range(kind[1]): c.append(a); a, b = b, a + b
        v = np.repeat(np.arange(len(c), dtype=np.uint8) * 3 + 1, c)
        rng.shuffle(v)
        return bytes(v)
    if n == 0: return b""
    if kind == "rle": return bytes([int(rng.integers(0, 256))]) * n
    if kind == "two": return bytes(rng.choice(np.array([65, 200], dtype=np.uint8), n, p=[0.8, 0.2]))
    if kind == "uniform": return bytes(rng.integers(0, 256, n, dtype=np.uint8))
    if kind == "geom": return bytes(np.minimum(rng.geometric(0.06, n) - 1, 255).astype(np.uint8))
    if isinstance(kind, tuple) and kind[0] == "alphabet":
        k = kind[1]
        v = rng.integers(0, k, n).astype(np.uint8)
        v[:min(k, n)] = np.arange(min(k, n), dtype=np.uint8)                   # every symbol at least once where they fit
        return bytes((v.astype(np.uint16) * (255 // max(k - 1, 1))).astype(np.uint8)) if k <= 128 else bytes(v)
    return bytes(np.minimum(rng.integers(0, 101, n), rng.integers(0, 101, n)).astype(np.uint8))


def mk(family, name, seqs, rng, kind="skew", tail=0, cfg=DEFAULT, route=None):
    n = sum(q[0] for q in seqs) + tail
    lits = lit_bytes(rng, n, kind)
    if isinstance(kind, tuple) and kind[0] == "fib": assert len(lits) == n, (len(lits), n)
    return Case(family, name, seqs, lits, cfg, route=route)


def cycle_offsets(base, i):
    """four offsets of one offset code that never meet the repeat-offset history (three entries) nor 'entry one minus one': spaced two apart, used in turn"""
    return base + 2 * (i % 4)


def plain_seqs(rng, n, ll=(0, 9), ml=(3, 9), lead=40):
    """n unremarkable sequences: a first literal run of `lead` bytes, then short runs (some empty) and matches at offsets inside what exists, a third of them at
    one of the three offsets used last (repeat codes in the canonical form)"""
    out, pos, used = [], 0, []
    for i in range(n):
        l = lead if i == 0 else int(rng.integers(ll[0], ll[1] + 1)); m = int(rng.integers(ml[0], ml[1] + 1))
        pos += l
        off = used[-1 - int(rng.integers(0, min(len(used), 3)))] if used and rng.random() < 0.35 else int(rng.integers(1, min(pos, 60000) + 1))
        out.append((l, m, off)); used.append(off)
        pos += m
    return out


# ------------------------------------------------------------------------------------------------------------------ families
def sequence_counts(seed=101):
    """the sequence-count header (1 byte below 128, 2 below 0x7F00, 3 from there), the eight-step loop of the three state chains and its remainder
    (every count 1..17), a block without sequences, and the slot's capacity"""
    rng = np.random.default_rng(seed)
    F, cases = "sequence counts", []
    cases.append(mk(F, "no sequences: literals only", [], rng, tail=300))
    for n in list(range(1, 18)) + [126, 127, 128, 129]:
        cases.append(mk(F, "%d sequences" % n, plain_seqs(rng, n), rng, tail=n % 3))
    # literal length <= 1 and match length 3: 0x7F01 sequences are 130 052 bytes at most. One source each, one loader route (a full block under the emulator is slow)
    for k, n in enumerate((0x7EFF, 0x7F00, 0x7F01)):
        # (every literal length 1 and 600 last literals: libzstd takes a list only while it is shorter than a quarter of the source)
        seqs = [(1, 3, 1)] + [(1, 3, 1 + int(o)) for o in rng.integers(0, 3, n - 1)]
        cases.append(mk(F, "%#x sequences" % n, seqs, rng, tail=600, route=k % 2))
    # the capacity itself cannot be reached by a valid list (43 704 matches of 3 bytes are 131 112 bytes): the longest valid list is 43 690 sequences, which libzstd's
    # sequence store (a third or a quarter of the block) refuses -- so the cases at the limit are refusals: one by the sum at the capacity, one by the count above it
    src = lit_bytes(rng, BLOCK_MAX, "skew")
    for n, why in ((SEQ_CAPACITY, "the capacity: refused for the lengths' sum"), (SEQ_CAPACITY + 1, "one above the capacity: refused for the count")):
        c = Case(F, "%d sequences, %s" % (n, why), [(0, 3, 4)] * n, src, refused=INVALID, route=0, ref_refuses=True)
        cases.append(c)
    return cases


def _hist_seqs(rng, table, codes, lead=64):
    """sequences whose `table` ("ll" / "of" / "ml") codes are exactly `codes`, in that order; the other two tables get a mild mix. The first sequence carries a
    literal run that makes room for the offsets unless the literal-length table is the one aimed at."""
    seqs, pos = [], 0
    n = len(codes)
    for i, c in enumerate(codes):
        ll = int(rng.integers(1, 5)); ml = int(rng.integers(3, 7)); off = None
        if table == "ll":
            ll = LL_BASE[c] + (int(rng.integers(0, LL_BASE[c + 1] - LL_BASE[c])) if c < 35 and c >= 16 else 0)
        elif table == "ml":
            ml = ML_BASE[c] + (int(rng.integers(0, ML_BASE[c + 1] - ML_BASE[c])) if c < 52 and c >= 32 else 0)
        else:
            lo = max((1 << c) - 3, 1); hi = (2 << c) - 4                          # offBase = offset + 3 has its highest bit at c
            off = cycle_offsets(lo, i) if hi - lo >= 7 else lo + i % (hi - lo + 1)
        if i == 0 and table != "ll": ll = lead
        if pos + ll == 0: ll = 1                                                 # (a first sequence without literals has nothing to copy from)
        # (the other tables' offsets: odd values of three ranges taken in turn, so that none meets the repeat-offset history and both forms of the list are one list)
        if off is None: off = cycle_offsets(5 + 8 * int(rng.integers(0, 3)), i)
        if off > pos + ll:                                                       # not enough history yet for this offset code: a longer literal run makes it
            if table == "ll": off = pos + ll                                     # (the literal-length table's lists keep their lengths: the farthest offset there is)
            else: ll = off - pos
        seqs.append((ll, ml, off)); pos += ll + ml
    return seqs


def _skewed(rng, n, alphabet, top):
    """n codes from `alphabet`, mildly skewed: `top` is the likeliest, the rest fall off"""
    w = np.array([1.0 / (1 + abs(a - top)) for a in alphabet]); w /= w.sum()
    return [int(x) for x in rng.choice(np.array(alphabet), n, p=w)]


TABLES = (("ll", list(range(0, 24)), 3, 6), ("of", list(range(2, 12)), 5, 5), ("ml", list(range(0, 40)), 2, 6))      # table, alphabet used, likeliest code, default norm log
STRATEGY_CONFIGS = (Config(level=1), Config(level=3), Config(level=5))      # fast, double-fast and -- for sources of 16 385 bytes and more, where the call takes it -- greedy


def table_modes(seed=102):
    """the choice between predefined, RLE, described (and, with a dictionary, repeated) tables, for each of the three tables: all codes equal at 1, 2, 3 and 50
    sequences (predefined up to 2, RLE above); every count 20..80 with a mildly skewed distribution under each strategy (libzstd's predefined / described switch
    sits at ((1 << defaultNormLog) * (10 - strategy)) >> 3 sequences: 36 / 32 / 28 for offsets and 72 / 64 / 56 for lengths under fast / double-fast / greedy); a dominant code whose share
    crosses count >> (defaultNormLog - 1); 999, 1 000 and 1 001 sequences.
    A deliberate thinning: fast and double-fast run at EVERY count 20 .. 80; greedy runs only at its own two marks and their neighbours (27, 28, 29 and 55, 56, 57). The
    call takes greedy from 16 385 bytes of source on, so each greedy case drags a 17 000-byte literal run along, and sixty-one of them per table would add a third to the
    emulator file's time for counts at which greedy's choice is the one double-fast already shows (the rule differs only in where the mark sits)."""
    rng = np.random.default_rng(seed)
    F, cases = "table modes", []
    for table, alphabet, top, norm_log in TABLES:
        for n in (1, 2, 3, 50):
            cases.append(mk(F, "%s: all %d codes equal" % (table, n), _hist_seqs(rng, table, [top + 14 if table == "ll" else top] * n), rng, tail=2))
        for n in range(20, 81):
            for cfg in STRATEGY_CONFIGS[:2]:
                cases.append(mk(F, "%s: %d sequences, mildly skewed, %r" % (table, n, cfg), _hist_seqs(rng, table, _skewed(rng, n, alphabet, top)), rng, tail=1, cfg=cfg))
        # greedy needs a source of 16 385 bytes or more: the same lists behind a long literal run
        for n in (27, 28, 29, 55, 56, 57):
            seqs = _hist_seqs(rng, table, _skewed(rng, n, alphabet, top), lead=17000 if table != "ll" else 64)
            tail = 1 if table != "ll" else 17000
            cases.append(mk(F, "%s: %d sequences, mildly skewed, greedy" % (table, n), seqs, rng, tail=tail, cfg=STRATEGY_CONFIGS[2]))
        # mostFrequent against count >> (normLog - 1): at 200 sequences the mark is 200 >> (normLog - 1) of them
        n = 200
        mark = n >> (norm_log - 1)
        for most in sorted({max(mark - 2, 1), mark - 1, mark, mark + 1, mark + 3, 2 * mark}):
            others = [a for a in alphabet if a != top]
            codes = [top] * most + [others[i % len(others)] for i in range(n - most)]
            if max(codes.count(a) for a in others) >= most: continue              # the aimed-at code must be the most frequent one
            rng.shuffle(codes)
            cases.append(mk(F, "%s: the most frequent code %d times in %d (the mark is %d)" % (table, most, n, mark), _hist_seqs(rng, table, codes), rng, tail=1))
        for n in (999, 1000, 1001):
            cases.append(mk(F, "%s: %d sequences" % (table, n), _hist_seqs(rng, table, _skewed(rng, n, alphabet, top)), rng, tail=1))
    return cases


def normalisation(seed=103):
    """FSE normalisation: one code at a share swept from 0.5 to 0.999 beside k codes seen once or twice, k from 1 to the alphabet's size; and histograms that use
    the highest code of each alphabet (offset code 17 at a 128 KiB window, literal-length code 35, match-length code 52). Which path of the normalisation
    ran cannot be read from a frame: this family sweeps.
    A deliberate thinning: k takes 1, 2, 3, 5, 9, half the alphabet and the whole alphabet (fewer at the two highest shares, where a list of k / (1 - share) sequences
    outgrows the block), each with the rare codes seen once and seen twice, not every k from 1 to the alphabet's size: nothing in a frame tells which k reached another
    path, so more values of k buy time under the emulator and no assertion. tests/stress_emu_entropy_sequences.py reseeds the sweep."""
    rng = np.random.default_rng(seed)
    F, cases = "normalisation", []
    full = {"ll": list(range(0, 31)), "of": list(range(2, 15)), "ml": list(range(0, 44))}          # alphabets whose codes stay affordable in bytes
    for table, _, _, _ in TABLES:
        alpha = full[table]
        top = alpha[2]
        others = [a for a in alpha if a != top]
        for share in (0.5, 0.7, 0.9, 0.97, 0.99, 0.999):
            ks = (1, 2, 3, 5, 9, len(others) // 2, len(others)) if share < 0.99 else (1, 2, 5) if share > 0.99 else (1, 3, len(others))
            for k in ks:
                for twice in (0, 1):
                    rare = others[:k]
                    nr = len(rare) * (1 + twice)
                    n = max(int(round(nr / (1 - share))), nr + 2)
                    if n > 9000: continue
                    codes = [top] * (n - nr) + list(rare) * (1 + twice)
                    rng.shuffle(codes)
                    if table == "of": codes.sort(key=lambda c: c > 8)              # the far offsets last: the history they need exists by then
                    seqs = _hist_seqs(rng, table, codes)
                    if sum(q[0] + q[1] for q in seqs) >= BLOCK_MAX: continue
                    cases.append(mk(F, "%s: share %.3f, %d other codes seen %s" % (table, share, k, "twice" if twice else "once"), seqs, rng, tail=1))
    # the top codes. Offset code 17 needs an offset of 2^17 - 3 = 131 069: three bytes before the block's end
    cases.append(mk(F, "of: offset code 17 (offset 131 069)", [(131069, 3, 131069)], rng, route=0))
    cases.append(mk(F, "of: offset codes 0..16 and 17", [(70000, 4, 65536 - 3), (3, 5, 1), (2, 4, 1), (61051, 3, 131069)], rng, route=1))
    cases.append(mk(F, "ll: the top code 35 (65 536 literals) among small ones", [(65536, 4, 9)] + plain_seqs(rng, 40, lead=3), rng, kind="uniform"))
    cases.append(mk(F, "ml: the top code 52 (65 539) among small ones", [(8, 65539, 3)] + plain_seqs(rng, 40, lead=3), rng))
    return cases


def lengths(seed=104):
    """each side of every code boundary of the literal-length and match-length tables, the 65 535 / 65 536 and 65 538 / 65 539 steps of the one-long-length flag
    (in the first, a middle and the last sequence), and the longest match of a block"""
    rng = np.random.default_rng(seed)
    F, cases = "lengths", []
    seqs = [(64, 3, 7)]
    for b in LL_BASE[16:32]: seqs += [(b - 1, 4, 11), (b, 3, 13), (b + 1, 5, 17)]
    cases.append(mk(F, "literal lengths around every code boundary 16 .. 4 096", seqs, rng))
    seqs = [(64, 3, 7)]
    for b in ML_BASE[32:48]: seqs += [(2, b - 1, 11), (1, b, 13), (3, b + 1, 1)]
    cases.append(mk(F, "match lengths around every code boundary 35 .. 2 051", seqs, rng))
    for b in (8192, 16384, 32768):
        for v in (b - 1, b):
            cases.append(mk(F, "literal length %d" % v, [(40, 5, 9), (v, 4, 100), (3, 3, 2)], rng, kind="two", tail=1))
    for b in (4099, 8195, 16387, 32771):
        for v in (b - 1, b):
            cases.append(mk(F, "match length %d" % v, [(40, 5, 9), (2, v, 31), (3, 3, 2)], rng, tail=1))
    for v in (65535, 65536):
        for where, seqs in (("first", [(v, 4, 9), (2, 5, 3), (3, 3, 20)]), ("middle", [(9, 4, 3), (v, 5, 3), (3, 3, 20)]), ("last", [(9, 4, 3), (3, 3, 5), (v, 5, 20)])):
            cases.append(mk(F, "literal length %d in the %s sequence" % (v, where), seqs, rng, kind="two", tail=2))
    for v in (65538, 65539):
        for where, seqs in (("first", [(9, v, 4), (2, 5, 3), (3, 3, 20)]), ("middle", [(9, 4, 3), (1, v, 3), (3, 3, 20)]), ("last", [(9, 4, 3), (3, 3, 5), (2, v, 7)])):
            cases.append(mk(F, "match length %d in the %s sequence" % (v, where), seqs, rng, tail=2))
    cases.append(mk(F, "a match of 131 071 bytes after one literal", [(1, BLOCK_MAX - 1, 1)], rng, route=0))
    return cases


LIT_TOTALS = (0, 1, 5, 6, 7, 62, 63, 64, 255, 256, 257, 1023, 1024, 16383, 16384)


def _spread(rng, total, n_seqs=3):
    """`total` literals over n_seqs sequences and a last run (the first run is 1 at least: a match needs history)"""
    if total == 0: return [], 0
    cut = sorted(int(x) for x in rng.integers(1, total + 1, n_seqs))
    runs = [cut[0]] + [cut[i] - cut[i - 1] for i in range(1, n_seqs)]
    return [(r, 4 + i, 1 + (i % 2)) for i, r in enumerate(runs)], total - cut[-1]


def literals(seed=105, cfg=DEFAULT, family="literals"):
    """the literals section: its size at every edge of the raw / compress rule (63 / 64 without a valid dictionary table, 5 / 6 / 7 with one), of the one- or
    four-stream switch (256) and of the header formats (32, 1 024, 4 096, 16 384; the full block), for each kind of content -- one value (RLE), two values,
    uniform (raw), skewed, Fibonacci-like counts (depth limiting), alphabets of 2, 127, 128, 129 and 256 symbols (weights direct or through FSE) --; and the
    wave-wide gather: runs of 0, 1, 63, 64, 65 and 4 096 literals, consecutive sequences without literals, all literals in the last run"""
    rng = np.random.default_rng(seed)
    F, cases = family, []
    for total in LIT_TOTALS + (31, 32, 4095, 4096):
        for kind in ("rle", "two", "uniform", "skew"):
            seqs, tail = _spread(rng, total)
            if total == 0: seqs, tail = [], 0
            if not seqs and total == 0:
                # no literal at all needs a dictionary to copy from; without one the smallest is one literal: covered by total 1
                continue
            cases.append(mk(F, "%d literals, %s" % (total, kind), seqs, rng, kind=kind, tail=tail, cfg=cfg))
    for kind in ("rle", "skew"):
        cases.append(mk(F, "a full block of literals, %s, no sequences" % kind, [], rng, kind=kind, tail=BLOCK_MAX, cfg=cfg, route=0 if kind == "rle" else 1))
    cases.append(mk(F, "131 068 literals and one match", [(131068, 4, 1)], rng, kind="geom", cfg=cfg, route=0))
    for k in (2, 127, 128, 129, 256):
        for total in (300, 5000):
            seqs, tail = _spread(rng, total)
            cases.append(mk(F, "%d literals over an alphabet of %d" % (total, k), seqs, rng, kind=("alphabet", k), tail=tail, cfg=cfg))
    for k in (12, 16, 20, 23):
        n = len(lit_bytes(rng, 0, ("fib", k)))
        seqs, tail = _spread(rng, n)
        cases.append(mk(F, "Fibonacci-like counts over %d symbols (%d literals)" % (k, n), seqs, rng, kind=("fib", k), tail=tail, cfg=cfg))
    seqs, tail = _spread(rng, 20000)
    cases.append(mk(F, "20 000 literals, geometric over 256 values", seqs, rng, kind="geom", tail=tail, cfg=cfg))
    for kind in ("skew", "uniform"):
        runs = [1, 0, 63, 64, 65, 0, 0, 4096, 1, 64, 0, 63, 65, 17, 16, 15, 0]
        cases.append(mk(F, "literal runs of 0, 1, 63, 64, 65 and 4 096, %s" % kind, [(r, 3 + i % 5, 1 + i % 3) for i, r in enumerate(runs)], rng, kind=kind, tail=64, cfg=cfg))
    cases.append(mk(F, "seventy sequences in a row without literals", [(5, 4, 2)] + [(0, 3 + i % 4, 1 + i % 5) for i in range(70)] + [(2, 3, 1)], rng, tail=3, cfg=cfg))
    cases.append(mk(F, "all literals in the last run", [(1, 4, 1)] + [(0, 3 + i % 4, 1 + (i % 2)) for i in range(9)], rng, tail=3000, cfg=cfg))
    return cases


def block_verdicts(seed=106):
    """compressed or raw: lists whose coded block comes out around the source's size less libzstd's minimum gain ((size >> 6) + 2) -- incompressible literals
    and one match whose length sweeps across the gain --; a source of one repeated byte described by one sequence (never an RLE block: it is the frame's first);
    sources of 6, 7 and 8 bytes (below 7 nothing is compressed)"""
    rng = np.random.default_rng(seed)
    F, cases = "block verdicts", []
    for n in (50, 200, 1000):
        for m in range(3, 3 + 12 + (n >> 6) * 2):
            cases.append(mk(F, "%d incompressible literals and a match of %d" % (n, m), [(n, m, 1 + m % 3)], rng, kind="uniform"))
    for n in (8, 100, 4096, BLOCK_MAX):
        cases.append(mk(F, "%d times one byte, one sequence" % n, [(1, n - 1, 1)], rng, route=None if n < BLOCK_MAX else 1))
    for n in (6, 7, 8):
        cases.append(mk(F, "%d bytes, one sequence" % n, [(1, n - 1, 1)], rng))
        cases.append(mk(F, "%d bytes, literals only" % n, [], rng, tail=n))
    cases.append(mk(F, "an empty source", [], rng, tail=0))
    return cases


def frame_forms(seed=107):
    """the frame around the block: content size on and off, checksum on and off (the trailer kernel), magicless, negative levels (literals stay raw), explicit
    window logs 10 and 17, other strategies' rows"""
    rng = np.random.default_rng(seed)
    F, cases = "frame forms", []
    cfgs = [Config(content_size=False), Config(checksum=True), Config(content_size=False, checksum=True), Config(magicless=True), Config(magicless=True, checksum=True),
            Config(level=-5), Config(level=-1), Config(level=1), Config(level=2), Config(window_log=10), Config(window_log=17),
            Config(level=1, window_log=17, hash_log=12), Config(min_match=3), Config(level=1, min_match=7, target_length=4)]
    for cfg in cfgs:
        small = cfg.params.get("window_log") == 10
        # (an explicit window of 1 KiB: sources up to 1 KiB -- beyond it the window would slide inside the block, which libzstd's blocks and these kernels do not do)
        for n, kind in ((0, "skew"), (5, "skew"), (40, "skew")) + (() if small else ((300, "two"), (3000, "skew"), (20000, "skew"))):
            seqs = plain_seqs(rng, n, lead=20) if n <= 300 else plain_seqs(rng, n // 10, ll=(1, 12), ml=(3, 12))
            cases.append(mk(F, "%d sequences, %s literals, %r" % (len(seqs), kind, cfg), seqs, rng, kind=kind, tail=4 if n else 230, cfg=cfg))
        cases.append(mk(F, "an empty source, %r" % cfg, [], rng, tail=0, cfg=cfg))
        cases.append(mk(F, "three bytes, %r" % cfg, [], rng, tail=3, cfg=cfg))
    return cases


def dictionary(dict_name, content_size, reps, seed=108, raw=False):
    """with a dictionary: lists close to the dictionary's own statistics (repeat mode is a candidate for each table and for the Huffman table) and lists far from
    them, 999 / 1 000 sequences (the repeat rule reads the count), offsets that reach into the dictionary, first sequences that use the repeat offsets the
    dictionary leaves, and the literal thresholds again (a valid dictionary table moves the raw / compress edge to 6)"""
    rng = np.random.default_rng(seed)
    F = "dictionary (%s)" % dict_name
    cfg = Config(dict_name=dict_name)
    cases = []
    D = content_size
    for n in (1, 2, 3, 10, 40, 200, 999, 1000, 1001):
        # JSON-like: short literal runs of text, matches of 4..20, offsets into the dictionary's tail
        seqs, pos = [], 0
        for i in range(n):
            ll = int(rng.integers(0, 6)); ml = int(rng.integers(4, 21)); pos += ll
            off = int(rng.integers(pos + 1, pos + min(D, 4000) + 1)) if i % 3 else int(rng.integers(1, pos + D + 1))
            seqs.append((ll, ml, off)); pos += ml
            if pos > 15000: break
        cases.append(mk(F, "%d text-like sequences into the dictionary" % len(seqs), seqs, rng, kind="text", tail=3, cfg=cfg))
    for n in (3, 40, 999, 1000):
        seqs = plain_seqs(rng, min(n, 1000), ll=(0, 3), ml=(3, 5), lead=2)
        cases.append(mk(F, "%d sequences unlike the dictionary's statistics" % len(seqs), seqs, rng, kind="uniform", tail=1, cfg=cfg))
    r0, r1, r2 = reps
    for name, first in (("entry one", [(2, 5, r0)]), ("entry two", [(2, 5, r1)]), ("entry three", [(3, 4, r2)]), ("entry two without literals", [(0, 5, r1)]),
                        ("entry three without literals", [(0, 5, r2)])) + ((("entry one minus one without literals", [(0, 6, r0 - 1)]),) if r0 > 1 else ()):
        cases.append(mk(F, "the first sequence uses the dictionary's repeat offset: " + name, first + plain_seqs(rng, 12, lead=3), rng, kind="text", tail=2, cfg=cfg))
    cases.append(mk(F, "an offset to the dictionary's first byte", [(0, 8, D), (3, 5, D + 3 + 8)], rng, kind="text", tail=2, cfg=cfg))
    cases.append(mk(F, "no literals at all: the whole source copied from the dictionary", [(0, 40, 200), (0, 30, 1000)], rng, cfg=cfg))
    for total in (1, 5, 6, 7, 62, 63, 64, 255, 256, 257, 1023, 1024):
        for kind in ("text", "rle", "uniform"):
            seqs, tail = _spread(rng, total)
            cases.append(mk(F, "%d literals, %s" % (total, kind), seqs, rng, kind=kind, tail=tail, cfg=cfg))
    # stretches of the dictionary's own text: the dictionary's Huffman table is the cheaper one (treeless sections, in one stream up to 1 023 literals, in four from 1 024)
    for total in (100, 300, 1023, 1024, 3000):
        seqs, tail = _spread(rng, total)
        cases.append(mk(F, "%d literals, a stretch of the dictionary's text" % total, seqs, rng, kind="slice", tail=tail, cfg=cfg))
    for ck in (cfg.with_checksum(), Config(dict_name=dict_name, level=1), Config(dict_name=dict_name, level=-3)):
        cases.append(mk(F, "40 text-like sequences, %r" % ck, [(int(rng.integers(0, 6)), int(rng.integers(4, 21)), int(rng.integers(1, D))) for _ in range(40)], rng, kind="text", tail=3, cfg=ck))
    return cases


def refused_lists(seed=109):
    """lists the loader must refuse with externalSequences_invalid (and a source above one block: 40), each beside good neighbours in the tests' batches"""
    rng = np.random.default_rng(seed)
    F = "refused lists"
    src = lit_bytes(rng, 500, "skew")
    cases = [Case(F, "a match length of 2", [(5, 4, 4), (3, 2, 4), (2, 5, 4)], src, refused=INVALID),
             Case(F, "a match length of 0", [(5, 0, 4)], src, refused=INVALID),
             Case(F, "lengths that sum to one more than the source", [(200, 200, 4), (50, 51, 5)], src, refused=INVALID, ref_refuses=True),
             Case(F, "lengths that sum to the source exactly (a good neighbour)", [(200, 200, 1), (50, 50, 2)], src),
             Case(F, "a literal length alone above the source", [(501, 3, 4)], src[:300], refused=INVALID, ref_refuses=True),
             Case(F, "an offset value of 0", [(5, 4, 0)], src, refused=INVALID),
             Case(F, "a good list on a source of 131 073 bytes", [(5, 4, 4)], lit_bytes(rng, BLOCK_MAX + 1, "two"), refused=UNSUPPORTED, route=0)]
    return cases


PLAIN = {"sequence counts": sequence_counts, "table modes": table_modes, "normalisation": normalisation, "lengths": lengths, "literals": literals,
         "block verdicts": block_verdicts, "frame forms": frame_forms, "refused lists": refused_lists}


def plain_families():
    return [c for f in PLAIN.values() for c in f()]


# the dictionaries: tests/golden/dict_json4k.bin as it is (trained: entropy tables, the format's default repeat offsets), the same with other repeat offsets
# written into its header, and a stretch of its content as a raw-content dictionary. Where the trained dictionary's content starts is pinned against the
# device parser by tests/test_emu_entropy_sequences.py
JSON4K_CONTENT_OFF = 122
OTHER_REPS = (7, 30, 100)


def load_dicts(root):
    import os
    d = open(os.path.join(root, "tests", "golden", "dict_json4k.bin"), "rb").read()
    off = JSON4K_CONTENT_OFF
    other = d[:off - 12] + struct.pack("<III", *OTHER_REPS) + d[off:]
    return {"json4k": (d, off, (1, 4, 8), False), "json4k, other repeat offsets": (other, off, OTHER_REPS, False), "raw content": (d[off + 5000:off + 9000], 0, (1, 4, 8), True)}


def dictionary_families(dicts):
    set_text_source(dicts["json4k"][0][JSON4K_CONTENT_OFF:])
    return [c for k, (name, (d, off, reps, raw)) in enumerate(dicts.items()) for c in dictionary(name, len(d) - off, reps, seed=108 + k, raw=raw)]


# ------------------------------------------------------------------------------------------------------------------ what a frame says about its block
def frame_census(frame, magicless=False):
    """header facts of a ONE-block frame (libzstd's, never ours): {"block": "raw" | "rle" | "compressed", and for a compressed block "lit_type" (0 raw, 1 RLE,
    2 compressed, 3 treeless), "lit_format" (the size format bits; raw and RLE: 0, 1 or 3), "streams", "count_width" (bytes of the sequence count), "modes"
    (literal lengths, offsets, match lengths: 0 predefined, 1 RLE, 2 described, 3 repeat) -- None without sequences}"""
    p = 0 if magicless else 4
    fhd = frame[p]; p += 1
    single, fcs, did = (fhd >> 5) & 1, fhd >> 6, fhd & 3
    if not single: p += 1
    p += (0, 1, 2, 4)[did]
    p += (1 if single else 0, 2, 4, 8)[fcs]
    bh = frame[p] | frame[p + 1] << 8 | frame[p + 2] << 16; p += 3
    assert bh & 1, "one block per frame"
    btype, bsize = (bh >> 1) & 3, bh >> 3
    if btype != 2: return {"block": ("raw", "rle")[btype]}
    end = p + bsize
    b0 = frame[p]
    lt, sf = b0 & 3, (b0 >> 2) & 3
    out = {"block": "compressed", "lit_type": lt}
    if lt < 2:
        hs = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        regen = int.from_bytes(frame[p:p + hs], "little") >> (3 if hs == 1 else 4)
        out["lit_format"] = 0 if hs == 1 else sf
        p += hs + (regen if lt == 0 else 1)
    else:
        hs, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
        v = int.from_bytes(frame[p:p + hs], "little")
        out["lit_format"] = sf; out["streams"] = 1 if sf == 0 else 4
        p += hs + ((v >> (4 + bits)) & ((1 << bits) - 1))
    out["lit_size_format"] = out["lit_format"]
    n0 = frame[p]
    if n0 == 0: out["count_width"], out["modes"], out["nb_seq"] = 1, None, 0; return out
    if n0 < 128: out["count_width"], out["nb_seq"] = 1, n0; p += 1
    elif n0 < 255: out["count_width"], out["nb_seq"] = 2, ((n0 - 128) << 8) + frame[p + 1]; p += 2
    else: out["count_width"], out["nb_seq"] = 3, frame[p + 1] + (frame[p + 2] << 8) + 0x7F00; p += 3
    m = frame[p]
    out["modes"] = (m >> 6, (m >> 4) & 3, (m >> 2) & 3)
    assert p < end
    return out


def write_fixture(path, items):
    """the stand-alone emulator program's input (tests/emu/emu_entropy_sequences.cpp): items = [(level, flags, source, packed sequences, status, libzstd's frame)]"""
    with open(path, "wb") as f:
        f.write(b"ZESQ" + struct.pack("<I", len(items)))
        for level, flags, src, packed, status, frame in items:
            f.write(struct.pack("<iIIIiI", level, flags, len(src), len(packed), status, len(frame)))
            f.write(src); f.write(np.asarray(packed, dtype="<u8").tobytes()); f.write(frame)
