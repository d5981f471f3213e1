"""Seeded families of frames whose Huffman tables, descriptions and streams are EXPLICIT choices (test infrastructure for
tests/test_emu_huffman_tables.py and tests/test_gpu_huffman_tables.py).

The suite's other frames carry the tables libzstd's encoder happens to emit (never deeper than 11 bits) or the natural tree craft.HufTable derives
from the literals. Here a table is a weight list (craft.HufTable.from_weights), its description a chosen form (direct, or FSE-compressed on a chosen
distribution), its section a chosen layout -- and every family sits on both sides of its limit. A case comes twice: as a block without sequences,
and as a twin with two or three sequences whose literal runs straddle the seams between the four streams. Case.build() writes the frame and asks
tests/hufmodel.py what it decodes to (or why it is refused); which decoder decisions a family reaches is asserted with hufmodel.census
(REQUIRED below) by the tests, never assumed here."""
import numpy as np

from tests import craft, hufmodel, seqmodel
from tests.seqfamilies import Case

T = craft.HufTable.from_weights


def staircase(log):
    """weights log, log - 1, ... 2, 1, 1: table log `log`, one code of every length"""
    return list(range(log, 0, -1)) + [1]


def longest_codes(log, ones=64):
    """`ones` symbols of weight 1 (the longest codes) first, then one symbol of each weight that completes the table to `log`"""
    w = [1] * ones
    k = ones.bit_length()                      # ones = 2^(k-1): the next weight that doubles the sum
    assert ones == 1 << (k - 1)
    return w + list(range(k, log + 1))


class HufCase(Case):
    """a Case whose expected value comes from hufmodel: the literals the model decodes, run through seqmodel.execute with the block's sequences.
    damaged: the case belongs to the damaged-stream family, the one place where the model may refuse ("a stream not consumed exactly") what libzstd
    decodes. align = (stream index, offset mod 16) the harness should place that stream at; aims = census events the case is there for."""
    damaged, align, aims = False, None, ()

    def model_dict(self):
        return self.dict_data if self.dict_data and not self.raw_dict else None

    def build(self, xxh64=None):
        Case.build(self, xxh64)
        infos = []
        try:
            it = iter(hufmodel.literals(self.frame, self.model_dict(), infos))
            blocks = [(("seq", next(it)) + tuple(b[2:])) if b[0] == "seq" else b for b in self.blocks]
            content = seqmodel.execute(blocks, self.dict_content(), self.start_reps)
            if self.want is not None and content != self.content:
                if len(content) == len(self.content): self.want = self.content = content
                else: self.want, self.why = None, "content size differs from the header's"
        except hufmodel.Refused as e:
            self.want, self.why = None, e.reason
        except seqmodel.Invalid as e:
            self.want, self.why = None, e.reason
        self.deep_blocks = sum(i.get("log", 0) > hufmodel.DEEP for i in infos)                       # Huffman sections K1 decodes in place: the table is above K1b's slots
        self.stream_at = [i["at"] + off for i in infos for off, _, _ in i.get("streams", ())]      # where the frame's Huffman streams start
        return self

    def pad_for(self, arena_pos):
        """filler bytes in front of this frame, to lie at `arena_pos` of an aligned arena, that put the aimed stream at the aimed offset mod 16"""
        if not self.align or self.align[0] >= len(self.stream_at): return 0
        return (self.align[1] - arena_pos - self.stream_at[self.align[0]]) % 16

    def with_lead(self):
        c = HufCase(self.family, self.name + " [after a raw block]", [("raw", b"L")] + list(self.blocks), self.dict_data, self.raw_dict,
                    self.fcs, self.checksum, self.start_reps, dict(self.header), None, self.short_by)
        if "claims" in c.header: c.header["claims"] += 1
        if self.dict_data and not self.raw_dict: c.content_off = self.content_off
        c.damaged, c.align, c.aims = self.damaged, self.align, self.aims
        return c

    def huf_census(self, base=0):
        return hufmodel.census(self.frame, self.model_dict(), base)


def draw(rng, table, n, weights=None):
    """n literals among the symbols of `table` (only those of the given weights, if any)"""
    syms = [s for s, w in enumerate(table.weights) if w and (weights is None or w in weights)]
    return bytes(np.asarray(syms, dtype=np.uint8)[rng.integers(0, len(syms), n)])


def twin_sequences(n):
    """two or three sequences over n literals whose literal runs straddle the seams of the four streams (at q, 2q, 3q; q = (n + 3) / 4)"""
    q = (n + 3) // 4
    lls = [min(q + 1, n)]
    while len(lls) < 3 and sum(lls) + q <= n and q: lls.append(q)
    if len(lls) == 1 and n >= 2: lls = [1, n - 1]
    return [(ll, 3 + i, 4) for i, ll in enumerate(lls) if ll]


def pair(family, name, lits, opts, claims=None, **kw):
    """the case as a block without sequences, and its twin with sequences"""
    out = []
    for seqs, tag in (([], ""), (twin_sequences(len(lits)), " + sequences")):
        if tag and not seqs: continue
        header = {"window_log": 17}
        if claims is not None: header["claims"] = claims + sum(q[1] for q in seqs)
        c = HufCase(family, name + tag, [("seq", lits, seqs, dict(opts))], header=header)
        for k, v in kw.items(): setattr(c, k, v)
        out.append(c)
    return out


def _modes(n):
    return ["huf1"] + (["huf4"] if n >= 6 else [])


# ------------------------------------------------------------------------------------------------ depth
def depth(seed=1):
    rng = np.random.default_rng(seed)
    cases = []
    tables = [("staircase of log %d" % L, staircase(L)) for L in range(1, 13)]
    tables += [("a flat table of log 7", [1] * 128), ("log 11, 64 longest codes", longest_codes(11)), ("log 12, 64 longest codes", longest_codes(12))]
    for name, w in tables:
        t = T(w)
        for mode in ("huf1", "huf4"):
            lits = draw(rng, t, 41)
            cases += pair("depth", "%s, %s" % (name, mode), lits, {"lit": mode, "huf_table": t})
    for L in (11, 12):                                                          # nothing but longest codes: the most bits a stream can ask of the reader
        t = T(longest_codes(L))
        cases += pair("depth", "log %d, all literals on longest codes, four streams" % L, draw(rng, t, 600, (1,)), {"lit": "huf4", "huf_table": t})
    return cases


# ------------------------------------------------------------------------------------------------ alphabet
def last_weight_tables(L):
    """tables of log L whose implied last weight is k, for every k = 1 .. L"""
    out = []
    for k in range(1, L + 1):
        w = list(range(L, k, -1)) + (staircase(k - 1) if k >= 2 else [1]) + [k]
        out.append((k, w))
    return out


def alphabet(seed=2):
    rng = np.random.default_rng(seed)
    cases = []

    def add(name, w, form="direct", n=37, **fse):
        t = T(w)
        desc = t.description(form, **fse) if form == "fse" else t.description()
        for mode in _modes(n):
            cases.extend(pair("alphabet", "%s, %s" % (name, mode), draw(rng, t, n), {"lit": mode, "huf_table": t, "huf_desc": desc}))
    add("two symbols", [1, 1])
    add("two written weights", [2, 1, 1])
    add("weights 1 and 2 only", [2, 2, 2, 1, 1])
    add("weights 3 and up beside the ones", [4, 4, 3, 3, 3, 1, 1, 1, 1])
    add("zero-weight gaps", [2, 0, 0, 1, 0, 0, 0, 1])
    add("127 written weights", [1] * 128)
    add("128 written weights", [1] * 126 + [2, 0, 8])
    add("256 symbols of weight 1", [1] * 256, "fse", accuracy_log=5)
    add("255 symbols", [1] * 254 + [2], "fse", accuracy_log=6)
    add("254 symbols", [1] * 252 + [2, 2], "fse", accuracy_log=5)
    sparse = [0] * 256
    for s, w in ((3, 4), (64, 3), (70, 1), (127, 2), (128, 1), (191, 1), (192, 3), (200, 1), (254, 2)): sparse[s] = w
    for s, w in ((20, 2), (30, 3), (255, 2)): sparse[s] = w                    # 32 = 2^5 with the implied weight of symbol 255
    assert sum(1 << (w - 1) for w in sparse if w) == 32
    add("symbols in all four quarters with gaps, symbol 255", sparse, "fse", accuracy_log=6)
    for L in (6,):
        for k, w in last_weight_tables(L): add("log %d, implied last weight %d" % (L, k), w)
    add("log 11, implied last weight 11", staircase(10) + [11])
    add("log 12, implied last weight 12", staircase(11) + [12])
    # one weight too many for the FSE form: 256 written weights, the decoder gives up at the 255th
    t = T([1] * 256, valid=False)
    rep = {}
    desc = t.description("fse", 5, report=rep)
    assert rep["exit"] == 3
    # (the literals are coded on the table of 256 symbols of weight 1: what a decoder that took all 256 written weights would build from its first 256)
    flat = T([1] * 256)
    cases += pair("alphabet", "the FSE list one weight too long", draw(rng, flat, 21), {"lit": "huf1", "huf_table": flat, "huf_desc": desc}, claims=21)
    return cases


# ------------------------------------------------------------------------------------------------ FSE descriptions
def _fill_description(w_front, target):
    """a weight list starting with w_front, then zeros and ones, whose FSE description at accuracy log 6 is exactly `target` bytes: zeros are coded
    on a 'less than one' count (6 bits each), so their number tunes the size"""
    for zeros in range(0, 200):
        for ones in range(2, 60, 2):
            w = list(w_front) + [0] * zeros + [1] * ones
            total = sum(1 << (x - 1) for x in w if x)
            if total & (total - 1) or len(w) > 256: continue
            t = T(w)
            norm = [0] * (max(w) + 1)
            norm[0] = -1
            present = sorted(set(x for x in t.written if x))
            for x in present: norm[x] = 1
            norm[1] += 64 - 1 - len(present)
            if 0 not in t.written: continue
            rep = {}
            try: d = t.description("fse", 6, norm, rep)
            except AssertionError: continue
            if rep["bytes"] == target: return t, d, norm
    raise AssertionError("no list found for %d bytes" % target)


def fse_descriptions(seed=3):
    rng = np.random.default_rng(seed)
    cases = []
    two = T([1, 1])

    def good(name, t, desc, n=29):
        for mode in _modes(n):
            cases.extend(pair("FSE descriptions", "%s, %s" % (name, mode), draw(rng, t, n), {"lit": mode, "huf_table": t, "huf_desc": desc}))

    def bad(name, desc, t=two, **kw):
        """(the literals are coded on `t`: where a decoder takes the description after all, on the table it would build, so that the frame then decodes)"""
        cases.extend(pair("FSE descriptions", name, draw(rng, t, 5), {"lit": "huf1", "huf_table": t, "huf_desc": desc}, claims=5, **kw))
    for log in (5, 6):
        for w in (staircase(6), staircase(5)):                                  # 6 written weights (even: the first exit), 5 (odd: the second)
            t = T(w)
            rep = {}
            d = t.description("fse", log, report=rep)
            good("accuracy log %d, %d weights, exit %d" % (log, rep["weights"], rep["exit"]), t, d)
    t = T(staircase(7))
    norm = [0, 26, -1, -1, -1, -1, -1, -1]                                      # 'less than one' counts: a full-width state read each
    assert sum(abs(x) for x in norm) == 32
    good("'less than one' counts at accuracy log 5", t, t.description("fse", 5, norm))
    # weight 12 in the distribution: libzstd decodes it at accuracy log 5 and refuses it at 6 (its work area is sized for log 6 and the weights 0 .. 11)
    t12 = T(staircase(12))
    good("log 12, weight 12 in a distribution of accuracy log 5", t12, t12.description("fse", 5))
    bad("weight 12 in a distribution of accuracy log 6", t12.description("fse", 6), t12)
    t11 = T(staircase(11))
    good("log 11, weight 11 in a distribution of accuracy log 6", t11, t11.description("fse", 6))
    # the description's size byte: 0 and 1 cannot hold a distribution, 2 and 3 hold one and no / a one-byte bit stream; 127 is the largest
    d = T(staircase(6)).description("fse", 5)
    bad("size byte 0", b"\x00")
    bad("size byte 1", b"\x01" + d[1:2])
    bad("size byte 2", b"\x02" + d[1:3])
    t, d127, _ = _fill_description([4, 3, 2], 127)
    good("a description of 127 bytes", t, d127)
    t, d126, _ = _fill_description([4, 3, 2], 126)
    good("a description of 126 bytes", t, d126)
    whole = [0, 32]                                                             # every state gives weight 1 and reads no bits: the stream never runs out
    bad("a distribution whose states read no bits", bytes([len(craft.ncount(whole, 5)) + 2]) + craft.ncount(whole, 5) + b"\x00\x04")       # (ten bits: the two states)
    short = [0, 31]
    one = craft.ncount(short, 5) + b"\x01"                                      # weight 1 on 31 cells, one cell left to whatever follows: the end-mark byte alone
    bad("a bit stream shorter than its two states", bytes([len(one)]) + one)
    # refused distributions and streams
    t13 = T([13, 1, 1, 2], valid=False)
    bad("a distribution naming weight 13, and a stream that uses it", t13.description("fse", 5))
    # several weights far above 12, each in a lane of its own: a refusal kept as one large addend per lane must not wrap to a sum that passes (four addends
    # of 2^30 do), nor a table builder shift by w - 1 = 32 and up. The literals are coded on what is left when the large weights vanish: w 1 1 and the implied 2.
    for big in ((33, 36, 40, 44), (33, 34, 35, 36, 40, 41, 43, 44)):
        norm = [0] * 45
        norm[1] = 16
        for w in big: norm[w] = 16 // len(big)
        left = T([0] * len(big) + [1, 1, 2])
        bad("%d weights of 33 .. 44 in lanes of their own" % len(big), T(list(big) + [1, 1], valid=False).description("fse", 5, norm), left)
    bad("accuracy log 7", T(staircase(6)).description("fse", 7), T(staircase(6)))
    # (a distribution whose counts OVERSHOOT 2^log cannot be written: the widest value a count field holds decodes to what is left minus one, so the readers'
    # "more than is left" and "not 2^log at the end" returns are reached only by running out of description or alphabet -- the next case and "size byte 2")
    n = craft.ncount([8, 8, 8], 5)                                              # 24 of 32 and nothing behind it
    bad("a distribution short of 2^log at the description's end", bytes([len(n)]) + n)
    d = T(staircase(6)).description("fse", 6)
    bad("a bit stream without its end mark", d[:-1] + b"\x00")
    bad("a description running past the section", bytes([100]) + d[1:])
    return cases


# ------------------------------------------------------------------------------------------------ refused tables
# (no "odd number of weights of 1" entry: once the rest is a power of two the total 2^log is even and so is the sum over the weights of 2 and up, hence the
# number of ones -- the decoders' parity test is implied by the test before it; test_emu_huffman_tables.py's mutation 1 has the argument)
REFUSED_TABLES = [
    ("weights that do not complete to a power of two", [3, 2, 1, 1, 1]),
    ("no weight of 1", [2, 2]),
    ("a single weight of 2", [2]),
    ("a weight of 13", [13, 1]),
    ("four weights of 13 .. 15, each in a lane of its own", [13, 14, 15, 13, 1, 1]),
    ("all weights zero", [0, 0]),
    ("one written weight, zero", [0]),
    ("a sum that needs log 13", [12, 12, 1]),
    ("a sum of exactly 2^12 before the implied weight", [12, 12]),
]


def refused_tables(seed=4):
    cases = []
    two = T([1, 1])
    for name, w in REFUSED_TABLES:
        d = T(w, valid=False).description()
        for mode, lits in (("huf1", b"\x00\x01\x01\x00\x01"), ("huf4", b"\x00\x01\x01\x00\x01\x01\x00")):
            cases += pair("refused tables", "%s, %s" % (name, mode), lits, {"lit": mode, "huf_table": two, "huf_desc": d}, claims=len(lits))
    # and beside them the nearest lists that ARE tables
    rng = np.random.default_rng(seed)
    for name, w in (("3 2 1 and the implied 1", [3, 2, 1, 1]), ("one written weight of 1, the implied one the second", [2, 1, 1]), ("a weight of 12", [12, 11] + staircase(10))):
        t = T(w)
        cases += pair("refused tables", "valid: " + name, draw(rng, t, 23), {"lit": "huf4", "huf_table": t})
    return cases


# ------------------------------------------------------------------------------------------------ streams
def stream_tables():
    return [("all codes of 11 bits", T(longest_codes(11)), (1,)), ("all codes of 1 bit", T([1, 1]), None), ("a mix of 1 .. 6 bits", T(staircase(6)), None)]


def streams(seed=5):
    rng = np.random.default_rng(seed)
    cases, turn = [], 0

    def one(name, t, lits, mode="huf1", **o):
        nonlocal turn
        for c in pair("streams", name, lits, dict({"lit": mode, "huf_table": t}, **o)):
            c.align = (turn % 4 if mode == "huf4" else 0, (turn * 5 + 3) % 16); turn += 1
            cases.append(c)
    for tname, t, only in stream_tables():
        for n in list(range(1, 18)) + [63, 64, 65]:
            one("%s, %d literals in one stream" % (tname, n), t, draw(rng, t, n, only))
        for n in (6, 7, 8, 9, 1023):
            one("%s, %d literals in four streams" % (tname, n), t, draw(rng, t, n, only), "huf4")
        for sf in (1, 2, 3):
            one("%s, four streams, size format %d" % (tname, sf), t, draw(rng, t, 44, only), "huf4", size_format=sf)
    # stream lengths in bytes: 1 .. 80 and ~200 -- below, at and above K1b's 64-byte ring
    tname, t, _ = stream_tables()[1]
    for b in list(range(1, 81)) + [199, 200, 201]:
        n = 8 * (b - 1) + b % 8
        if n == 0: continue
        if n < 1024: one("1-bit codes, a stream of %d bytes" % b, t, draw(rng, t, n))
        else: one("1-bit codes, four streams of ~%d bytes" % b, t, draw(rng, t, 4 * n - (b % 4)), "huf4")
    tname, t, only = stream_tables()[0]
    for k in [2, 3, 5, 8, 13, 21, 29, 37, 45, 46, 47, 48, 52, 58, 145, 146]:       # 11 k + 1 bits: 46 symbols = 64 bytes (the ring), 47 = 65
        one("11-bit codes, a stream of %d symbols" % k, t, draw(rng, t, k, only))
    for k in (46, 47, 146):
        one("11-bit codes, four streams of %d symbols" % k, t, draw(rng, t, 4 * k, only), "huf4")
    t12 = T(longest_codes(12))
    for k in (44, 150):
        one("12-bit codes, four streams of %d symbols" % k, t12, draw(rng, t12, 4 * k, (1,)), "huf4")
    tname, t, _ = stream_tables()[2]
    for n in (100, 250, 330, 600):
        one("mixed codes, one stream of %d literals" % n, t, draw(rng, t, n))
    return cases


# ------------------------------------------------------------------------------------------------ damaged streams
def _damage(which, how):
    def f(parts):
        p = list(parts)
        if how == "last byte 0": p[which] = p[which][:-1] + b"\x00"
        elif how == "a byte added in front": p[which] = b"\x5a" + p[which]
        elif how == "a byte removed": p[which] = p[which][1:]
        return p
    return f


def damaged_streams(seed=6):
    rng = np.random.default_rng(seed)
    cases = []
    for tname, t, only in stream_tables():
        l1, l4 = draw(rng, t, 40, only), draw(rng, t, 160, only)
        for how in ("last byte 0", "a byte added in front", "a byte removed"):
            cases += pair("damaged streams", "%s, one stream, %s" % (tname, how), l1, {"lit": "huf1", "huf_table": t, "mangle": _damage(0, how)}, claims=40, damaged=True)
            for k in range(4):
                cases += pair("damaged streams", "%s, stream %d of four, %s" % (tname, k + 1, how), l4, {"lit": "huf4", "huf_table": t, "mangle": _damage(k, how)}, claims=160, damaged=True)
        for d in (-1, 1):
            cases += pair("damaged streams", "%s, one stream, count %+d" % (tname, d), l1, {"lit": "huf1", "huf_table": t, "claim": 40 + d}, claims=40 + d, damaged=True)
            cases += pair("damaged streams", "%s, four streams, count %+d" % (tname, d), l4, {"lit": "huf4", "huf_table": t, "claim": 160 + d}, claims=160 + d, damaged=True)
        sizes = [len(t.stream(l4[i * 40:(i + 1) * 40])) for i in range(4)]
        cases += pair("damaged streams", "%s, a jump table one byte past the section" % tname, l4,
                      {"lit": "huf4", "huf_table": t, "jump": [sizes[0], sizes[1], sizes[2] + sizes[3] + 1]}, claims=160, damaged=True)
        cases += pair("damaged streams", "%s, a jump table that leaves the fourth stream no byte" % tname, l4,
                      {"lit": "huf4", "huf_table": t, "jump": [sizes[0], sizes[1], sizes[2] + sizes[3]]}, claims=160, damaged=True)
        cases += pair("damaged streams", "%s, undamaged" % tname, l4, {"lit": "huf4", "huf_table": t}, damaged=True)
    two = T([1, 1])
    cases += pair("damaged streams", "five literals in four streams", b"\x00\x01\x01\x00\x01\x01", {"lit": "huf4", "huf_table": two, "claim": 5}, claims=5, damaged=True)
    return cases


# ------------------------------------------------------------------------------------------------ inheritance (frames of several blocks)
def inheritance(seed=7):
    rng = np.random.default_rng(seed)
    cases = []

    def blk(t, n, mode, seq=False, **o):
        lits = draw(rng, t, n)
        return ("seq", lits, twin_sequences(n) if seq else [], dict({"lit": mode, "huf_table": t}, **o))

    def rawlit(n, seq):
        lits = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        return ("seq", lits, twin_sequences(n) if seq else [], {})
    t6, t12, t5, t11 = T(staircase(6)), T(longest_codes(12)), T(staircase(5)), T(staircase(11))
    for seq in (False, True):
        tag = " + sequences" if seq else ""
        plans = [
            ("a table, treeless in one stream, treeless in four", [blk(t6, 50, "huf4", seq), blk(t6, 33, "treeless1", seq), blk(t6, 90, "treeless4", seq)]),
            ("a table of log 11, treeless twice", [blk(t11, 50, "huf1", seq), blk(t11, 33, "treeless4", seq), blk(t11, 20, "treeless1", seq)]),
            ("a table of log 12, treeless in one stream and in four", [blk(t12, 50, "huf4", seq), blk(t12, 33, "treeless1", seq), blk(t12, 90, "treeless4", seq)]),
            ("log 12, a block of raw literals, treeless", [blk(t12, 50, "huf1", seq), rawlit(20, seq), blk(t12, 40, "treeless4", seq)]),
            ("log 12, a raw block, treeless", [blk(t12, 50, "huf1", seq), ("raw", b"between"), blk(t12, 40, "treeless1", seq)]),
            ("log 12, a table of log 5, treeless", [blk(t12, 50, "huf4", seq), blk(t5, 30, "huf1", seq), blk(t5, 40, "treeless4", seq)]),
            ("log 5, a table of log 12, treeless", [blk(t5, 50, "huf4", seq), blk(t12, 30, "huf1", seq), blk(t12, 40, "treeless4", seq)]),
        ]
        for name, blocks in plans:
            cases.append(HufCase("inheritance", name + tag, blocks, header={"window_log": 17}))
        bad = T([2, 2], valid=False).description()
        cases.append(HufCase("inheritance", "a refused table in the second block" + tag,
                             [blk(t6, 50, "huf1", seq), blk(T([1, 1]), 9, "huf1", seq, huf_desc=bad)], header={"window_log": 17}))
        cases.append(HufCase("inheritance", "treeless with nothing to inherit" + tag, [rawlit(9, seq), blk(t6, 12, "treeless1", seq)], header={"window_log": 17}))
    return cases


# ------------------------------------------------------------------------------------------------ dictionaries
def replaced_dictionary(trained, table, form="direct", **fse):
    """`trained` with its Huffman description replaced by `table`'s; returns (dictionary, offset of its content)"""
    _, end = hufmodel.dictionary_weights(trained)
    d = trained[:8] + (table.description(form, **fse) if form == "fse" else table.description()) + trained[end:]
    return d


def dictionaries(trained, content_off, seed=8):
    """per dictionary: (name, dictionary bytes, cases) -- the trained dictionary of tests/golden with a table of log 11 / log 12 in place of its own;
    frames whose first block is treeless in one and in four streams, a frame that brings its own table, and treeless blocks behind a raw block"""
    rng = np.random.default_rng(seed)
    _, old_end = hufmodel.dictionary_weights(trained)
    out = []
    for name, w in (("log 11", longest_codes(11)), ("log 12", longest_codes(12)), ("log 12, a staircase", staircase(12))):
        t = T(w)
        d = replaced_dictionary(trained, t)
        _, new_end = hufmodel.dictionary_weights(d)
        dict_id = int.from_bytes(d[4:8], "little")
        cases = []
        for mode, n in (("treeless1", 30), ("treeless4", 70), ("treeless4", 6), ("treeless1", 1)):
            for c in pair("dictionaries", "%s, first block %s of %d" % (name, mode, n), draw(rng, t, n), {"lit": mode, "huf_table": t}):
                cases.append(c)
        own = T(staircase(7))
        cases += pair("dictionaries", "%s, the frame's own table" % name, draw(rng, own, 30), {"lit": "huf4", "huf_table": own})
        for seq in (False, True):
            lits = [draw(rng, t, 40), draw(rng, own, 25), draw(rng, own, 31)]
            blocks = [("seq", lits[0], twin_sequences(40) if seq else [], {"lit": "treeless4", "huf_table": t}),
                      ("seq", lits[1], [], {"lit": "huf1", "huf_table": own}), ("seq", lits[2], twin_sequences(31) if seq else [], {"lit": "treeless4", "huf_table": own})]
            cases.append(HufCase("dictionaries", "%s, treeless, a table, treeless%s" % (name, " + sequences" if seq else ""), blocks, header={"window_log": 17}))
        for c in cases:
            c.dict_data, c.raw_dict, c.content_off = d, False, content_off - old_end + new_end
            c.header["dict_id"] = dict_id
        out.append((name, d, cases))
    return out


# ------------------------------------------------------------------------------------------------ K1b groups
def k1b_groups(seed=9):
    """(name, cases in batch order): 1, 11, 12, 13 and 25 Huffman frames among raw-literal ones (K1b takes 12 frames a wave trip), all of one size so
    that they share a bin; a damaged stream in the first and in the twelfth Huffman frame -- every neighbour must still decode"""
    rng = np.random.default_rng(seed)
    tabs = [T(staircase(6)), T(longest_codes(11)), T(staircase(3)), T([1, 1])]
    out = []
    for n in (1, 11, 12, 13, 25):
        for hurt in ((), (0,), (11,), (0, 11)):
            if any(h >= n for h in hurt): continue
            cases = []
            for i in range(n):
                t = tabs[i % 4]
                o = {"lit": "huf4" if i % 3 else "huf1", "huf_table": t}
                if i in hurt: o["mangle"] = _damage(0, "last byte 0" if i == 0 else "a byte added in front")
                c = pair("K1b groups", "%d frames, frame %d%s" % (n, i, " damaged" if i in hurt else ""), draw(rng, t, 200), o, claims=200 if i in hurt else None, damaged=i in hurt)[i % 2]
                cases.append(c)
                if i % 2: cases.append(HufCase("K1b groups", "raw literals beside frame %d" % i, [("seq", bytes(rng.integers(0, 256, 30, dtype=np.uint8)), [(9, 4, 5)], {})], header={"window_log": 17}))
            out.append(("%d Huffman frames, damaged %s" % (n, list(hurt)), cases))
    return out


FAMILIES = {"depth": depth, "alphabet": alphabet, "FSE descriptions": fse_descriptions, "refused tables": refused_tables, "streams": streams,
            "damaged streams": damaged_streams, "inheritance": inheritance}

REFUSALS = {
    "FSE descriptions": {"weights: a distribution above libzstd's work area", "description: an FSE form below two bytes", "weights: more than 255 of them",
                         "weights: one above 12", "weights' bit stream: no end mark", "description: runs past the section", "weights: accuracy log above 6",
                         "distribution: runs past the description"},
    "refused tables": {"weights: the sum does not complete to a power of two", "weights: fewer than two weights of 1", "weights: one above 12", "weights: all zero",
                       "weights: a sum that needs a table log above 12"},
    "damaged streams": {hufmodel.INEXACT, "a stream: no end mark", "a stream: empty", "literals: the jump table runs past the section", "literals: too few for the stream count"},
}

REQUIRED = {
    "depth": ["table log %d" % L for L in range(1, 13)] + ["table above K1b's slots", "a stream of longest codes above the ring", "one stream", "four streams"],
    "alphabet": ["two symbols", "symbols in 64..127", "symbols in 128..191", "symbols in 192..255", "symbol 255", "zero-weight gaps",
                 "cells written one at a time (weights 1 and 2)", "cells written eight bytes at a time (weights 3 and up)",
                 "direct weights: 1", "direct weights: 2", "direct weights: 127", "direct weights: 128", "FSE weights: 255", "FSE weights: 254", "FSE weights: 253",
                 "implied last weight equal to the log", "refused: weights: more than 255 of them"] + ["implied last weight %d of log 6" % k for k in range(1, 7)] +
                ["implied last weight 11 of log 11", "implied last weight 12 of log 12"],
    "FSE descriptions": ["FSE accuracy log 5", "FSE accuracy log 6", "FSE decode ends through exit 1", "FSE decode ends through exit 2", "FSE description of 127 bytes",
                         "FSE description of 126 bytes", "FSE distribution with a 'less than one' count", "FSE description in a frame of one block",
                         "FSE description in a frame of several blocks", "table log 12"] + ["refused: " + r for r in sorted(REFUSALS["FSE descriptions"])],
    "refused tables": ["refused: " + r for r in sorted(REFUSALS["refused tables"])],
    "streams": ["stream start at %d mod 16" % a for a in range(16)] + ["trip tail %d" % k for k in range(8)] + ["stream of %d bytes" % b for b in range(1, 81)] +
               ["stream of 200 and up bytes", "stream below the ring", "stream at the ring", "stream above the ring", "empty fourth stream", "a stream of longest codes above the ring",
                "size format of 10 bits", "size format of 14 bits", "size format of 18 bits"] + ["four streams of %d literals" % n for n in (6, 7, 8, 9, 1023)] +
               ["stream of %d symbols" % n for n in range(0, 8)],
    "damaged streams": ["refused: " + r for r in sorted(REFUSALS["damaged streams"])],
    "inheritance": ["treeless, one stream", "treeless, four streams", "treeless block rebuilds a table above K1b's slots", "treeless after huf, then another block type, log 12",
                    "a new table of log 5 after one of log 12", "a new table of log 12 after one of log 5", "table above K1b's slots in a frame of several blocks",
                    "refused: weights: fewer than two weights of 1", "refused: literals: treeless with nothing to inherit"],
    "dictionaries": ["dictionary table log 11", "dictionary table log 12", "treeless after dictionary, log 11", "treeless after dictionary, log 12", "treeless, one stream",
                     "treeless, four streams"],
}
