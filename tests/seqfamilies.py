"""Scenario generators for tests/test_emu_sequences.py, tests/test_gpu_sequences.py and tests/stress_emu_sequences.py (test infrastructure).

Every generator is deterministic (seeded), takes the kernel constants (seqmodel.K3Consts) as a parameter, and returns Cases: a frame DESCRIBED by
blocks of explicit sequences. Case.build() writes the frame (tests/craft.py) and computes what it must decode to (seqmodel.execute); which of K3's
limits a family reaches, and from which side, is asserted with seqmodel.census by the tests, never assumed here.

A generator aims at a batch boundary by construction: a batch is the next 64 sequences unless bytes cut it short, so `fill(64, T)` -- 64 plain
sequences of T bytes together -- is one batch that leaves T bytes of history (T a multiple of 16: no carried tail), and what follows it opens the
next batch at a known position."""
import numpy as np

from tests import craft, seqmodel
from tests.seqmodel import K3


class Case:
    def __init__(self, family, name, blocks, dict_data=None, raw_dict=True, fcs="auto", checksum=None, start_reps=(1, 4, 8), header=None, cap=None, short_by=0):
        self.family, self.name, self.blocks = family, name, blocks
        self.dict_data, self.raw_dict, self.start_reps = dict_data, raw_dict, start_reps
        self.fcs, self.checksum, self.header, self.cap = fcs, checksum, header or {}, cap
        self.short_by = short_by
        self.unjudged = None                                                   # or: why libzstd is not asked about this frame
        self.frame = self.want = None

    def dict_content(self):
        if not self.dict_data: return b""
        return self.dict_data if self.raw_dict else self.dict_data[self.content_off:]

    def build(self, xxh64=None):
        """writes .frame; .want = the bytes it must decode to, or None (it must be refused); .cap = the slot it is decoded into"""
        try:
            self.content = seqmodel.execute(self.blocks, self.dict_content(), self.start_reps)
            self.why = None
        except seqmodel.Invalid as e:
            self.content, self.why = None, e.reason
        n = len(self.content) if self.content is not None else self.header.get("claims", 0)
        fcs = n if self.fcs == "auto" else self.fcs
        ck = None
        if self.checksum is not None:
            ck = (xxh64(self.content or b"") + (0 if self.checksum == "right" else 1)) & 0xFFFFFFFF
        h = {k: v for k, v in self.header.items() if k != "claims"}
        self.frame = craft.write_frame(self.blocks, fcs=fcs, checksum=ck, **h)
        self.want = self.content
        if self.content is not None and fcs is not None and fcs != n: self.want, self.why = None, "content size differs from the header's"
        if self.checksum == "wrong": self.want, self.why = None, "wrong content checksum"
        if self.cap is None: self.cap = (fcs if fcs is not None else n) - self.short_by
        if self.want is not None and self.cap < len(self.want): self.want, self.why = None, "slot too small"
        return self

    def with_lead(self):
        """the several-block form: a 1-byte raw block in front"""
        c = Case(self.family, self.name + " [after a raw block]", [("raw", b"L")] + list(self.blocks), self.dict_data, self.raw_dict,
                 self.fcs if self.fcs in ("auto", None) else self.fcs + 1, self.checksum, self.start_reps, dict(self.header),
                 None if self.cap is None or self.frame is not None else self.cap + 1, self.short_by)
        if "claims" in c.header: c.header["claims"] += 1
        if self.dict_data and not self.raw_dict: c.content_off = self.content_off
        c.unjudged = self.unjudged
        return c

    def census(self, k=K3):
        return seqmodel.census(self.blocks, k, len(self.dict_content()), self.start_reps)


class Builder:
    """sequences of one compressed block, by absolute position; literal bytes are drawn at the end (values 0..100, skewed, so a Huffman table fits)"""
    def __init__(self, rng, pos=0):
        self.rng, self.pos, self.seqs, self.nlit = rng, pos, [], 0

    def seq(self, ll, ml, off):
        self.seqs.append((ll, ml, off + 3)); self.pos += ll + ml; self.nlit += ll
        return self

    def rep(self, ll, ml, code):
        self.seqs.append((ll, ml, code)); self.pos += ll + ml; self.nlit += ll
        return self

    def at(self, ll, ml, src):
        """a match whose source starts at absolute position `src`"""
        return self.seq(ll, ml, self.pos + ll - src)

    def fill(self, n, total, far=None):
        """n plain sequences of `total` bytes together (each at least 1 literal + a 3-byte match, offsets anywhere in what exists)"""
        assert total >= 4 * n
        sizes = [total // n + (1 if i < total % n else 0) for i in range(n)]
        for s in sizes:
            ml = int(self.rng.integers(3, min(s - 1, 12) + 1)); ll = s - ml
            have = self.pos + ll
            off = int(self.rng.integers(1, have + 1)) if far is None else min(have, far)
            self.seq(ll, ml, off)
        return self

    def block(self, rest=0, **opts):
        n = self.nlit + rest
        lits = bytes(np.minimum(self.rng.integers(0, 101, n), self.rng.integers(0, 101, n)).astype(np.uint8))
        self.pos += rest
        return ("seq", lits, list(self.seqs), dict(opts))


def lit_variant(blocks, mode):
    """the same sequences with the literals section of every compressed block in `mode`: "rle" (one byte value), "huf" (one stream below 1 000
    literals, four from 64), "raw2" / "raw3" (the longer raw headers)"""
    out = []
    for b in blocks:
        if b[0] != "seq": out.append(b); continue
        lits, seqs, o = b[1], b[2], dict(b[3]) if len(b) > 3 else {}
        if mode == "rle" and lits: lits = bytes([lits[0] | 1]) * len(lits); o["lit"] = "rle"
        elif mode == "huf" and len(set(lits)) >= 2: o["lit"] = "huf4" if len(lits) >= 1000 else "huf1"
        elif mode == "huf4" and len(set(lits)) >= 2 and len(lits) >= 64: o["lit"] = "huf4"
        elif mode == "raw2" and len(lits) < 4096: o["lit_hdr"] = 2
        elif mode == "raw3": o["lit_hdr"] = 3
        out.append(("seq", lits, seqs, o))
    return out


LIT_LENGTHS = (0, 1, 8, 15, 16, 17, 31, 32, 33, 48, 100, 700)


def literal_runs(k=K3, seed=1):
    rng = np.random.default_rng(seed)
    cases = []
    for rest in (0, 9):
        b = Builder(rng).seq(3, 4, 2)
        for ll in LIT_LENGTHS + LIT_LENGTHS[::-1]: b.seq(ll, int(rng.integers(3, 9)), int(rng.integers(1, b.pos + ll + 1)))
        b.seq(k.asm_bytes + 5, 4, 7)                                           # more than a batch's room
        for ll in LIT_LENGTHS: b.seq(ll, 5, int(rng.integers(1, 300)))
        blk = b.block(rest=rest)
        for mode in ("raw", "raw2", "raw3", "huf", "rle"):
            cases.append(Case("literal runs", "lengths 0..700 and above the room, %s, %d last literals" % (mode, rest), lit_variant([blk], mode)))
    small = Builder(rng).seq(20, 4, 3).seq(0, 3, 9).seq(17, 3, 2).block(rest=3)
    cases += [Case("literal runs", "a small block, raw literals with a 2-byte header", lit_variant([small], "raw2")),
              Case("literal runs", "a small block, raw literals with a 3-byte header", lit_variant([small], "raw3")),
              Case("literal runs", "a small block, one Huffman stream", lit_variant([small], "huf")),
              Case("literal runs", "a small block, RLE literals", lit_variant([small], "rle"))]
    for mode in ("raw", "huf", "huf4", "rle"):
        cases.append(Case("literal runs", "no sequences, %s" % mode, lit_variant([Builder(rng).block(rest=300)], mode)))
    cases.append(Case("literal runs", "no sequences, more literals than a batch's room", [Builder(rng).block(rest=k.asm_bytes + 100)]))
    cases.append(Case("literal runs", "last literals above a batch's room", [Builder(rng).seq(5, 5, 2).block(rest=k.asm_bytes + 33)]))
    # treeless: the second block reuses the first one's Huffman table
    b1 = Builder(rng).seq(30, 4, 3).fill(20, 600).block(rest=5, lit="huf4")
    b2 = Builder(rng, 0).seq(17, 4, 3).seq(40, 6, 20).seq(3, 3, 1).block(rest=2)
    tl = set(b1[1])
    b2 = ("seq", bytes(x if x in tl else b1[1][0] for x in b2[1]), b2[2], {"lit": "treeless1"})
    b3 = ("seq", b1[1][:300], [(100, 5, 40), (150, 9, 3)], {"lit": "treeless4"})
    cases.append(Case("literal runs", "treeless literals after a Huffman block", [b1, b2, b3]))
    return cases


def _opened(rng, k, history_batches=2):
    """a block that starts with a big literal run (so the LDS history does not reach the frame's first byte) and `history_batches` batches of 64
    sequences, 1 024 bytes each: returns (builder, position where the history starts). The next sequence opens a batch with no carried tail."""
    b = Builder(rng).seq(k.asm_bytes + 40, 8, 11)
    h0 = b.pos
    per = 512 if k.asm_bytes >= 4096 else 256
    for _ in range(history_batches): b.fill(64, per)
    return b, h0


def far_matches(k=K3, seed=2):
    rng = np.random.default_rng(seed)
    cases = []
    for ml in (3, 16, 17, 40, 200):
        b, h0 = _opened(rng, k)
        ob = b.pos
        for src in (100, h0 + 300, h0, h0 - 1, ob - ml, ob - ml + 1, ob - 1, h0 - ml, h0 - ml + 1):
            b.at(int(rng.integers(1, 4)), ml, src)
        b.fill(64 - 9, 400)
        cases.append(Case("far matches", "length %d: below, inside, at and around the history's first byte, ending at the batch" % ml, [b.block(rest=3)]))
    # units per batch: 0 (short items only), 64, 65, above 128 -- the unit pass's second trip starts at 65
    for name, items in (("0", [(4, 5)] * 30), ("64", [(2, 1024)]), ("65", [(2, 1025)]), ("64 in pairs", [(17, 17)] * 16), ("above 128", [(1040, 1025)])):
        b = Builder(rng).seq(k.asm_bytes + 40, 8, 11)
        b.fill(64, 640, far=3000)                                               # (short far matches below an empty history: no units)
        for ll, ml in items: b.seq(ll, ml, b.pos + ll - 50 if ml > 16 else 2000)
        b.fill(64 - len(items), 256, far=3000)
        if k.asm_bytes >= 4096 or name in ("0", "64 in pairs"):
            cases.append(Case("far matches", "units in one batch: " + name, [b.block()]))
    return cases


NEAR_OFFSETS = tuple(range(1, 34)) + (63, 64, 65)


def near_matches(k=K3, seed=3):
    rng = np.random.default_rng(seed)
    cases = []
    b = Builder(rng).seq(70, 3, 70)
    for of in NEAR_OFFSETS:
        for ml in sorted({3, 4, 15, 16, 17, 31, 32, 33, 100, of, of + 1, max(3, of - 1)}):
            if ml >= 3: b.seq(int(rng.integers(0, 4)), ml, of)
    cases.append(Case("near matches", "offsets 1-33, 63, 64, 65 x lengths 3-33 and 100", [b.block(rest=1)]))
    b = Builder(rng).seq(70, 3, 70)
    for of in (1, 2, 3, 7, 31, 32, 33, 63, 64, 65, 100):
        b.seq(int(rng.integers(0, 3)), 700, of).fill(63, 300)
    cases.append(Case("near matches", "whole-wave matches of 700 bytes, offsets below and from 64", [b.block()]))
    # a part in front of the batch: the batch opens with a match whose source starts p bytes before it
    b = Builder(rng).fill(64, 512)
    for p in (1, 2, 15, 16, 17, 40, 300):
        for ml in (max(3, p + 1), p + 10, p + 40):
            b.seq(2, ml, p + 2)                                                 # the batch's first sequence: its source starts p bytes before the batch
            b.fill(63, 512 + (-(2 + ml)) % 16)                                  # together a multiple of 16: the next batch starts without a tail
    cases.append(Case("near matches", "pre-batch parts of 1 to 300 bytes", [b.block(rest=2)]))
    # dependency chains: every match reads the one before it
    for depth in (1, 2, 3, 8, 40, 62, 63, 64):
        b = Builder(rng).fill(64, 512).seq(8, 4, 6)
        for _ in range(depth - 1): b.seq(1, 4, 5)
        if depth < 64: b.fill(64 - depth, 16 * 40 - (12 + 5 * (depth - 1)) % 16, far=400)
        b.fill(64, 512)
        cases.append(Case("near matches", "a chain of %d dependent matches in one batch" % depth, [b.block()]))
    # exact edges of the dependency search: the last byte, the first byte, only the literals in between
    b = Builder(rng).fill(64, 512)
    b.seq(4, 6, 3).seq(5, 3, 6)                                                 # B reads A's last byte and two literals
    b.seq(4, 6, 3); a_beg = b.pos - 6
    b.seq(9, 3, 0 + (b.pos + 9) - (a_beg - 2))                                  # C reads two literals and A's first byte
    b.seq(4, 6, 3).seq(12, 5, 9)                                                # D reads only the literals between two matches
    b.seq(4, 40, 3).seq(5, 3, 6)                                                # the same two edges behind a whole-wave match, which a round serves AFTER its short ones
    b.seq(4, 40, 3); a_beg = b.pos - 40
    b.seq(9, 3, (b.pos + 9) - (a_beg - 2))
    b.fill(64 - 10, 300)
    cases.append(Case("near matches", "a match reading exactly the last / first byte of an earlier one, and only literals between two", [b.block()]))
    return cases


def batch_shapes(k=K3, seed=4):
    rng = np.random.default_rng(seed)
    A = k.asm_bytes
    cases = []
    b = Builder(rng).fill(64, 512).fill(30, 30 * 200).fill(64, 300)
    cases.append(Case("batch shape", "batches of 64 sequences and batches cut by bytes", [b.block()]))
    for over in (0, 1):
        b = Builder(rng).fill(9, A - 300).seq(100, 200 + over, 50).fill(20, 400)
        cases.append(Case("batch shape", "ten sequences of the room's %d bytes%s" % (A, " + 1" if over else ""), [b.block()]))
        b = Builder(rng).fill(64, 512 + 5).fill(9, A - 512 - 300 - 5).seq(100, 200 + over, 50).fill(20, 400)         # with a history and a carried tail of 5
        cases.append(Case("batch shape", "behind a history and a tail: the room%s" % (" + 1" if over else ""), [b.block()]))
    blocks = []
    for c in range(16):
        blocks.append(Builder(rng, 1).fill(10, 160 + c).block(rest=c % 3))
    cases.append(Case("batch shape", "blocks that end with a carried tail of 0 ... 15", [("raw", b"x")] + blocks))
    b = Builder(rng)
    for i in range(17): b.fill(64, 256 + 1)
    cases.append(Case("batch shape", "every carried tail in turn", [b.block()]))
    for name, ll, ml in (("literals", A + 900, 3), ("match", 2, A + 1900), ("both", A + 900, A + 1900)):
        b = Builder(rng).fill(64, 512).fill(64, 512 + 7)
        b.seq(ll, ml, 300)                                                      # big, directly after a history (and a tail of 7)
        b.seq(3, 20, 100).seq(1, 5, 4 + ml).seq(2, 40, 3000)                     # directly before matches into what it wrote and into the old history
        b.fill(61, 400)
        cases.append(Case("batch shape", "a big item (%s) between a history and matches into it" % name, [b.block(rest=1)]))
    S, KEEP = k.hist_slide, k.hist_keep
    for extra in (0, 16):
        b = Builder(rng).fill(64, S + extra)
        if not extra: b.fill(64, 256)                                           # at the mark nothing slides; this batch passes it
        ob = b.pos
        for ml in (5, 16, 17, 40):
            for src in (ob - KEEP, ob - KEEP - 1, ob - KEEP - ml, ob - KEEP + 100, ob - KEEP - 200, ob - 1 - ml):
                b.at(2, ml, src)
        b.fill(64 - 24, 200)
        cases.append(Case("batch shape", "history at the slide mark%s, then sources in and just outside the kept region" % (" + 16" if extra else ""), [b.block()]))
    return cases


def slot_edges(k=K3, seed=5):
    rng = np.random.default_rng(seed)
    cases = []
    for n in (1, 5, 31):
        cases.append(Case("slot edges", "%d bytes of output" % (n + 3), [Builder(rng).seq(n, 3, 1).block()]))
    cases.append(Case("slot edges", "20 bytes, matches only near the slot's end", [Builder(rng).seq(6, 4, 2).seq(1, 3, 9).seq(0, 3, 1).block(rest=3)]))
    b = Builder(rng).seq(k.asm_bytes + 40, 8, 11)                                # (a big item: no LDS history behind it, the sources are read from the slot)
    ob = b.pos
    b.at(2, 4, ob - 6).at(1, 3, ob - 4).at(0, 9, ob - 9).at(1, 3, ob - 20)       # short far items whose sources lie in the slot's last 32 bytes
    cases.append(Case("slot edges", "short far matches within 32 bytes of the slot's end", [b.block(rest=1)]))
    for big in (False, True):                                                   # from the LDS history; from the slot itself, behind a big item
        b = Builder(rng).seq(k.asm_bytes + 40, 8, 11) if big else Builder(rng).fill(64, 256)
        b.at(2, 20, b.pos - 20)
        cases.append(Case("slot edges", "a far match in units within 32 bytes of the slot's end" + (", no history" if big else ""), [b.block(rest=1)]))
    short = Builder(rng).fill(64, 256).seq(3, 9, 100).block(rest=2)
    cases.append(Case("slot edges", "a slot one byte short", [short], short_by=1))
    return cases


def extremes(k=K3, seed=6):
    rng = np.random.default_rng(seed)
    cases = []
    for ll in (65535, 65536):
        cases.append(Case("extremes", "literal length %d" % ll, [Builder(rng).seq(ll, 5, 7).seq(2, 3, 1).block(rest=1)]))
    cases.append(Case("extremes", "literal length 131 071 (more than a block holds)", [("seq", bytes(1000), [(131071, 3, 4)], {})], header={"claims": 131074}))
    # (131 072, the longest a block holds, needs a byte to copy from: the frame's own raw block in front; from a dictionary: raw_dictionaries)
    cases.append(Case("extremes", "match length 131 072 behind a raw block", [("raw", b"L"), Builder(rng, 1).seq(0, 131072, 1).block()]))
    for ml in (65538, 65539, 131071):
        cases.append(Case("extremes", "match length %d" % ml, [Builder(rng).seq(1, ml, 1).block()] if ml == 131071 else [Builder(rng).seq(40, ml, 33).seq(2, 3, 1).block(rest=1)]))
    return cases


def many_blocks(k=K3, seed=7):
    """nine blocks and more: offsets above 128 KiB that reach the frame's first byte, and the sequence with the most extra bits at once"""
    rng = np.random.default_rng(seed)
    head = bytes(rng.integers(0, 256, 1000, dtype=np.uint8))
    blocks = [("raw", head)] + [("rle", 0x40 + i, 131072) for i in range(8)]
    pos = 1000 + 8 * 131072
    b = Builder(rng, pos)
    b.at(40000, 65539 + 300, 0)                                                 # LL code 34, ML code 52, offset code 20: 15 + 16 + 20 extra bits
    b.at(3, 900, 5).at(0, 40, 0).at(2, 3, 999)
    blocks.append(b.block(rest=4))
    blocks.append(Builder(rng, b.pos).rep(3, 10, 1).rep(0, 5, 1).at(1, 700, 100).block())
    return [Case("many blocks", "ten blocks: offsets of 1 MiB back to the frame's first byte, 51 extra bits in one sequence", blocks, header={"window_log": 21})]


OPENING = [(ofv, ll) for ofv in (1, 2, 3, None) for ll in (0, 2)]


def repeat_offsets(k=K3, seed=8, depth=3, blocks_per_frame=7):
    """every opening of `depth` sequences over offset value {1, 2, 3, new} x literal length {0, > 0}, each as a block that follows a block which
    left another history; chains of 'repeat offset 1 minus one'; raw, RLE and sequence-less blocks in between; blocks of repeat codes only"""
    rng = np.random.default_rng(seed)
    cases = []
    combos = [[]]
    for _ in range(depth): combos = [c + [o] for c in combos for o in OPENING]
    for f0 in range(0, len(combos), blocks_per_frame):
        first = Builder(rng).seq(90, 5, 17).seq(3, 4, 29).seq(2, 6, int(rng.integers(40, 60)))
        blocks = [first.block(rest=2)]
        pos = first.pos
        for n, combo in enumerate(combos[f0:f0 + blocks_per_frame]):
            b = Builder(rng, pos)
            for ofv, ll in combo:
                if ofv is None: b.seq(ll, 4, int(rng.integers(9, 80)))
                else: b.rep(ll, int(rng.integers(3, 7)), ofv)
            b.seq(1, 3, int(rng.integers(9, 80))).seq(2, 3, int(rng.integers(9, 80)))         # leaves the next block another history
            blocks.append(b.block(rest=n % 2)); pos = b.pos
            if (f0 + n) % 5 == 0: blocks.append(("raw", b"between")); pos += 7
            if (f0 + n) % 7 == 0: blocks.append(("rle", 0x55, 9)); pos += 9
            if (f0 + n) % 11 == 0: blocks.append(("seq", b"only literals", [], {})); pos += 13
        cases.append(Case("repeat offsets", "openings %d-%d" % (f0, f0 + blocks_per_frame - 1), blocks))
    for chain in (2, 3, 5, 9):
        first = Builder(rng).seq(90, 5, 17).seq(3, 4, 29).seq(2, 6, 12)
        b = Builder(rng, first.pos)
        for _ in range(chain): b.rep(0, 3, 3)
        cases.append(Case("repeat offsets", "'repeat offset 1 minus one' %d times after a block boundary" % chain, [first.block(), b.block()]))
        b2 = Builder(rng, b.pos)
        for _ in range(chain): b2.rep(0, 3, 3)
        cases.append(Case("repeat offsets", "... and %d more in a third block, behind a raw block" % chain, [first.block(), b.block(), ("raw", b"r"), b2.block(rest=1)]))
    for left in (1, 2, 3):                                                      # the chain reaches 0: invalid, the invalid block last
        first = Builder(rng).seq(90, 5, 17).seq(3, 4, 29).seq(2, 6, left)
        b = Builder(rng, first.pos)
        for _ in range(left): b.rep(0, 3, 3)
        cases.append(Case("repeat offsets", "a chain from %d that reaches 0" % left, [first.block(), b.block()], header={"claims": first.pos + 3 * left}))
    first = Builder(rng).seq(90, 5, 17).seq(3, 4, 29).seq(2, 6, 12)
    blocks = [first.block()]; pos = first.pos
    for n in range(4):
        b = Builder(rng, pos).rep(n % 2, 3, 2).rep(1, 4, 3).rep(0, 3, 1).rep(2, 5, 1).rep(0, 4, 2)
        blocks.append(b.block()); pos = b.pos
    cases.append(Case("repeat offsets", "four blocks in a row that use repeat codes only", blocks))
    return cases


def raw_dictionaries(k=K3, seed=9):
    rng = np.random.default_rng(seed)
    dd = bytes(rng.integers(0, 256, 3000, dtype=np.uint8))
    D = len(dd)
    cases = []

    def case(name, blocks, **kw): cases.append(Case("raw dictionaries", name, blocks, dict_data=dd, raw_dict=True, **kw))
    case("sources wholly in the dictionary, ending at the frame's first byte", [Builder(rng).seq(0, 10, 50).seq(2, 12, 14).seq(1, 5, D + 13).fill(61, 400).at(3, 20, -20).at(1, 9, -9).at(2, 40, -2000).block(rest=1)])
    case("seven bytes of output from the dictionary", [Builder(rng).seq(0, 5, 50).block(rest=2)])
    case("a first match that runs from the dictionary into its own output", [Builder(rng).seq(0, 40, 8).seq(1, 100, 3).block()])
    b = Builder(rng).fill(64, 1024)
    b.at(2, 12, -6).at(1, 16, -1).at(0, 17, -16).at(3, 300, -100).at(1, 900, -10).at(2, 700, -690).fill(58, 300)
    case("straddlers: short, long and reading their own output", [b.block()])
    b = Builder(rng).seq(7, 5, 7 + D).seq(2, 4, 14 + D)
    case("an offset of exactly position + dictionary size", [b.block()])
    b = Builder(rng).seq(7, 5, 7 + D).seq(2, 4, 14 + D + 1)
    case("an offset one beyond position + dictionary size", [b.block()], header={"claims": 18})
    case("match length 131 072 from the dictionary's last byte", [Builder(rng).seq(0, 131072, 1).block()])
    return cases


def trained_dictionaries(dict_bytes, content_off, reps, k=K3, seed=10):
    """frames for a trained dictionary: the first sequences use repeat codes, so they start from the dictionary's own history"""
    rng = np.random.default_rng(seed)
    cases = []
    for name, first in (("1", [(2, 5, 1), (0, 4, 1), (0, 3, 2)]), ("2 with no literals", [(0, 5, 2), (3, 4, 2)]), ("3", [(4, 6, 3), (0, 4, 3)]), ("3 with no literals, which is zero and refused", [(0, 5, 3), (0, 3, 3)])):
        b = Builder(rng)
        for ll, ml, c in first: b.rep(ll, ml, c)
        b.fill(20, 300)
        c = Case("trained dictionaries", "a frame that opens with repeat code " + name, [b.block(rest=2)], dict_data=dict_bytes, raw_dict=False, start_reps=reps)
        c.content_off = content_off
        cases.append(c)
    return cases


def invalid_frames(k=K3, seed=11):
    rng = np.random.default_rng(seed)
    cases = []

    def case(name, blocks, n, **kw): cases.append(Case("invalid frames", name, blocks, header={"claims": n}, **kw))
    b = Builder(rng).fill(64, 512)
    b.seqs.append((2, 5, b.pos + 2 + 1 + 3)); b.nlit += 2
    case("an offset one beyond the history", [b.block()], 519)
    good = Builder(rng).fill(64, 512).block(rest=4)
    case("literal lengths that sum past the section", [("seq", good[1][:-40], good[2], {})], 516)
    over = [Builder(rng).seq(10, 131072, 1).block()]
    case("output past the 128 KiB block maximum, no content size in the header", over, 131082, fcs=None)
    # The same block with the content size declared: libzstd's one-pass decoder bounds a block's literals and compressed size but not its output
    # (DESIGN.md 4.1), and with more room it keeps the literals inside the destination, 128 KiB + 32 bytes on, where such a block writes over them.
    # Its answer for a block that breaks the format's limit is therefore no specification; the decoders here refuse the block, and this case pins that.
    c = Case("invalid frames", "output past the 128 KiB block maximum, content size declared", over, header={"claims": 131082})
    c.unjudged = "libzstd's one-pass decoder does not bound a block's output"
    cases.append(c)
    fine = Builder(rng).fill(70, 800).block(rest=4)
    cases.append(Case("invalid frames", "output one byte past the declared content size", [fine], fcs=803))
    cases.append(Case("invalid frames", "output one byte short of the declared content size", [fine], fcs=805))
    cases.append(Case("invalid frames", "a wrong content checksum", [fine], checksum="wrong"))
    cases.append(Case("invalid frames", "the same frame with the right checksum", [fine], checksum="right"))
    return cases


def header_forms(k=K3, seed=12, longest=False):
    """longest: only the block of 32 512 sequences (the 3-byte count), which takes the emulator half a minute per route"""
    rng = np.random.default_rng(seed)
    blk = Builder(rng).fill(70, 800).block(rest=4)
    cases = []
    for name, h, fcs in (("single segment", {"single_segment": True}, "auto"), ("window descriptor, content size", {"window_log": 12}, "auto"),
                         ("8-byte content size", {"window_log": 17, "fcs_bytes": 8}, "auto"), ("2-byte content size", {"single_segment": True, "fcs_bytes": 2}, "auto")):
        cases.append(Case("header forms", name, [blk], header=h, fcs=fcs))
        cases.append(Case("header forms", name + ", checksum", [("raw", b"abc"), blk, ("rle", 7, 50)], header=h, fcs=fcs, checksum="right"))
    for modes in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        seqs = [(5 if modes[0] else 8 if i == 0 else int(rng.integers(1, 9)), 7 if modes[2] else int(rng.integers(3, 9)),
                 (8 + (int(rng.integers(0, 4)) if i else 0)) if modes[1] else 4 + int(rng.integers(0, 4))) for i in range(200)]
        lits = bytes(rng.integers(0, 100, sum(q[0] for q in seqs), dtype=np.uint8))
        cases.append(Case("header forms", "RLE-mode tables %s, 2-byte sequence count" % (modes,), [("seq", lits, seqs, {"modes": modes})]))
    seqs = [(1, 3, 4)] * 0x7F00
    if longest: return [Case("header forms", "32 512 sequences: the 3-byte count", [("seq", bytes(rng.integers(0, 100, len(seqs), dtype=np.uint8)), seqs, {})])]
    cases.append(Case("header forms", "5 sequences, count in 2 bytes", [("seq", b"abcdefghij", [(2, 3, 4)] * 5, {"count_bytes": 2})]))
    return cases


def k3_families(k=K3):
    """the families that aim at zp_exec_block's limits (what the -DZP_ASM_BYTES variant build runs too)"""
    return literal_runs(k) + far_matches(k) + near_matches(k) + batch_shapes(k) + slot_edges(k)


def plain_families(k=K3):
    """everything without a dictionary that a batch of small and middling frames can hold (header_forms(longest=True) and many_blocks run apart)"""
    return k3_families(k) + extremes(k) + repeat_offsets(k) + invalid_frames(k) + header_forms(k)


_OPEN_NAMES = [(v, l) for v in (1, 2, 3, "new") for l in ("0", "+")]
# The invalid frames never reach K3's batching and the header forms do not bear on it, so the census has nothing to say about them: their tests
# assert the reason each invalid frame is refused for (INVALID_REASONS) and the forms by name.
INVALID_REASONS = {"offset beyond the history", "literal lengths past the section", "block output above the block maximum",
                   "content size differs from the header's", "wrong content checksum"}
# what the census must report over k3_families() (in the one-block form or behind a raw block), by family
# (a batch with exactly ONE 16-byte unit does not exist: only items above 16 bytes are cut into units, and those have two at least)
REQUIRED = {
    "literal runs": ["%s literals: %s" % (m, n) for m in ("raw", "huf", "rle") for n in ("0", "1..15", "16", "17..32", "above 32")] + [
        "block without sequences", "last literals: none", "last literals: some", "last literals above a batch's room", "big item: literals"],
    "far matches": ["far match: up to 16", "far match: 17 and up", "far match: source below the history", "far match: source inside the history",
                    "far match: source starts at the history's first byte", "far match: source one byte before the history", "far match ends exactly at the batch",
                    "near match: source ends one byte past the batch's start", "pre-batch part: 1",
                    "units in a batch: 0", "units in a batch: 64", "units in a batch: 65", "units in a batch: above 128"],
    "near matches": ["near match: offset %s" % o for o in NEAR_OFFSETS] + [
        "near match: offset below the length", "near match: offset equal to the length", "near match: offset above the length",
        "near match: length up to 32", "near match: length 33", "near match: length long", "whole-wave near match: offset below 64", "whole-wave near match: offset 64 and up",
        "pre-batch part: 1", "pre-batch part: 2..16", "pre-batch part: above 16", "pre-batch part: up to 16", "pre-batch part: 17 and up",
        "dependency depth 1", "dependency depth 2..8", "dependency depth 9..62", "dependency depth 63 and up",
        "near match reads an earlier one's last byte", "near match reads an earlier one's first byte", "near match reads only this batch's literals"],
    "batch shape": ["batch of 64 sequences", "batch cut by bytes", "batch fills the room exactly", "first sequence left out is one byte above the room"] + [
        "carry %d" % c for c in range(16)] + ["carry %d at the block's end" % c for c in range(16)] + [
        "big item: literals", "big item: match", "big item: both", "big item after a history", "match into what a big item wrote",
        "history exactly at the slide mark", "slide", "slide 16 bytes past the mark", "after a slide: source in the kept region", "after a slide: source just outside it"],
    "slot edges": ["frame below 32 bytes", "short far match within 32 bytes of the slot's end", "far units within 32 bytes of the slot's end"],
    "extremes": ["literal length 65535", "literal length 65536", "match length 65538", "match length 65539", "match length 131072"],
    "many blocks": ["LL code 34, ML code 52 and an offset code of 20 or more in one sequence", "offset above 128 KiB back to the frame's first byte"],
    "repeat offsets": ["opening after a block boundary: " + " ".join("%s/%s" % o for o in (a, b, c))
                       for a in _OPEN_NAMES for b in _OPEN_NAMES for c in _OPEN_NAMES] + [
        "'repeat offset 1 minus one' after a block boundary: 2 times", "'repeat offset 1 minus one' after a block boundary: 3 times",
        "'repeat offset 1 minus one' after a block boundary: 4 and more times", "raw block between compressed blocks", "RLE block between compressed blocks",
        "block without sequences between compressed blocks", "three blocks in a row of repeat codes only"],
    "raw dictionaries": ["dictionary: source wholly inside", "dictionary: source wholly inside, ending at the frame's first byte",
                         "dictionary straddler: short", "dictionary straddler: long", "dictionary straddler: self-overlapping"],
}
