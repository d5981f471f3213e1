"""Case lists for tests/test_emu_k2_steps.py and tests/test_gpu_k2_steps.py (test infrastructure): frames aimed at ONE STEP of the sequence kernel
(zp_seqq_body) -- the trip count of its unrolled body, the widths of the fields its prefix sums place, the selects of the repeat
offsets, the upkeep of its ring -- rather than at K3's batching, which tests/seqfamilies.py aims at.

Frames are described as seqfamilies.Cases and written by craft.py's pieces; what craft.sequences_section lacks is added here: tables in the
COMPRESSED mode (an FSE table description in front of the stream, any accuracy log the format allows: 5 ... 9 for literal and match lengths,
5 ... 8 for offsets) and a sequence stream damaged on purpose. libzstd judges every frame before a kernel sees it (seqmodel.check_model)."""
import itertools

import numpy as np

from tests import craft, seqmodel
from tests import seqfamilies as F

MAX_LOG = (9, 8, 9)                    # LL, OF, ML (RFC 8878 3.1.1.3.2.1)


def write_ncount(norm, log):
    """the FSE table description of RFC 8878 4.1.1 for `norm` (probabilities, none 'less than one'; they sum to 1 << log; the last one is not 0)"""
    assert sum(norm) == 1 << log and norm[-1] > 0 and all(c >= 0 for c in norm)
    w = craft._Bits()
    w.add(log - 5, 4)
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    s, prev0 = 0, False
    while remaining > 1:
        if prev0:
            start = s
            while norm[s] == 0: s += 1
            while s >= start + 24: start += 24; w.add(0xFFFF, 16)
            while s >= start + 3: start += 3; w.add(3, 2)
            w.add(s - start, 2)
        count = norm[s]; s += 1
        mx = 2 * threshold - 1 - remaining
        remaining -= count
        count += 1
        if count >= threshold: count += mx
        w.add(count, nb - (1 if count < mx else 0))
        prev0 = count == 1
        while remaining < threshold: nb -= 1; threshold >>= 1
    assert s == len(norm)
    if w.n: w.out.append(w.acc)                                     # (no closing bit: the description ends on a byte boundary as it is)
    return bytes(w.out)


def _table(kind, spec, used):
    """(mode bits, bytes written behind the modes byte, (cells, log, {symbol: [states]})) of table `kind` (0 LL, 1 OF, 2 ML) for the codes in `used`.
    spec: "pre", "rle", or ("fse", log): every used code once, one more code so that there are two, the rest to the most frequent"""
    if spec == "pre": return 0, b"", craft._seq_table(kind)
    if spec == "rle":
        assert len(set(used)) == 1, "RLE mode needs one code for every sequence"
        return 1, bytes([used[0]]), craft._seq_table(kind, used[0])
    log = spec[1]
    assert spec[0] == "fse" and 5 <= log <= MAX_LOG[kind]
    syms = sorted(set(used))
    if len(syms) == 1: syms = sorted(set(syms) | {syms[0] + 1 if syms[0] == 0 else syms[0] - 1})
    assert len(syms) <= 1 << log
    norm = [0] * (syms[-1] + 1)
    for s in syms: norm[s] = 1
    norm[max(syms, key=lambda s: (list(used).count(s), s))] += (1 << log) - len(syms)
    cells = craft._decode_table(norm, log)
    by = {}
    for x, c in enumerate(cells): by.setdefault(c[0], []).append(x)
    return 2, write_ncount(norm, log), (cells, log, by)


def sequences_section(seqs, tables=("pre", "pre", "pre"), damage=None):
    """craft.sequences_section with a spec per table (LL, OF, ML), see _table; returns (section, bytes of its bit stream).
    damage: "zero last" (the stream's last byte, which holds the end mark, is 0), "extra byte" (one more byte than the sequences read, at the
    stream's start), "cut byte" (its first byte is missing)"""
    n = len(seqs)
    assert 0 < n < 0x7F00
    head = bytes([n]) if n < 128 else bytes([0x80 + (n >> 8), n & 255])
    codes = [craft.seq_codes(*q) for q in seqs]
    made = [_table(k, tables[k], [c[k][0] for c in codes]) for k in range(3)]
    head += bytes([(made[0][0] << 6) | (made[1][0] << 4) | (made[2][0] << 2)]) + b"".join(m[1] for m in made)
    tabs = [m[2] for m in made]
    w = craft._Bits()
    st = [tabs[k][2][codes[n - 1][k][0]][0] for k in range(3)]
    for i in range(n - 1, -1, -1):                                  # (as craft.sequences_section: backwards, fields in reverse of reading order)
        (_, lx, lb), (_, ox, ob), (_, mx, mb) = codes[i]
        if i < n - 1:
            upd = []
            for k in range(3):
                cells = tabs[k][0]; succ = st[k]
                x = next(x for x in tabs[k][2][codes[i][k][0]] if cells[x][2] <= succ < cells[x][2] + (1 << cells[x][1]))
                upd.append((succ - cells[x][2], cells[x][1])); st[k] = x
            w.add(*upd[1]); w.add(*upd[2]); w.add(*upd[0])
        w.add(lx, lb); w.add(mx, mb); w.add(ox, ob)
    w.add(st[2], tabs[2][1]); w.add(st[1], tabs[1][1]); w.add(st[0], tabs[0][1])
    stream = w.finish()
    if damage == "zero last": stream = stream[:-1] + b"\0"
    elif damage == "extra byte": stream = b"\x5a" + stream
    elif damage == "cut byte": stream = stream[1:]
    else: assert damage is None
    return head + stream, len(stream)


class Case(F.Case):
    """a seqfamilies.Case whose compressed blocks may carry the options "tables" and "damage" of sequences_section above (raw or RLE literals);
    .stream_bytes lists the sizes of its sequence bit streams once it is built"""
    def build(self, xxh64=None):
        assert self.checksum is None and not self.dict_data
        try: self.content, self.why = seqmodel.execute(self.blocks, b"", self.start_reps), None
        except seqmodel.Invalid as e: self.content, self.why = None, e.reason
        n = len(self.content) if self.content is not None else self.header["claims"]
        out, self.stream_bytes, damaged = [craft.frame_header(fcs=n, **{k: v for k, v in self.header.items() if k != "claims"})], [], False
        for i, b in enumerate(self.blocks):
            last = i == len(self.blocks) - 1
            if b[0] == "raw": out.append(craft.block(0, b[1], last))
            elif b[0] == "rle": out.append(craft.block(1, (b[1], b[2]), last))
            else:
                o = b[3] if len(b) > 3 else {}
                assert o.get("lit", "raw") in ("raw", "rle")
                if b[2]:
                    sec, nbytes = sequences_section(b[2], o.get("tables", ("pre", "pre", "pre")), o.get("damage"))
                    self.stream_bytes.append(nbytes); damaged |= o.get("damage") is not None
                else: sec = b"\0"
                out.append(craft.block(2, craft.literals_section(bytes(b[1]), o.get("lit", "raw"), o.get("lit_hdr")) + sec, last))
        self.frame = b"".join(out)
        self.want, self.cap = self.content, n
        if damaged: self.want, self.why = None, "damaged sequence stream"
        return self

    def with_lead(self):
        c = F.Case.with_lead(self)
        return Case(c.family, c.name, c.blocks, start_reps=c.start_reps, header=c.header)


def _opts(b, **o):
    return ("seq", b[1], b[2], o)


COUNTS = tuple(range(1, 10)) + (63, 64, 65)


def counts(seed=21):
    """nbSeq = 1 ... 9, 63, 64, 65: the trip count modulo the unrolled four, the pipeline's five extra trips, one- and two-sequence frames"""
    rng = np.random.default_rng(seed)
    return [Case("counts", "%d sequences" % n, [F.Builder(rng).fill(n, 7 * n + int(rng.integers(0, 9))).block(rest=n % 3)]) for n in COUNTS]


TABLE_KINDS = ("pre", "rle", "small", "large")


def _uniform_seqs(rng, rle, n=12):
    """sequences that allow RLE mode in the tables named in `rle` (one code there), as seqfamilies.header_forms draws them"""
    return [(5 if rle[0] else 8 if i == 0 else int(rng.integers(1, 9)), 7 if rle[2] else int(rng.integers(3, 9)),
             (8 + (int(rng.integers(0, 4)) if i else 0)) if rle[1] else 4 + int(rng.integers(0, 4))) for i in range(n)]


def table_modes(seed=22):
    """every combination of predefined / RLE / compressed at log 5 / compressed at the largest log over the three tables, then every log alone"""
    rng = np.random.default_rng(seed)
    cases = []

    def spec(kind, k): return kind if kind in ("pre", "rle") else ("fse", 5 if kind == "small" else MAX_LOG[k])
    for combo in itertools.product(TABLE_KINDS, repeat=3):
        seqs = _uniform_seqs(rng, [c == "rle" for c in combo], n=int(rng.integers(5, 14)))
        lits = bytes(rng.integers(0, 100, sum(q[0] for q in seqs) + 2, dtype=np.uint8))
        cases.append(Case("table modes", "LL %s, OF %s, ML %s" % combo, [("seq", lits, seqs, {"tables": tuple(spec(c, k) for k, c in enumerate(combo))})]))
    for log in range(5, 10):
        b = F.Builder(rng).fill(40, 700).block(rest=1)
        t = (("fse", log), ("fse", min(log, 8)), ("fse", log))
        cases.append(Case("table modes", "all three compressed at log %d" % log, [_opts(b, tables=t)]))
    return cases


def wide_fields(seed=23):
    """the largest offset code a frame of 128 KiB holds (17), literal-length code 35 and match-length code 52 (16 extra bits each) beside a 16-bit
    offset, and a long stream of mixed widths, on predefined and on 9 / 8 / 9-bit tables: fields at every bit position of the ring's rows"""
    rng = np.random.default_rng(seed)
    big = (("fse", 9), ("fse", 8), ("fse", 9))
    cases = [Case("wide fields", "offset code 17 with its 17 extra bits", [("seq", b"\x07" * 131069, [(131069, 3, 131069 + 3)], {"lit": "rle"})]),    # (RLE literals: the block itself must stay below 128 KiB)
             Case("wide fields", "literal-length code 35 and offset code 16 in one sequence", [F.Builder(rng).seq(65536 + 77, 3, 65536 + 40).seq(0, 4, 65600).block(rest=1)]),
             Case("wide fields", "match-length code 52 behind literal-length code 34", [F.Builder(rng).seq(40000, 65539 + 300, 39999).seq(1, 3, 2).block()])]
    for tables in (("pre", "pre", "pre"), big):
        b = F.Builder(rng).seq(3000, 3, 2999)
        for _ in range(260):
            ll = int(rng.choice([0, int(rng.integers(1, 16)), int(rng.integers(16, 64)), int(rng.integers(64, 1200))]))
            ml = int(rng.choice([int(rng.integers(3, 35)), int(rng.integers(35, 131)), int(rng.integers(131, 900))]))
            b.seq(ll, ml, int(rng.integers(1, b.pos + ll + 1)))
        assert b.pos < 128 * 1024
        cases.append(Case("wide fields", "260 sequences of mixed field widths, %s tables" % ("predefined" if tables[0] == "pre" else "9 / 8 / 9-bit"), [_opts(b.block(rest=5), tables=tables)]))
    return cases


def selects(seed=24):
    """one block of 400 sequences drawn over offset value {1, 2, 3, new} x literal length {0, > 0}: every arm of the repeat-offset selects behind
    every other; a frame whose 'repeat offset 1 minus one' reaches zero is kept as one that must be refused"""
    cases = []
    for s in range(4):
        rng = np.random.default_rng(seed + 100 * s)
        b = F.Builder(rng).seq(200, 5, 17).seq(3, 4, 29).seq(2, 6, 44)
        for _ in range(400):
            ll = 0 if rng.integers(0, 2) else int(rng.integers(1, 6))
            ofv = int(rng.integers(1, 5))
            if ofv == 4: b.seq(ll, int(rng.integers(3, 8)), int(rng.integers(2, 120)))
            else: b.rep(ll, int(rng.integers(3, 8)), ofv)
        if s == 0: b.seq(2, 4, 1).rep(0, 3, 3)                                  # (offset 1, then 'repeat offset 1 minus one')
        blk = b.block(rest=s)
        cases.append(Case("selects", "400 sequences over the repeat codes, draw %d" % s, [blk], header={"claims": b.pos}))
    return cases


STREAM_BYTES = tuple(range(1, 18))


def ring_edges(seed=25):
    """sequence streams of 1 ... 17 bytes (three one-cell tables: no state bits, the two extra bits of offset code 2 per sequence), and streams on the predefined
    tables whose sizes cover every residue modulo the ring's 16-byte blocks and reach past its 128 bytes"""
    rng = np.random.default_rng(seed)
    cases = []
    for nbytes in STREAM_BYTES:
        n = 1 if nbytes == 1 else 4 * (nbytes - 1)
        seqs = _uniform_seqs(rng, (True, False, True), n)
        lits = bytes(rng.integers(0, 100, sum(q[0] for q in seqs), dtype=np.uint8))
        cases.append(Case("ring edges", "a stream of %d bytes" % nbytes, [("seq", lits, seqs, {"tables": ("rle", "rle", "rle")})]))
    for n in range(10, 42, 2):
        cases.append(Case("ring edges", "%d sequences on the predefined tables" % n, [F.Builder(rng).fill(n, 9 * n).block()]))
    for n in (100, 101, 200, 333):
        cases.append(Case("ring edges", "%d sequences: the ring turns over" % n, [F.Builder(rng).fill(n, 11 * n).block(rest=2)]))
    return cases


def damaged(seed=26):
    """valid frames with the sequence stream damaged: no end mark, one byte too many, one byte missing"""
    rng = np.random.default_rng(seed)
    cases = []
    for n in (1, 2, 5, 40):
        for how in ("zero last", "extra byte", "cut byte"):
            b = F.Builder(rng).fill(n, 9 * n).block(rest=1)
            cases.append(Case("damaged", "%d sequences, %s" % (n, how), [_opts(b, damage=how)]))
    return cases


def all_cases():
    """every family above, then seqfamilies' repeat offsets and invalid frames (seqfamilies.Cases)"""
    return counts() + table_modes() + wide_fields() + selects() + ring_edges() + damaged() + F.repeat_offsets() + F.invalid_frames()


BATCHES = (1, 14, 15, 16, 31)          # frames per call: part of a group of 15, all but one, a whole group, a second group of one, two groups and one


def batch_of(n, seed=27):
    """n frames of mixed sequence counts in shuffled order: lanes run on past their frame's last sequence while their neighbours go on"""
    rng = np.random.default_rng(seed + n)
    pool = counts(seed + n) + ring_edges(seed + n)
    return [pool[int(i)] for i in rng.permutation(len(pool))[:n]]
