"""Hand-made zstd frames for cases no encoder emits (test infrastructure).

`sequences_block()` writes a compressed block whose sequences use the PREDEFINED FSE tables (RFC 8878 3.1.1.3.2.2), from explicit
(literal length, match length, offset VALUE) triples -- the offset value is the number in the stream (1..3 = repeat codes, n + 3 = a
new offset n), so a test can ask for "repeat offset 1 minus one" where that is zero, which libzstd 1.5.7 refuses
(zstd/zstd.c:46941 "0 is not valid: input corrupted => force offset to -1").  The tables are built as the format says (the decoder's
spread and state assignment); encoding walks the sequences backwards choosing, for every symbol, the one state whose range holds the
state that follows.  Values are read from oracle/zo_common's tables through the oracle library so that nothing is typed twice."""
import ctypes as C

from tests import reflib

_LL_BASE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096,
            8192, 16384, 32768, 65536]
_LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
_ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
_ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def _defnorm(name, n):
    lib = C.CDLL(reflib.ORACLE_SO)
    return list((C.c_int16 * n).in_dll(lib, name))


def _decode_table(norm, log):
    """[(symbol, nbBits, base)] per state, as the format's decoder builds it."""
    size = 1 << log
    sym = [0] * size
    high = size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s; high -= 1
    step, mask, pos = (size >> 1) + (size >> 3) + 3, size - 1, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & mask
            while pos > high: pos = (pos + step) & mask
    nxt = [1 if c == -1 else c for c in norm]
    cells = []
    for x in range(size):
        s = sym[x]; n = nxt[s]; nxt[s] += 1
        nb = log - (n.bit_length() - 1)
        cells.append((s, nb, (n << nb) - size))
    return cells


def _code(value, base):
    c = 0
    for i, b in enumerate(base):
        if b <= value: c = i
    return c


def sequences_block(literals, seqs, last=True, of_rle=False):
    """One compressed block: raw literals + `seqs` = [(ll, ml, offset_value)] on predefined tables. Returns block header + content.
    of_rle: the offset codes in RLE mode (one code for every sequence, any of 0..31 -- the predefined table ends at 28)."""
    assert len(literals) < 32 and 0 < len(seqs) < 128
    tabs = [(_decode_table(_defnorm("zo_ll_defnorm", 36), 6), 6), (_decode_table(_defnorm("zo_of_defnorm", 29), 5), 5),
            (_decode_table(_defnorm("zo_ml_defnorm", 53), 6), 6)]
    if of_rle:
        oc = seqs[0][2].bit_length() - 1
        assert all(q[2].bit_length() - 1 == oc for q in seqs)
        tabs[1] = ([(oc, 0, 0)], 0)
    codes = []
    for ll, ml, ofv in seqs:
        lc, mc, oc = _code(ll, _LL_BASE), _code(ml, _ML_BASE), ofv.bit_length() - 1
        codes.append(((lc, ll - _LL_BASE[lc], _LL_BITS[lc]), (oc, ofv - (1 << oc), oc), (mc, ml - _ML_BASE[mc], _ML_BITS[mc])))
    # states, last sequence first: any state of the symbol for the last one, then the state whose range holds its successor
    states = [None] * len(seqs)
    for n in range(len(seqs) - 1, -1, -1):
        st = []
        for k in range(3):
            cells = tabs[k][0]; want = codes[n][k][0]
            if n == len(seqs) - 1: x = next(i for i, c in enumerate(cells) if c[0] == want); bits = None
            else:
                succ = states[n + 1][k][0]
                x = next(i for i, c in enumerate(cells) if c[0] == want and c[2] <= succ < c[2] + (1 << c[1]))
                bits = (succ - cells[x][2], cells[x][1])
            st.append((x, bits))
        states[n] = st
    # the fields in the order the decoder reads them (from the top of the stream down)
    reads = [(states[0][0][0], 6), (states[0][1][0], tabs[1][1]), (states[0][2][0], 6)]
    for n in range(len(seqs)):
        (_, lx, lb), (_, ox, ob), (_, mx, mb) = codes[n]
        reads += [(ox, ob), (mx, mb), (lx, lb)]
        if n + 1 < len(seqs): reads += [states[n][0][1], states[n][2][1], states[n][1][1]]      # LL, ML, OF state bits
    acc = 1
    for v, nb in reads: acc = (acc << nb) | v
    stream = acc.to_bytes((acc.bit_length() + 7) // 8, "little")
    content = bytes([len(literals) << 3]) + bytes(literals) + (bytes([len(seqs), 0x10, tabs[1][0][0][0]]) if of_rle else bytes([len(seqs), 0])) + stream
    bh = (1 if last else 0) | (2 << 1) | (len(content) << 3)
    return bh.to_bytes(3, "little") + content


def raw_block(data, last=False):
    bh = (1 if last else 0) | (len(data) << 3)
    return bh.to_bytes(3, "little") + bytes(data)


def frame(blocks, content_size):
    """magic + single-segment header with a one-byte content size + blocks"""
    assert content_size < 256
    return b"\x28\xb5\x2f\xfd" + bytes([0x20, content_size]) + b"".join(blocks)


def _hdr(fcs=None, window_log=None):
    """frame header: single-segment with the content size, or a window descriptor with / without it"""
    magic = b"\x28\xb5\x2f\xfd"
    if window_log is None:
        assert fcs is not None and fcs < 256
        return magic + bytes([0x20, fcs])
    wd = bytes([(window_log - 10) << 3])
    if fcs is None: return magic + b"\x00" + wd
    return magic + b"\x80" + wd + fcs.to_bytes(4, "little")


def rle_block(byte, n, last=True):
    return ((1 if last else 0) | (1 << 1) | (n << 3)).to_bytes(3, "little") + bytes([byte])


def edge_frames():
    """(name, frame, declared size, accepted by libzstd 1.5.7 as the reference drives it) -- what an encoder never writes but a decoder
    must answer like libzstd: zstd.c:46941 (repeat offset 1 minus one = 0), :47714 / :44239-44246 (block sizes against the frame's
    maximum in the one-pass decoder) and ZSTD_decompressContinue's stricter check when the content size is not in the header."""
    lit = b"abcdefgh"
    pat = bytes(range(256)) * 8
    out = [
        ("rep0 minus one is zero", frame([sequences_block(lit, [(8, 30, 4), (0, 3, 3)])], 41), 41, False),
        ("rep0 minus one is one", frame([sequences_block(lit, [(8, 30, 5), (0, 3, 3)])], 41), 41, True),
        ("repeat codes with empty literal runs", frame([sequences_block(lit, [(8, 30, 4), (0, 3, 2), (0, 4, 3)])], 45), 45, True),
        ("second block: rep0 minus one is zero", frame([raw_block(lit), sequences_block(b"", [(0, 3, 3)])], 11), 11, False),
        ("second block inherits history", frame([raw_block(lit), sequences_block(b"xy", [(1, 4, 2), (0, 3, 2), (1, 3, 1)])], 20), 20, True),
        ("compressed block above the frame's maximum", frame([sequences_block(lit, [(8, 3, 4)])], 11), 11, False),
        ("raw block above the window, size known", _hdr(2000, 10) + raw_block(pat[:2000], True), 2000, True),
        ("raw block above the window, size unknown", _hdr(None, 10) + raw_block(pat[:2000], True), 2000, False),
        ("RLE block above the window, size known", _hdr(2000, 10) + rle_block(7, 2000), 2000, True),
        ("RLE block above the window, size unknown", _hdr(None, 10) + rle_block(7, 2000), 2000, False),
        ("RLE block above 128 KiB, size known", _hdr(200000, 20) + rle_block(9, 200000), 200000, True),
        ("RLE block above 128 KiB, size unknown", _hdr(None, 20) + rle_block(9, 200000), 200000, False),
        ("raw block above 128 KiB, size known", _hdr(200000, 20) + raw_block((pat * 98)[:200000], True), 200000, True),
        ("raw blocks then RLE above the window", _hdr(5000, 10) + raw_block(pat[:1500]) + raw_block(pat[:1500]) + rle_block(3, 2000), 5000, True),
        # offsets the decode kernels' packed sequences cannot hold (2^29 and up): never valid in a frame this small
        ("offset codes in RLE mode", frame([sequences_block(lit, [(4, 5, 4), (4, 3, 6)], of_rle=True)], 16), 16, True),
        ("an offset of 768 MiB", frame([sequences_block(lit, [(8, 30, 0x30000003)], of_rle=True)], 38), 38, False),
        ("an offset of 3 GiB in a second block", frame([raw_block(lit), sequences_block(b"xy", [(1, 4, 0x80000007), (1, 3, 0xC0000003)], of_rle=True)], 17), 17, False),
        ("offsets around the packed form's limit", frame([sequences_block(lit, [(4, 3, 0x1E000002), (4, 3, 0x1E000003)], of_rle=True)], 14), 14, False),
    ]
    return out


def skippable_frames():
    """(name, item bytes, declared size, accepted) -- skippable frames (RFC 8878 3.1.2) as batch items: ZSTD_decompressStream passes over one
    and stops at the frame boundary with nothing produced (zstd.c:43706-43715, :44731), so the reference returns an empty segment;
    what follows the first frame of an item is never looked at (c-ext/decompressor.c:1150-1163)."""
    skip = b"\x50\x2a\x4d\x18" + (5).to_bytes(4, "little") + b"hello"
    whole = frame([sequences_block(b"abcdefgh", [(8, 30, 5), (0, 3, 3)])], 41)
    return [
        ("skippable frame", skip, 0, True),
        ("skippable frame, last magic, no payload", b"\x5f\x2a\x4d\x18" + bytes(4), 0, True),
        ("skippable frame, then a frame", skip + whole, 0, True),
        ("a frame, then a skippable frame", whole + skip, 41, True),
        ("a frame, then bytes that are no frame", whole + b"garbage!", 41, True),
        ("skippable frame, payload cut short", skip[:-2], 0, False),
        ("skippable frame, header cut short", skip[:6], 0, False),
        ("one past the skippable magics", b"\x60\x2a\x4d\x18" + skip[4:], 0, False),
    ]


def encoding_variants():
    """(name, frame, declared size, accepted) -- legal but non-minimal encodings and small illegal ones around the section headers: literal
    sizes in the longer header forms, the sequence count in its 2- and 3-byte forms, RLE-mode tables with symbols beyond the alphabets,
    reserved mode bits, degenerate block sizes, a treeless literals section with nothing to inherit. All agreed with libzstd when they were
    written (round 3); they stay as a fence."""
    magic = b"\x28\xb5\x2f\xfd"

    def blk(content, last=True): return ((1 if last else 0) | (2 << 1) | (len(content) << 3)).to_bytes(3, "little") + content

    def frm(blocks): return magic + bytes([0x00, (17 - 10) << 3]) + b"".join(blocks)
    lits = b"abcdefgh"
    seqpart = sequences_block(lits, [(8, 30, 5), (0, 3, 3)])[3:][1 + 8:]              # count, modes, stream
    rl_seq = sequences_block(b"aaaaaaaa", [(8, 30, 5), (0, 3, 3)])[3:][1 + 8:]

    def seq_rle(ll, of, ml, stream): return bytes([1, (1 << 6) | (1 << 4) | (1 << 2), ll, of, ml]) + stream
    h1 = bytes([8 << 3])
    out = [
        ("raw literals, 2-byte header", frm([blk(((8 << 4) | (1 << 2)).to_bytes(2, "little") + lits + seqpart)]), 41, True),
        ("raw literals, 3-byte header", frm([blk(((8 << 4) | (3 << 2)).to_bytes(3, "little") + lits + seqpart)]), 41, True),
        ("RLE literals, 1-byte header", frm([blk(bytes([(8 << 3) | 1]) + b"a" + rl_seq)]), 41, True),
        ("RLE literals, 2-byte header", frm([blk(((8 << 4) | (1 << 2) | 1).to_bytes(2, "little") + b"a" + rl_seq)]), 41, True),
        ("RLE literals, 3-byte header", frm([blk(((8 << 4) | (3 << 2) | 1).to_bytes(3, "little") + b"a" + rl_seq)]), 41, True),
        ("sequence count in the 2-byte form", frm([blk(h1 + lits + bytes([0x80, 2]) + seqpart[1:])]), 41, True),
        ("sequence count in the 3-byte form, far too many", frm([blk(h1 + lits + bytes([0xFF, 0x02, 0x81]) + seqpart[1:])]), 41, False),
        ("no sequences, count in the 2-byte form", frm([blk(h1 + lits + bytes([0x80, 0]))]), 8, True),
        ("no sequences but bytes after the count", frm([blk(h1 + lits + bytes([0, 0]))]), 8, False),
        ("RLE-mode tables", frm([blk(h1 + lits + seq_rle(8, 2, 0, bytes([0b100])))]), 11, True),
        ("RLE-mode literal-length symbol 36", frm([blk(h1 + lits + seq_rle(36, 2, 0, bytes([1])))]), 11, False),
        ("RLE-mode offset symbol 32", frm([blk(h1 + lits + seq_rle(8, 32, 0, bytes([1])))]), 11, False),
        ("RLE-mode match-length symbol 53", frm([blk(h1 + lits + seq_rle(8, 2, 53, bytes([1])))]), 11, False),
        ("reserved mode bits set", frm([blk(h1 + lits + bytes([2, 1]) + seqpart[2:])]), 41, False),
        ("compressed block of one byte", _hdr(0, 17) + blk(b"\x00"), 0, False),                       # (content size 0 in the header: a batch item needs one)
        ("compressed block without literals or sequences", _hdr(0, 17) + blk(b"\x00\x00"), 0, True),
        ("treeless literals with nothing to inherit", frm([blk(bytes([0x83, 0x40, 0x01]) + b"\x01\x02\x03\x04\x05" + bytes([0]))]), 8, False),
    ]
    return out


# ------------------------------------------------------------------------------------------------ frames from explicit sequences, at any size
# A frame is DESCRIBED as a list of blocks -- ("seq", literals, [(ll, ml, offset value)], options), ("raw", data), ("rle", byte, n) -- which
# tests/seqmodel.py executes in plain Python and write_frame() below turns into bytes. Nothing above this line changes (tests/golden/edge_frames.json
# pins its bytes); the writer here has no size caps: 1/2/3-byte sequence counts, each table predefined, RLE, described (a distribution written in the block) or a
# repeat of what an earlier block or a dictionary left, the last sequence's states and with them the initial states a choice, raw / RLE / Huffman literals
# (one or four streams, direct weights, treeless), every frame-header form. The bit streams are built byte by byte, in linear time.
class _Bits:
    """LSB-first bit writer; finish() appends the closing 1 bit. The format's decoders read such a stream from its end, so the fields are added in
    the REVERSE of reading order and every field's most significant bit is read first."""
    def __init__(self):
        self.out = bytearray(); self.acc = 0; self.n = 0

    def add(self, v, nb):
        self.acc |= v << self.n; self.n += nb
        while self.n >= 8:
            self.out.append(self.acc & 255); self.acc >>= 8; self.n -= 8

    def finish(self):
        self.add(1, 1)
        if self.n: self.out.append(self.acc); self.acc = 0; self.n = 0
        return bytes(self.out)


_TABS = {}


def _seq_table(kind, rle_code=None):
    """(cells, log, {symbol: [states]}) of the predefined table `kind` (0 LL, 1 OF, 2 ML), or the one-cell table of RLE mode"""
    if rle_code is not None:
        return [(rle_code, 0, 0)], 0, {rle_code: [0]}
    if kind not in _TABS:
        name, n, log = [("zo_ll_defnorm", 36, 6), ("zo_of_defnorm", 29, 5), ("zo_ml_defnorm", 53, 6)][kind]
        cells = _decode_table(_defnorm(name, n), log)
        by = {}
        for x, c in enumerate(cells): by.setdefault(c[0], []).append(x)
        _TABS[kind] = (cells, log, by)
    return _TABS[kind]


def seq_codes(ll, ml, ofv):
    """((code, extra value, extra bits) for LL, OF, ML) of one sequence"""
    lc = ll if ll < 16 else _code(ll, _LL_BASE)
    mc = ml - 3 if ml < 35 else _code(ml, _ML_BASE)
    oc = ofv.bit_length() - 1
    return (lc, ll - _LL_BASE[lc], _LL_BITS[lc]), (oc, ofv - (1 << oc), oc), (mc, ml - _ML_BASE[mc], _ML_BITS[mc])


def fse_table(norm, log):
    """(cells, log, {symbol: [states]}) of the table an FSE distribution describes (-1 = "less than one"), in the form sequences_section walks"""
    cells = _decode_table(norm, log)
    by = {}
    for x, c in enumerate(cells): by.setdefault(c[0], []).append(x)
    return cells, log, by


def described(norm, log, desc=None, walk=None):
    """mode 2 for one table of sequences_section's `modes`: the distribution `norm` at accuracy log `log` is written in the block (or `desc`, raw bytes, in
    its place) and the states walk the table it describes -- or the table of `walk` = (norm, log), for a description the stream then does not follow. A
    count of 0 is fine as long as no sequence uses that symbol."""
    return {"mode": 2, "norm": list(norm), "log": log, "desc": desc, "walk": walk}


def _state_walk(table, syms, last, first):
    """the states of one table over `syms`, walked backwards: each symbol takes the state whose range holds its successor (in a table built from a
    distribution there is exactly one). The last sequence's state is free: `last` = "first" (the lowest state of its symbol), "most" / "least" (the one
    that reads the most / fewest bits when it is reached), or a state number; `first`, a state number, asks for the choice that makes the walk START there
    (the stream's initial state). Returns (initial state, [(bits value, width)] behind every sequence but the last)."""
    cells, _, by = table
    cands = by[syms[-1]]
    if isinstance(last, int): cands = [last]; assert cells[last][0] == syms[-1]
    elif last == "most": cands = sorted(cands, key=lambda x: -cells[x][1])
    elif last == "least": cands = sorted(cands, key=lambda x: cells[x][1])
    for st in cands:
        upd = [None] * (len(syms) - 1)
        for i in range(len(syms) - 2, -1, -1):
            succ = st
            st = next(x for x in by[syms[i]] if cells[x][2] <= succ < cells[x][2] + (1 << cells[x][1]))
            upd[i] = (succ - cells[st][2], cells[st][1])
        if first is None or st == first: return st, upd
    raise AssertionError("no choice of the last state starts the walk at state %r" % (first,))


def sequences_section(seqs, modes=(0, 0, 0), count_bytes=None, inherit=None, last="first", first=(None, None, None), used=None):
    """count + modes byte + RLE symbols / descriptions + bit stream for seqs = [(ll, ml, offset value)]; modes = (LL, OF, ML), each 0 (predefined), 1 (RLE:
    every sequence then has the same code in that table), described(...) (mode 2: a distribution written in the block) or 3 (repeat: the table is
    inherit[k], a fse_table() / _seq_table() value -- with nothing to inherit only the mode bits are written and the stream walks the predefined table);
    count_bytes forces the 1-, 2- or 3-byte form of the count; last / first choose the states (_state_walk: one value, or one per table); `used`, a
    list, receives the three tables the block leaves to a later "repeat"."""
    n = len(seqs)
    if count_bytes is None: count_bytes = 1 if n < 128 else 2 if n < 0x7F00 else 3
    if count_bytes == 1: assert n < 128; head = bytes([n])
    elif count_bytes == 2: assert n < 0x7F00; head = bytes([0x80 + (n >> 8), n & 255])
    else: assert 0x7F00 <= n < 0x7F00 + 65536; head = b"\xff" + (n - 0x7F00).to_bytes(2, "little")
    if n == 0: return head
    codes = [seq_codes(*q) for q in seqs]
    tabs, bits, body, left = [], [], b"", []
    for k in range(3):
        m = modes[k]
        if isinstance(m, dict):
            bits.append(2); body += ncount(m["norm"], m["log"]) if m["desc"] is None else bytes(m["desc"])
            left.append(fse_table(m["norm"], m["log"]) if 0 < sum(abs(c) for c in m["norm"]) == 1 << m["log"] else None)
            tabs.append(fse_table(*m["walk"]) if m["walk"] else left[-1])
        elif m == 3:
            bits.append(3); left.append(inherit[k] if inherit else None); tabs.append(left[-1] or _seq_table(k))
        elif m:
            assert all(c[k][0] == codes[0][k][0] for c in codes), "RLE mode needs one code for every sequence"
            bits.append(1); body += bytes([codes[0][k][0]]); tabs.append(_seq_table(k, codes[0][k][0])); left.append(tabs[-1])
        else: bits.append(0); tabs.append(_seq_table(k)); left.append(tabs[-1])
    if used is not None: used[:] = left
    head += bytes([(bits[0] << 6) | (bits[1] << 4) | (bits[2] << 2)]) + body
    # walk backwards: the last sequence takes any state of its symbols; each earlier one the state of its symbol whose range holds its successor.
    # Fields in reading order per sequence: OF, ML, LL extra bits, then (not after the last) LL, ML, OF state bits -- added here in reverse.
    lasts = last if isinstance(last, (tuple, list)) else (last,) * 3
    walks = [_state_walk(tabs[k], [c[k][0] for c in codes], lasts[k], first[k]) for k in range(3)]
    w = _Bits()
    for i in range(n - 1, -1, -1):
        (_, lx, lb), (_, ox, ob), (_, mx, mb) = codes[i]
        if i < n - 1:
            w.add(*walks[1][1][i]); w.add(*walks[2][1][i]); w.add(*walks[0][1][i])
        w.add(lx, lb); w.add(mx, mb); w.add(ox, ob)
    w.add(walks[2][0], tabs[2][1]); w.add(walks[1][0], tabs[1][1]); w.add(walks[0][0], tabs[0][1])
    return head + w.finish()


def ncount(norm, log):
    """An FSE distribution as the format writes it (RFC 8878 4.1.1): the accuracy log, then every count in its variable width with the zero-run
    flags, up to the symbol that completes the total (a list that stays below 2^log ends where it ends: the reader goes on into what follows)"""
    w = _Bits()
    w.add(log - 5, 4)
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    s = 0
    while s < len(norm) and remaining > 1:
        c = norm[s]; s += 1
        v, mx = c + 1, 2 * threshold - 1 - remaining
        assert 0 <= v <= remaining, "a count above what is left cannot be written"
        if v < mx: w.add(v, nb - 1)
        elif v < threshold: w.add(v, nb)
        else: w.add(v + mx, nb)
        remaining -= abs(c)
        while 1 <= remaining < threshold: nb -= 1; threshold >>= 1
        if c == 0 and remaining > 1 and s < len(norm):
            run = 0
            while s < len(norm) and norm[s] == 0: run += 1; s += 1
            for _ in range(run // 3): w.add(3, 2)
            w.add(run % 3, 2)
    if w.n: w.out.append(w.acc)
    return bytes(w.out)


def fit_norm(ws, log):
    """a normalised distribution over the weights in `ws` that totals 2^log: every weight present gets at least one cell, the most frequent one the rest"""
    size, cnt = 1 << log, [0] * (max(ws) + 1)
    for x in ws: cnt[x] += 1
    norm = [max(1, c * size // len(ws)) if c else 0 for c in cnt]
    top = max(range(len(cnt)), key=lambda i: cnt[i])
    while sum(norm) > size:
        big = max(range(len(norm)), key=lambda i: norm[i]); norm[big] -= 1
    norm[top] += size - sum(norm)
    if norm[top] == size:                                                       # one weight value alone: no state would read a bit and the stream never end
        if len(norm) == 1: norm.append(0)
        norm[top] -= 1; norm[1 if top == 0 else 0] = 1
    assert all(n > 0 for n, c in zip(norm, cnt) if c) and sum(norm) == size
    return norm


def fse_weights(ws, log, norm, report=None):
    """distribution + the two-state backward bit stream of the weights `ws`. The decoder gives weight 0, 2, 4 ... from its first state and 1, 3, 5 ...
    from its second, and ends when a state update asks for more bits than are left: the weight just given and one more from the OTHER state are
    the last two. So the stream holds the updates behind the weights 0 .. n - 3 and not one bit more, and the state that gives weight n - 2 is one
    whose update reads at least one bit. Walked backwards: each weight takes the state of its symbol whose range holds the state two weights on."""
    n = len(ws)
    assert n >= 2
    cells = _decode_table(norm, log)
    by = {}
    for x, c in enumerate(cells): by.setdefault(c[0], []).append(x)
    st = [None] * n
    st[n - 1] = by[ws[n - 1]][0]
    st[n - 2] = next(x for x in by[ws[n - 2]] if cells[x][1] >= 1)
    w = _Bits()
    for i in range(n - 3, -1, -1):
        succ = st[i + 2]
        x = next(x for x in by[ws[i]] if cells[x][2] <= succ < cells[x][2] + (1 << cells[x][1]))
        w.add(succ - cells[x][2], cells[x][1]); st[i] = x
    w.add(st[1], log); w.add(st[0], log)
    body = ncount(norm, log) + w.finish()
    if report is not None:
        report.update({"weights": n, "exit": 3 if n > 255 else 1 if n % 2 == 0 else 2, "bytes": len(body)})
    return body


class HufTable:
    """A canonical Huffman code of the format (RFC 8878 4.2.1) over the byte values in `data` (all <= 128, so the weights fit the direct form;
    at least two different values), code lengths capped at 11 bits. nbits[s] / code[s] per symbol; description() is the tree as direct weights."""
    def __init__(self, data):
        import heapq
        freq = {}
        for b in data: freq[b] = freq.get(b, 0) + 1
        assert len(freq) >= 2 and max(freq) <= 128
        while True:
            heap = [(f, s, (s,)) for s, f in freq.items()]
            heapq.heapify(heap)
            depth = dict.fromkeys(freq, 0)
            while len(heap) > 1:
                fa, sa, ma = heapq.heappop(heap); fb, sb, mb = heapq.heappop(heap)
                for s in ma + mb: depth[s] += 1
                heapq.heappush(heap, (fa + fb, min(sa, sb), ma + mb))
            if max(depth.values()) <= 11: break
            freq = {s: (f >> 1) + 1 for s, f in freq.items()}                 # flatter counts give a flatter tree
        self.max_bits = mb_ = max(depth.values())
        self.weights = [mb_ + 1 - depth[s] if s in depth else 0 for s in range(max(freq) + 1)]
        self.nbits, self.code, pos = {}, {}, 0
        for w in range(1, mb_ + 1):                                             # lowest weight (longest code) first, symbols in natural order
            for s, ws in enumerate(self.weights):
                if ws == w: self.nbits[s] = mb_ + 1 - w; self.code[s] = pos >> (w - 1); pos += 1 << (w - 1)
        assert pos == 1 << mb_

    @classmethod
    def from_weights(cls, weights, valid=True):
        """The canonical code of an explicit weight list: weights[s] for the symbols 0 .. len - 1 (any of 0 .. 255), zero = the symbol is absent, table log
        1 .. 12. valid=True: the list is the whole alphabet -- its last weight is the one the format leaves implied and must be what completes the
        sum to a power of two. valid=False: `weights` are the WRITTEN weights as they stand (nothing implied, nothing checked): a list to be
        described, not to encode with."""
        t = cls.__new__(cls)
        t.weights = list(weights)
        t.written = t.weights[:-1] if valid else t.weights
        t.nbits, t.code, t.max_bits = {}, {}, None
        if not valid: return t
        assert 2 <= len(t.weights) <= 256 and t.weights[-1] > 0 and all(0 <= w <= 12 for w in t.weights)
        total = sum(1 << (w - 1) for w in t.weights if w)
        assert total & (total - 1) == 0 and total >= 2, "the weights do not complete to a power of two"
        t.max_bits = mb_ = total.bit_length() - 1
        assert any(t.written), "no weight in front of the implied one"        # (the reader takes the log from the written sum: always the list's own)
        pos = 0
        for w in range(1, mb_ + 1):
            for s, ws in enumerate(t.weights):
                if ws == w: t.nbits[s] = mb_ + 1 - w; t.code[s] = pos >> (w - 1); pos += 1 << (w - 1)
        assert pos == 1 << mb_
        return t

    def description(self, form="direct", accuracy_log=6, norm=None, report=None):
        """The tree description. form "direct": 4-bit weights (at most 128 of them). form "fse": the weights FSE-compressed (RFC 8878 4.2.1.2) on the
        normalised distribution `norm` over the weights 0 .. len(norm) - 1 (-1 = "less than one"; default: one fitted to the list) at `accuracy_log`
        (5 or 6); `report`, a dict, receives "weights" (how many the stream carries), "exit" (which of the decoder's ends it takes: 1 = the stream
        runs out behind a weight of the first state, 2 = of the second, 3 = the list is too long and the decoder gives up first) and "bytes"."""
        ws = getattr(self, "written", self.weights[:-1])                        # the last symbol's weight is implied
        if form == "direct":
            assert 1 <= len(ws) <= 128
            pad = ws + [0] * (len(ws) & 1)
            return bytes([127 + len(ws)]) + bytes((pad[i] << 4) | pad[i + 1] for i in range(0, len(pad), 2))
        if norm is None: norm = fit_norm(ws, accuracy_log)
        body = fse_weights(ws, accuracy_log, norm, report)
        assert len(body) < 128, "an FSE description has at most 127 bytes (%d)" % len(body)
        return bytes([len(body)]) + body

    def stream(self, data):
        w = _Bits()
        for b in reversed(data): w.add(self.code[b], self.nbits[b])
        return w.finish()


def literals_section(lits, mode="raw", hdr=None, table=None, desc=None, jump=None, mangle=None, claim=None, size_format=None):
    """The literals section of `lits`. mode: "raw" / "rle" (hdr = 1, 2 or 3 header bytes, default the shortest), "huf1" / "huf4" (Huffman with `table`
    written in front, one or four streams) or "treeless1" / "treeless4" (the previous block's table, `table`, not written).
    Huffman sections from explicit choices: desc = the description's bytes instead of table.description(); four streams of 6 literals and up (the
    fourth stream is then empty: its end mark alone); jump = the three sizes of the jump table as written; mangle = a function from the list of
    stream byte strings to the list to write; claim = the literal count the header states; size_format = 1 / 2 / 3 forces the 10- / 14- / 18-bit
    sizes of the four-stream header."""
    n = len(lits)
    if mode in ("raw", "rle"):
        t = 0 if mode == "raw" else 1
        if mode == "rle": assert n > 0 and lits == lits[:1] * n
        if hdr is None: hdr = 1 if n < 32 else 2 if n < 4096 else 3
        if hdr == 1: assert n < 32; h = bytes([(n << 3) | t])
        elif hdr == 2: assert n < 4096; h = ((n << 4) | (1 << 2) | t).to_bytes(2, "little")
        else: assert n < (1 << 20); h = ((n << 4) | (3 << 2) | t).to_bytes(3, "little")
        return h + (bytes(lits) if mode == "raw" else bytes(lits[:1]))
    t = 2 if mode.startswith("huf") else 3
    body = (table.description() if desc is None else desc) if t == 2 else b""
    said = n if claim is None else claim
    if mode.endswith("1"):
        parts = [table.stream(lits)]
        if mangle: parts = mangle(parts)
        body += parts[0]
        assert said < 1024 and len(body) < 1024
        return (t | (0 << 2) | (said << 4) | (len(body) << 14)).to_bytes(3, "little") + body
    q = (n + 3) // 4
    parts = [table.stream(lits[i * q:(i + 1) * q]) for i in range(3)] + [table.stream(lits[3 * q:])]
    assert n >= 3 * q and n >= 6 and all(len(p) < 65536 for p in parts[:3])
    if mangle: parts = mangle(parts)
    sizes = [len(p) for p in parts[:3]] if jump is None else list(jump)
    body += b"".join(x.to_bytes(2, "little") for x in sizes) + b"".join(parts)
    for sf, bits, size in ((1, 10, 3), (2, 14, 4), (3, 18, 5)):
        if size_format not in (None, sf): continue
        if said < (1 << bits) and len(body) < (1 << bits):
            return (t | (sf << 2) | (said << 4) | (len(body) << (4 + bits))).to_bytes(size, "little") + body
    raise AssertionError("literals too large")


def block(kind, content, last):
    """3-byte block header + content; kind 0 raw, 1 RLE (content = the byte, size given as a pair (byte, n)), 2 compressed"""
    if kind == 1:
        byte, n = content
        return ((1 if last else 0) | (1 << 1) | (n << 3)).to_bytes(3, "little") + bytes([byte])
    assert len(content) < (1 << 21)
    return ((1 if last else 0) | (kind << 1) | (len(content) << 3)).to_bytes(3, "little") + bytes(content)


def frame_header(fcs=None, single_segment=False, window_log=17, dict_id=None, checksum=False, fcs_bytes=None):
    """magic + frame header: single-segment (needs fcs) or a window descriptor; fcs None = no content size; dict_id None = no field;
    fcs_bytes forces the width of the content-size field (1 only with single_segment, 2, 4 or 8)"""
    fhd = (0x20 if single_segment else 0) | (4 if checksum else 0)
    tail = b""
    if not single_segment: tail += bytes([(window_log - 10) << 3])
    else: assert fcs is not None
    if dict_id is not None:
        nb = 1 if dict_id < 256 else 2 if dict_id < 65536 else 4
        fhd |= {1: 1, 2: 2, 4: 3}[nb]; tail += dict_id.to_bytes(nb, "little")
    if fcs is not None:
        if fcs_bytes is None: fcs_bytes = 1 if single_segment and fcs < 256 else 2 if 256 <= fcs < 65536 + 256 else 4 if fcs < (1 << 32) else 8
        if fcs_bytes == 1: assert single_segment and fcs < 256
        if fcs_bytes == 2: assert 256 <= fcs < 65536 + 256
        fhd |= {1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes] << 6
        tail += (fcs - 256 if fcs_bytes == 2 else fcs).to_bytes(fcs_bytes, "little")
    return b"\x28\xb5\x2f\xfd" + bytes([fhd]) + tail


def write_frame(blocks, fcs="auto", content=None, checksum=None, dict_tables=None, **header):
    """A frame of `blocks`: ("seq", literals, seqs, options) / ("raw", data) / ("rle", byte, n). A "seq" block's options: lit = the literals mode
    of literals_section (default "raw"), lit_hdr, modes, count_bytes; Huffman tables are built per block ("huf*") and inherited ("treeless*"), or
    explicit: huf_table (a HufTable, e.g. from_weights), huf_desc (the description's bytes), jump, mangle, claim, size_format (literals_section).
    fcs "auto" declares len(content); checksum = the 32-bit trailer to write (the caller computes it: Oracle.xxh64(content) & 0xFFFFFFFF, or a
    wrong one); other keywords go to frame_header. Sequence tables: a block's `modes` may hold described(...) and 3 (sequences_section); a "repeat"
    inherits what the last block WITH sequences left, whatever its modes were, and the first such block what dict_tables gives (a dictionary's three
    tables, or None: nothing to inherit); seq_last / seq_first choose the states (sequences_section's last / first); seq_mangle = a function from the sequences section's bytes to the bytes to write (a block cut short, a stream damaged)."""
    if fcs == "auto": fcs = len(content)
    out = [frame_header(fcs=fcs, checksum=checksum is not None, **header)]
    table, seq_tabs = None, dict_tables
    for i, b in enumerate(blocks):
        last = i == len(blocks) - 1
        if b[0] == "raw": out.append(block(0, b[1], last))
        elif b[0] == "rle": out.append(block(1, (b[1], b[2]), last))
        else:
            lits, seqs = bytes(b[1]), b[2]
            o = b[3] if len(b) > 3 else {}
            mode = o.get("lit", "raw")
            if "huf_table" in o: table = o["huf_table"]                        # (with a treeless mode: the table the block inherits, a dictionary's)
            elif mode.startswith("huf"): table = HufTable(o.get("huf_from", lits))
            left = []
            sec = sequences_section(seqs, o.get("modes", (0, 0, 0)), o.get("count_bytes"), seq_tabs, o.get("seq_last", "first"), o.get("seq_first", (None, None, None)), left)
            if seqs: seq_tabs = left
            if "seq_mangle" in o: sec = o["seq_mangle"](sec)
            body = literals_section(lits, mode, o.get("lit_hdr"), table, o.get("huf_desc"), o.get("jump"), o.get("mangle"), o.get("claim"), o.get("size_format")) + sec
            out.append(block(2, body, last))
    if checksum is not None: out.append((checksum & 0xFFFFFFFF).to_bytes(4, "little"))
    return b"".join(out)
