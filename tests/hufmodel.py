"""What the Huffman side of a frame decodes to, in plain Python from RFC 8878 (test infrastructure).

* read_description(): a tree description in either form -- 4-bit weights, or weights FSE-compressed (4.2.1.2: a distribution, its decoding
  table, two interleaved states over a backward bit stream that ends when a state update over-reads) -- with the checks of 4.2.1.1: no weight
  above 12, the sum completing to a power of two of at most 2^12, an even number, at least two, of weights 1.
* build_table() / decode_stream(): the canonical code (4.2.1.3) as a lookup table of 2^log cells, one backward stream decoded symbol by symbol.
  A stream must be consumed EXACTLY -- the rule DESIGN.md section 2 keeps stricter than libzstd, whose four-stream fast loop only checks the
  produced length: the one reason this model may refuse where libzstd decodes, "a stream not consumed exactly". A literal stream whose last
  byte is 0 falls under it only where that fast loop runs (four streams of 8 bytes and more each: it decodes the 160 literals of
  huffamilies' 11-bit table behind one); everywhere else it is "a stream: no end mark" and libzstd's careful loop must refuse it too.
* literals() walks a frame's blocks and returns each compressed block's literals, or raises Refused(reason). It is the expected value of
  tests/test_emu_huffman_tables.py and tests/test_gpu_huffman_tables.py; libzstd 1.5.7 is asked about every frame first (check_model), and a
  disagreement is reported as THIS MODEL's fault.
* census() names what a frame reaches in the decoders (table logs, description forms, the FSE decode's exits, stream sizes against K1b's
  64-byte ring, start alignments, the 8-symbol trip's tails ...). It is used only to assert coverage, never for expected bytes.

Nothing here is shared with the writer (tests/craft.py): the FSE table below is built from the format's text a second time on purpose."""
import struct

LOG_MAX = 12                     # the format's largest Huffman table log
RING = 64                        # K1b's ring (ZP_HUF_RING dwords): census only
DEEP = 11                        # ZP_HUF_LOGMAX: tables above it are decoded inside K1 (census only; pinned against the header by the tests)
INEXACT = "a stream not consumed exactly"


class Refused(Exception):
    def __init__(self, reason):
        Exception.__init__(self, reason); self.reason = reason


class _Back:
    """a backward bit stream: bits are read from the top, below the end mark; reading past the first byte gives zeros and a negative `left`"""
    def __init__(self, data, what):
        if len(data) == 0: raise Refused("%s: empty" % what)
        if data[-1] == 0: raise Refused("%s: no end mark" % what)
        self.v = int.from_bytes(data, "little")
        self.left = self.v.bit_length() - 1

    def peek(self, n):
        lo = self.left - n
        return ((self.v >> lo) if lo >= 0 else (self.v << -lo)) & ((1 << n) - 1)

    def read(self, n):
        x = self.peek(n) if n else 0
        self.left -= n
        return x


def read_ncount(buf, max_symbol=255):
    """an FSE distribution (4.1.1) -> (counts with -1 for "less than one", accuracy log, bytes used)"""
    if len(buf) == 0: raise Refused("distribution: nothing to read")
    v, pos = int.from_bytes(buf, "little"), 4
    log = (v & 15) + 5
    if log > 15: raise Refused("distribution: accuracy log above 15")
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    norm, prev0 = [], False
    while remaining > 1 and len(norm) <= max_symbol:
        if prev0:
            while True:
                r = (v >> pos) & 3; pos += 2
                norm += [0] * r
                if r != 3: break
                if pos > 8 * len(buf): raise Refused("distribution: runs past the description")
            if len(norm) > max_symbol: raise Refused("distribution: a symbol above the alphabet")
        mx = 2 * threshold - 1 - remaining
        low = (v >> pos) & ((1 << (nb - 1)) - 1)
        if low < mx: count = low; pos += nb - 1
        else:
            count = (v >> pos) & ((1 << nb) - 1)
            if count >= threshold: count -= mx
            pos += nb
        count -= 1
        remaining -= abs(count)
        if remaining < 1: raise Refused("distribution: counts above 2^log")
        norm.append(count); prev0 = count == 0
        while remaining < threshold: nb -= 1; threshold >>= 1
        if (pos + 7) // 8 > len(buf): raise Refused("distribution: runs past the description")
    if remaining != 1: raise Refused("distribution: does not total 2^log")
    return norm, log, (pos + 7) // 8


def fse_table(norm, log):
    """[(symbol, bits to read, base of the next state)] per state (4.1.1: "less than one" symbols from the top, the spread walk, states in order)"""
    size = 1 << log
    sym, high = [None] * size, size - 1
    for s, c in enumerate(norm):
        if c == -1: sym[high] = s; high -= 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) % size
            while pos > high: pos = (pos + step) % size
    if pos != 0: raise Refused("distribution: the spread does not close")
    nxt = [1 if c == -1 else c for c in norm]
    cells = []
    for x in range(size):
        s = sym[x]; n = nxt[s]; nxt[s] += 1
        nb = log - (n.bit_length() - 1)
        cells.append((s, nb, (n << nb) - size))
    return cells


def fse_weights(buf, info=None):
    """the FSE-compressed weights of a description's `buf` (the bytes behind the size byte) -> the written weights"""
    norm, log, used = read_ncount(buf)
    if log > 6: raise Refused("weights: accuracy log above 6")
    # (not the RFC's but libzstd's: it decodes the weights in a work area sized for log 6 and the weights 0 .. 11 -- HUF_READ_STATS_WORKSPACE_SIZE, counted
    # in 4-byte units -- and refuses a distribution that needs more: at log 6 one that names weight 12, at log 5 one that names a symbol above 91)
    if (1 << log) + (2 * len(norm) + (1 << log) + 8 + 3) // 4 > 64 + 24: raise Refused("weights: a distribution above libzstd's work area")
    cells = fse_table(norm, log)
    b = _Back(buf[used:], "weights' bit stream")
    s1 = b.read(log); s2 = b.read(log)
    out, ends = [], None
    while True:
        if len(out) > 253: ends = 3; break
        sym, nb, base = cells[s1]; out.append(sym)
        s1 = base + b.read(nb)
        if b.left < 0: out.append(cells[s2][0]); ends = 1; break
        if len(out) > 253: ends = 3; break
        sym, nb, base = cells[s2]; out.append(sym)
        s2 = base + b.read(nb)
        if b.left < 0: out.append(cells[s1][0]); ends = 2; break
    if info is not None: info.update({"form": "fse", "accuracy_log": log, "exit": ends, "bytes": len(buf), "written": len(out), "norm": norm})
    if ends == 3: raise Refused("weights: more than 255 of them")
    return out


def complete(written):
    """the written weights -> (all weights, the implied last one included; table log), after 4.2.1.1's checks"""
    if any(w > LOG_MAX for w in written): raise Refused("weights: one above 12")
    total = sum(1 << (w - 1) for w in written if w)
    if total == 0: raise Refused("weights: all zero")
    log = total.bit_length()
    if log > LOG_MAX: raise Refused("weights: a sum that needs a table log above 12")
    rest = (1 << log) - total
    if rest & (rest - 1): raise Refused("weights: the sum does not complete to a power of two")
    last = rest.bit_length()
    ones = sum(w == 1 for w in written) + (last == 1)
    if ones < 2 or ones & 1: raise Refused("weights: %s weights of 1" % ("fewer than two" if ones < 2 else "an odd number of"))
    return list(written) + [last], log


def read_description(buf, info=None):
    """a tree description at the start of `buf` -> (weights of the symbols 0 .. n - 1, table log, bytes used)"""
    if len(buf) == 0: raise Refused("description: nothing to read")
    hb = buf[0]
    if hb >= 128:
        n = hb - 127; used = 1 + (n + 1) // 2
        if used > len(buf): raise Refused("description: runs past the section")
        written = [(buf[1 + i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(n)]
        if info is not None: info.update({"form": "direct", "written": n})
    else:
        used = 1 + hb
        if used > len(buf): raise Refused("description: runs past the section")
        if info is not None: info.update({"form": "fse", "bytes": hb})
        if hb < 2: raise Refused("description: an FSE form below two bytes")
        written = fse_weights(buf[1:used], info)
    weights, log = complete(written)
    if info is not None: info.update({"log": log, "weights": weights})
    return weights, log, used


def build_table(weights):
    """[(symbol, code length)] x 2^log: lowest weight first, symbols in natural order inside a weight (4.2.1.3)"""
    total = sum(1 << (w - 1) for w in weights if w)
    log = total.bit_length() - 1
    assert total == 1 << log and 1 <= log <= LOG_MAX
    table = []
    for w in range(1, log + 1):
        for s, ws in enumerate(weights):
            if ws == w: table += [(s, log + 1 - w)] * (1 << (w - 1))
    assert len(table) == 1 << log
    return table, log


def decode_stream(table, log, data, count, careful=True):
    # A last byte of 0 -- no end mark, so nothing says where the bits to consume begin. libzstd's careful loop refuses such a stream; its fast four-stream loop --
    # taken when every one of the four streams has 8 bytes and more (`careful` False) -- decodes behind it. Only there is it reported as inexact consumption,
    # the one class where this model may be stricter than libzstd; everywhere else it keeps its own name and libzstd must refuse it too (check_model).
    if len(data) and data[-1] == 0 and not careful: raise Refused(INEXACT)
    b = _Back(data, "a stream")
    out = bytearray()
    for _ in range(count):
        sym, nb = table[b.peek(log)]
        b.left -= nb
        if b.left < 0: raise Refused(INEXACT)
        out.append(sym)
    if b.left != 0: raise Refused(INEXACT)
    return bytes(out)


def literals_section(buf, prev, block_max=131072, info=None):
    """the literals section at the start of a block's content `buf`; prev = the weights a treeless section inherits (or None).
    -> (literals, bytes used, the weights later blocks inherit)"""
    if len(buf) < 1: raise Refused("literals: nothing to read")
    t, fmt = buf[0] & 3, (buf[0] >> 2) & 3
    if t < 2:
        if fmt == 1: hdr, regen = 2, int.from_bytes(buf[:2], "little") >> 4
        elif fmt == 3: hdr, regen = 3, int.from_bytes(buf[:3], "little") >> 4
        else: hdr, regen = 1, buf[0] >> 3
        if len(buf) < hdr or regen > block_max: raise Refused("literals: size")
        if t == 0:
            if hdr + regen > len(buf): raise Refused("literals: raw bytes past the block")
            if info is not None: info["kind"] = "raw"
            return bytes(buf[hdr:hdr + regen]), hdr + regen, prev
        if hdr + 1 > len(buf): raise Refused("literals: no RLE byte")
        if info is not None: info["kind"] = "rle"
        return bytes(buf[hdr:hdr + 1]) * regen, hdr + 1, prev
    if len(buf) < 5: raise Refused("literals: a compressed section below five bytes")
    v = int.from_bytes(buf[:5], "little")
    if fmt < 2: hdr, four, regen, csize, bits = 3, fmt, (v >> 4) & 0x3FF, (v >> 14) & 0x3FF, 10
    elif fmt == 2: hdr, four, regen, csize, bits = 4, 1, (v >> 4) & 0x3FFF, (v >> 18) & 0x3FFF, 14
    else: hdr, four, regen, csize, bits = 5, 1, (v >> 4) & 0x3FFFF, (v >> 22) & 0x3FFFF, 18
    if regen > block_max: raise Refused("literals: more than the block maximum")
    if (regen < 6) if four else (regen == 0): raise Refused("literals: too few for the stream count")
    if hdr + csize > len(buf): raise Refused("literals: section past the block")
    body = buf[hdr:hdr + csize]
    d = {}
    if t == 3:
        if prev is None: raise Refused("literals: treeless with nothing to inherit")
        weights, used = prev, 0
    else:
        weights, _, used = read_description(body, d)
    table, log = build_table(weights)
    streams = body[used:]
    if info is not None:
        info.update({"kind": "huf" if t == 2 else "treeless", "four": four, "bits": bits, "regen": regen, "log": log, "desc": d, "weights": weights,
                     "stream_off": hdr + used, "streams": []})
    if not four:
        if info is not None: info["streams"].append((hdr + used, len(streams), regen))
        return decode_stream(table, log, streams, regen), hdr + csize, weights
    if len(streams) < 10: raise Refused("literals: four streams in fewer than ten bytes")
    s1, s2, s3 = struct.unpack("<3H", streams[:6])
    if 6 + s1 + s2 + s3 > len(streams): raise Refused("literals: the jump table runs past the section")
    seg = (regen + 3) // 4
    if 3 * seg > regen: raise Refused("literals: too few for four streams")
    sizes = [s1, s2, s3, len(streams) - 6 - s1 - s2 - s3]
    counts = [seg, seg, seg, regen - 3 * seg]
    if 0 in sizes: raise Refused("a stream: empty")
    out, at, first = b"", 6, None
    for k in range(4):
        if info is not None: info["streams"].append((hdr + used + at, sizes[k], counts[k]))
        try: out += decode_stream(table, log, streams[at:at + sizes[k]], counts[k], careful=min(sizes) < 8)
        except Refused as e: first = first or e
        at += sizes[k]
    if first: raise first
    return out, hdr + csize, weights


def dictionary_weights(dict_data):
    """the Huffman weights of a trained dictionary and where its description ends, or (None, 0) for raw content"""
    if not dict_data or len(dict_data) < 8 or dict_data[:4] != b"\x37\xa4\x30\xec": return None, 0
    weights, _, used = read_description(dict_data[8:])
    return weights, 8 + used


def walk(frame):
    """(block type, content offset, content size, last) per block of `frame`; raises Refused for a header this model does not know"""
    if frame[:4] != b"\x28\xb5\x2f\xfd": raise Refused("frame: magic")
    fhd = frame[4]
    pos = 5 + (0 if fhd & 0x20 else 1) + (0, 1, 2, 4)[fhd & 3]
    fcs = fhd >> 6
    pos += (1 if fhd & 0x20 else 0, 2, 4, 8)[fcs]
    out = []
    while True:
        if pos + 3 > len(frame): raise Refused("frame: block header past the end")
        bh = int.from_bytes(frame[pos:pos + 3], "little"); pos += 3
        t, size = (bh >> 1) & 3, bh >> 3
        body = 1 if t == 1 else size
        if pos + body > len(frame): raise Refused("frame: block past the end")
        out.append((t, pos, size, bh & 1))
        pos += body
        if bh & 1: return out


def literals(frame, dict_data=None, infos=None):
    """the literals of every compressed block of `frame`, in order; raises Refused(reason) for the first section that must be refused"""
    prev, _ = dictionary_weights(dict_data)
    out = []
    for t, pos, size, _ in walk(frame):
        if t != 2: continue
        info = {"at": pos}
        if infos is not None: infos.append(info)
        lits, _, prev = literals_section(frame[pos:pos + size], prev, info=info)
        out.append(lits)
    return out


def check_model(ref, frame, want, cap, why, dict_data=None, stricter_allowed=False):
    """libzstd's verdict on `frame` against this model's (`want`: bytes, or None with the reason `why`). A disagreement is a failure of the MODEL,
    raised as such before any kernel is looked at -- but for the one documented class: the model refuses with "a stream not consumed exactly",
    libzstd decodes something, and the caller says the frame belongs to the damaged-stream family (stricter_allowed). Returns True for that class."""
    try:
        got = ref.decompress_advanced(frame, cap, dict_data=dict_data) if dict_data else ref.decompress(frame, cap)
        if dict_data is not None and len(got) != cap: got = None
    except RuntimeError:
        got = None
    if got == want: return False
    if want is None and got is not None and why == INEXACT and stricter_allowed: return True
    raise AssertionError("TEST MODEL, not a kernel: hufmodel and libzstd disagree (libzstd %s, the model %s)" % (
        "refuses" if got is None else "%d bytes" % len(got), "refuses: %s" % why if want is None else "%d bytes" % len(want)))


def census(frame, dict_data=None, base=0):
    """the set of named things `frame`, lying at absolute offset `base` of its arena, reaches in the Huffman decoders. Coverage only."""
    ev, infos = set(), []
    try: literals(frame, dict_data, infos)
    except Refused as e: ev.add("refused: " + e.reason)
    blocks = sum(1 for b in walk(frame))
    seen_deep, prev_log, prev_kind = False, None, None
    if dictionary_weights(dict_data)[0]:
        prev_log = build_table(dictionary_weights(dict_data)[0])[1]; prev_kind = "dictionary"
        ev.add("dictionary table log %d" % prev_log)
    for t, pos, size, _ in walk(frame):
        if t != 2:
            if prev_kind == "huf": prev_kind = "huf, then another block type"
            continue
        i = next((x for x in infos if x["at"] == pos), None)
        if i is None or "log" not in i: break
        if i["kind"] in ("raw", "rle"):
            if prev_kind in ("huf", "treeless"): prev_kind = "huf, then another block type"
            continue
        log, d, w = i["log"], i["desc"], i["weights"]
        if i["kind"] == "huf":
            ev.add("table log %d" % log)
            if log > DEEP: ev.add("table above K1b's slots" + (" in a frame of several blocks" if blocks > 1 else ""))
            if prev_log is not None and prev_kind != "dictionary": ev.add("a new table of log %d after one of log %d" % (log, prev_log))
            ev.add("description: %s" % d["form"])
            n = len(w) - 1
            if d["form"] == "direct": ev.add("direct weights: %s" % (n if n in (1, 2, 127, 128) else "odd" if n & 1 else "even"))
            else:
                ev.add("FSE accuracy log %d" % d["accuracy_log"]); ev.add("FSE decode ends through exit %d" % d["exit"])
                ev.add("FSE weights: %s" % (n if n >= 253 else "below 253"))
                ev.add("FSE description of %s bytes" % (d["bytes"] if d["bytes"] in (2, 3, 126, 127) else "4..125"))
                if -1 in d["norm"]: ev.add("FSE distribution with a 'less than one' count")
                if blocks == 1: ev.add("FSE description in a frame of one block")
                else: ev.add("FSE description in a frame of several blocks")
            for lo in (64, 128, 192):
                if any(x for x in w[lo:lo + 64]): ev.add("symbols in %d..%d" % (lo, lo + 63))
            if len(w) == 256: ev.add("symbol 255")
            if len(w) == 2: ev.add("two symbols")
            if any(x == 0 for x in w): ev.add("zero-weight gaps")
            if any(x in (1, 2) for x in w): ev.add("cells written one at a time (weights 1 and 2)")
            if any(x >= 3 for x in w): ev.add("cells written eight bytes at a time (weights 3 and up)")
            ev.add("implied last weight %d of log %d" % (w[-1], log))
            if w[-1] == log: ev.add("implied last weight equal to the log")
        else:
            ev.add("treeless, %s" % ("four streams" if i["four"] else "one stream"))
            ev.add("treeless after %s, log %d" % (prev_kind, log))
            if log > DEEP and blocks > 1 and prev_kind != "dictionary": ev.add("treeless block rebuilds a table above K1b's slots")
        ev.add("four streams" if i["four"] else "one stream")
        ev.add("size format of %d bits" % i["bits"])
        lens = set(build_table(w)[0][k][1] for k in range(1 << log))
        for off, nbytes, count in i["streams"]:
            ev.add("stream start at %d mod 16" % ((base + pos + off) % 16))
            ev.add("stream of %s bytes" % (nbytes if nbytes <= 80 else "81..199" if nbytes < 200 else "200 and up"))
            ev.add("stream %s the ring" % ("below" if nbytes < RING else "at" if nbytes == RING else "above"))
            ev.add("trip tail %d" % (count % 8))
            if count < 8: ev.add("stream of %d symbols" % count)
            if count == 0: ev.add("empty fourth stream")
            if i["four"]: ev.add("four streams of %s literals" % (i["regen"] if i["regen"] in (6, 7, 8, 9, 1023) else "other"))
            if nbytes > RING and count and 8 * nbytes >= log * count and log >= DEEP: ev.add("a stream of longest codes above the ring")
        prev_log, prev_kind = log, i["kind"] if i["kind"] == "huf" else prev_kind
        if i["kind"] == "treeless" and prev_kind == "huf, then another block type": prev_kind = "huf"
    return ev
