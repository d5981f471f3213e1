"""What the sequences side of a frame decodes to when its three FSE tables are EXPLICIT choices, in plain Python from RFC 8878 (test infrastructure).

* read_table(): one table description (4.1.1) under the limits of 3.1.1.3.2.1 -- accuracy logs 9 / 8 / 9, alphabets 35 / 31 / 52, the total, the
  zero-run rules, a description that runs past the block's end. The distribution reader and the table builder are tests/hufmodel.py's (read_ncount,
  fse_table: written from the format's text a second time, nothing shared with tests/craft.py's writer).
* sequences(): a whole frame -- every block's literals (hufmodel.literals_section), the sequence count, the modes byte, each table in its mode
  (predefined / RLE / described / repeat), the three interleaved states over the backward bit stream -- to the block list seqmodel.execute takes.
  The repeat rules are libzstd 1.5.7's: "repeat" takes what the last block WITH sequences used, whatever its mode was; a block without sequences, a
  raw block and an RLE block change nothing; a frame's first block with sequences has nothing to repeat unless a (trained) dictionary gave it tables.
  The bit stream must be consumed exactly.
* decode(): the verdict and, for an accepted frame, the content through seqmodel.execute. It is the expected value of
  tests/test_emu_sequence_tables.py and tests/test_gpu_sequence_tables.py; libzstd is asked about every frame first (seqmodel.check_model) and a
  disagreement is reported as THIS MODEL's fault. No "stricter" class exists here: verdict and bytes equal libzstd's on every case.
* census(): what a frame reaches in zd_read_ncount_to / zd_build_fse / zp_pack_fse / zd_seq_table / K2's bit ring, by name. Coverage only."""
import ctypes as C

from tests import hufmodel, reflib, seqmodel
from tests.hufmodel import Refused

KINDS = ("LL", "OF", "ML")
MAX_SYMBOL = (35, 31, 52)
MAX_LOG = (9, 8, 9)
DEF_LOG = (6, 5, 6)
K2_CELLS = (512, 256, 512)                                   # K2's slot: 512 LL + 512 ML + 256 OF two-byte cells (ZP_FSE_CELLS; pinned by the tests)
STAGED = 256                                                 # bytes of a block's descriptions K0 and K1 stage
LL_BASE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
_DEF = {}


class Table:
    """one decoding table and where it came from: source = "predefined" / "RLE" / "described" / "dictionary"; norm None for an RLE table"""
    def __init__(self, cells, log, source, norm=None, used=0, chains=()):
        self.cells, self.log, self.source, self.norm, self.used, self.chains = cells, log, source, norm, used, chains


def predefined(kind):
    if kind not in _DEF:
        lib = C.CDLL(reflib.ORACLE_SO)
        name, n = (("zo_ll_defnorm", 36), ("zo_of_defnorm", 29), ("zo_ml_defnorm", 53))[kind]
        norm = list((C.c_int16 * n).in_dll(lib, name))
        _DEF[kind] = Table(hufmodel.fse_table(norm, DEF_LOG[kind]), DEF_LOG[kind], "predefined", norm)
    return _DEF[kind]


def zero_chains(buf):
    """the zero-run flag chains of the (valid) description at the start of `buf`, each as a tuple of its 2-bit flags: coverage only"""
    v, pos = int.from_bytes(buf, "little"), 4
    log = (v & 15) + 5
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    chains, prev0, n, forms = [], False, 0, []
    while remaining > 1:
        if prev0:
            ch = []
            while True:
                r = (v >> pos) & 3; pos += 2; ch.append(r); n += r
                if r != 3: break
            chains.append(tuple(ch))
        mx = 2 * threshold - 1 - remaining
        low = (v >> pos) & ((1 << (nb - 1)) - 1)
        if low < mx: count = low; pos += nb - 1; forms.append("short")
        else:
            count = (v >> pos) & ((1 << nb) - 1)
            if count >= threshold: count -= mx
            pos += nb; forms.append("long")
        count -= 1; remaining -= abs(count); prev0 = count == 0; n += 1
        while remaining < threshold: nb -= 1; threshold >>= 1
    zero_chains.forms = forms                                  # (the width each count was written in, of the last description read)
    return tuple(chains), pos


def read_table(buf, kind, source="described"):
    """the description at the start of `buf` (the rest of the block) -> Table; Refused under the limits of `kind`"""
    norm, log, used = hufmodel.read_ncount(buf, MAX_SYMBOL[kind])
    if log > MAX_LOG[kind]: raise Refused("accuracy log %d above %d" % (log, MAX_LOG[kind]))
    t = Table(hufmodel.fse_table(norm, log), log, source, norm, used, zero_chains(buf[:used] + bytes(8))[0])
    t.forms = list(zero_chains.forms)
    return t


def dictionary_tables(dict_data):
    """the three tables of a trained dictionary (offsets, match lengths, literal lengths behind its Huffman table), as [LL, OF, ML], or None"""
    weights, at = hufmodel.dictionary_weights(dict_data)
    if weights is None: return None
    tabs = {}
    for kind in (1, 2, 0):
        tabs[kind] = read_table(dict_data[at:], kind, "dictionary"); at += tabs[kind].used
    return [tabs[0], tabs[1], tabs[2]]


def sequences_section(buf, prev, info):
    """the sequences section `buf` (to the block's end); prev = the three Tables a "repeat" takes, or None. -> ([(ll, ml, offset value)], Tables left)"""
    if len(buf) < 1: raise Refused("sequences: nothing to read")
    n, at = buf[0], 1
    if n > 127:
        if n == 255:
            if at + 2 > len(buf): raise Refused("sequences: count past the block")
            n = int.from_bytes(buf[1:3], "little") + 0x7F00; at = 3
        else:
            if at + 1 > len(buf): raise Refused("sequences: count past the block")
            n = ((n - 128) << 8) + buf[1]; at = 2
    info["count"] = n
    if n == 0:
        if at != len(buf): raise Refused("sequences: bytes behind a count of zero")
        return [], prev
    if at + 1 > len(buf): raise Refused("sequences: no modes byte")
    modes = buf[at]; at += 1
    if modes & 3: raise Refused("sequences: reserved mode bits")
    tabs, start = [], at
    info["modes"] = tuple((modes >> s) & 3 for s in (6, 4, 2))
    for kind, mode in enumerate(info["modes"]):
        if mode == 0: t = predefined(kind)
        elif mode == 1:
            if at >= len(buf): raise Refused("%s table: no RLE symbol" % KINDS[kind])
            if buf[at] > MAX_SYMBOL[kind]: raise Refused("%s table: RLE symbol above the alphabet" % KINDS[kind])
            t = Table([(buf[at], 0, 0)], 0, "RLE"); at += 1
        elif mode == 2:
            try: t = read_table(buf[at:], kind)
            except Refused as e: raise Refused("%s table: %s" % (KINDS[kind], e.reason))
            at += t.used
        else:
            if prev is None: raise Refused("%s table: repeat with nothing to repeat" % KINDS[kind])
            t = prev[kind]
        tabs.append(t)
    info["tables"], info["desc_bytes"], info["stream_off"], info["stream_bytes"] = tabs, at - start, at, len(buf) - at
    try: b = hufmodel._Back(buf[at:], "sequences' bit stream")
    except Refused: raise Refused("sequences: no bit stream behind the tables")
    st = [b.read(tabs[0].log), b.read(tabs[1].log), b.read(tabs[2].log)]
    info["initial"] = tuple(st)
    seqs, steps, visited = [], [], [set(), set(), set()]
    for i in range(n):
        if b.left < 0: raise Refused("sequences: the bit stream runs out")
        for k in range(3): visited[k].add(st[k])
        lc, oc, mc = tabs[0].cells[st[0]][0], tabs[1].cells[st[1]][0], tabs[2].cells[st[2]][0]
        ofv = (1 << oc) + b.read(oc)
        ml = ML_BASE[mc] + b.read(ML_BITS[mc])
        ll = LL_BASE[lc] + b.read(LL_BITS[lc])
        seqs.append((ll, ml, ofv))
        if i + 1 < n:
            state_bits = 0
            for k in (0, 2, 1):
                _, nb, base = tabs[k].cells[st[k]]
                st[k] = base + b.read(nb); state_bits += nb
            steps.append((state_bits, oc + ML_BITS[mc] + LL_BITS[lc]))
    if b.left < 0: raise Refused("sequences: the bit stream runs out")
    if b.left > 0: raise Refused("sequences: bits left over")
    info["steps"], info["visited"] = steps, visited
    return seqs, tabs


def sequences(frame, dict_data=None, infos=None):
    """the frame's blocks in seqmodel.execute's form, every compressed block's literals and sequences decoded from its bytes"""
    huf, _ = hufmodel.dictionary_weights(dict_data)
    prev = dictionary_tables(dict_data)
    blocks = []
    for t, pos, size, _ in hufmodel.walk(frame):
        if t == 0: blocks.append(("raw", frame[pos:pos + size])); continue
        if t == 1: blocks.append(("rle", frame[pos], size)); continue
        if t == 3: raise Refused("frame: reserved block type")
        if size > seqmodel.BLOCK_MAX: raise Refused("frame: compressed block above the block maximum")
        info = {"at": pos}
        if infos is not None: infos.append(info)
        buf = frame[pos:pos + size]
        lits, used, huf = hufmodel.literals_section(buf, huf)
        seqs, prev = sequences_section(buf[used:], prev, info)
        info["stream_at"] = pos + used + info.get("stream_off", 0)
        blocks.append(("seq", lits, seqs))
    return blocks


def decode(frame, dict_data=None, dict_content=b"", start_reps=(1, 4, 8), infos=None):
    """the content of `frame`; raises hufmodel.Refused / seqmodel.Invalid with the reason"""
    return seqmodel.execute(sequences(frame, dict_data, infos), dict_content, start_reps)


def census(frame, dict_data=None, base=0):
    """the set of named things `frame`, lying at absolute offset `base` of its arena, reaches on the sequence-table path. Coverage only."""
    ev, infos = set(), []
    try: sequences(frame, dict_data, infos)
    except (Refused, seqmodel.Invalid) as e: ev.add("refused: " + e.reason)
    for i in infos:
        if "tables" not in i or "steps" not in i: continue
        tabs = i["tables"]
        ev.add("modes %d %d %d" % i["modes"])
        ev.add("description bytes in a block: %s" % ("0" if i["desc_bytes"] == 0 else "1..31" if i["desc_bytes"] < 32 else "32..99" if i["desc_bytes"] < 100 else "100 and up"))
        ev.add("bit stream starts at %d mod 16" % ((base + i["stream_at"]) % 16))
        if i["stream_bytes"] == 1: ev.add("bit stream of one byte")
        if i["count"] == 1: ev.add("one sequence")
        for k, t in enumerate(tabs):
            K = KINDS[k]
            if i["modes"][k] == 3: ev.add("repeat of a %s table" % t.source)
            ev.add("%s initial state %s" % (K, "0" if i["initial"][k] == 0 else "the last" if i["initial"][k] == (1 << t.log) - 1 else "inside"))
            if t.norm is None or t.source == "predefined": continue
            ev.add("%s log %d" % (K, t.log))
            top = len(t.norm) - 1
            ev.add("%s highest symbol %d" % (K, top))
            used_top = any(t.cells[x][0] == MAX_SYMBOL[k] for x in i["visited"][k])
            if used_top: ev.add("%s top code in use" % K)
            low = sum(c == -1 for c in t.norm)
            ev.add("%s 'less than one' symbols: %s" % (K, "none" if low == 0 else "one" if low == 1 else "all cells" if low == 1 << t.log else "all but one symbol" if low == sum(c != 0 for c in t.norm) - 1 else "several"))
            if low > 8: ev.add("%s log %d: %d 'less than one' symbols" % (K, t.log, low))
            if t.norm[0] == -1 and low >= 2: ev.add("'less than one' at the lowest symbols")
            if t.norm[-1] == -1 and low >= 2: ev.add("'less than one' at the highest symbols")
            for ch in t.chains: ev.add("zero-run flags %s" % ",".join(str(x) for x in ch))
            for n, f in enumerate(getattr(t, "forms", ())): ev.add("%s %s count in the %s form" % (K, "first" if n == 0 else "later", f))
            present = sum(c != 0 for c in t.norm)
            ev.add("%s symbols present: %s" % (K, present if present <= 3 else "all" if present == MAX_SYMBOL[k] + 1 else "several"))
            if present == 1:
                ev.add("%s single-symbol table of log %d, symbol %d" % (K, t.log, top))
                if k == 2 and t.log == 9 and top == 52: ev.add("K2 cell with x = 1023 beside symbol 52")
            if len(i["visited"][k]) == 1 << t.log: ev.add("every cell of a %s log-%d table visited" % (K, t.log))
        if all(t.log == K2_CELLS[k].bit_length() - 1 for k, t in enumerate(tabs)): ev.add("K2 slot filled: 512 + 512 + 256 cells")
        if i["steps"]:
            most = max(s for s, _ in i["steps"]); least = min(s for s, _ in i["steps"])
            ev.add("state bits in a step: %d" % most)
            if least == 0: ev.add("a step that reads no state bits")
            ev.add("bits in a step, extra bits included: %d" % max(s + e for s, e in i["steps"]))
            per = [s + e for s, e in i["steps"]]
            if len(per) >= 4:
                ev.add("bits in four consecutive steps: %d, the stream's first byte at %d mod 16" % (max(sum(per[j:j + 4]) for j in range(len(per) - 3)), (base + i["stream_at"]) % 16))
    return ev


def group_census(frames, dict_data=None):
    """what a batch of frames of one block, decoded side by side in K2's waves, holds. Coverage only."""
    ev = {"K2 group of %d frames" % len(frames)}
    logs, refused, shared, own = set(), 0, 0, 0
    for f in frames:
        infos = []
        try: sequences(f, dict_data, infos)
        except (Refused, seqmodel.Invalid): refused += 1; continue
        for i in infos:
            if "tables" not in i: continue
            logs.add(tuple(t.log for t in i["tables"]))
            if all(t.source == "dictionary" for t in i["tables"]): shared += 1
            if any(t.source == "described" for t in i["tables"]): own += 1
    if (5, 5, 5) in logs and MAX_LOG in logs: ev.add("K2 group: logs 5 5 5 beside 9 8 9")
    if shared and own: ev.add("K2 group: shared dictionary tables beside described ones")
    if refused and refused < len(frames): ev.add("K2 group: a refused frame among the others")
    return ev
