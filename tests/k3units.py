"""Cases for K3's long-item units and its scalar-base addressing (test infrastructure for tests/test_emu_k3_units.py and tests/test_gpu_k3_units.py).

A literal run or a far match (or the part of a near match that precedes the batch) above 16 bytes is not copied by its own lane: zp_exec_block cuts
it into 16-byte units -- the last one shifted back to end with the item --, deals the batch's units out to the lanes, and a unit finds its item by a
binary search over the unit prefix sums and reads what it needs of the item from the item lane's 16-byte record in LDS (ZpUnitRec: source, position
in the batch and length of the literal run and of the match item, the item's first unit, its count of literal units). Without a dictionary every
global address of the batch loop is the frame's slot, the block's literals or the block's sequences plus an unsigned 32-bit lane offset.

The cases are the smallest shapes at which that can go wrong: unit counts around the 64 lanes of a trip, items of every last-unit shift, both items
in one lane, lanes 0 and 63, the record's fields at their largest, sources in, at and below the LDS history before and after a slide, sources above
2^17 and 2^20, sources in a dictionary, slots smaller than the 32 bytes of slack the short loads like to have. Expected bytes are seqmodel.execute's;
`batches()` restates the unit staging of zp_exec_block for the coverage assertions only."""
import numpy as np

from tests import seqfamilies as F
from tests.seqmodel import K3, resolved

FAMILY = "k3 units"
MODES = ("raw", "huf", "rle")
ITEM_LENGTHS = (17, 31, 32, 33, 48)             # the last unit shifted back by 15, 1, 0, 15, 0


def units(n, short=16):
    return (n + 15) >> 4 if n > short else 0


def batches(blocks, k=K3, start_reps=(1, 4, 8)):
    """the batches of every compressed block as zp_exec_block forms them (big items left out): for each, the bytes of history and the carried tail in
    front of it, whether a slide preceded it, its literal mode, and its long items in unit order -- lane, kind ("lit", "far", "pre"), length, first
    unit, units, source (position in the block's literals / in the frame, negative: in the dictionary), position in the batch, and for a match item
    where its source lies against the LDS history"""
    A, KEEP, SLIDE = k.asm_bytes, k.hist_keep, k.hist_slide
    out, pos = [], 0
    for b, seqs in zip(blocks, resolved(blocks, start_reps)):
        if seqs is None:
            pos += len(b[1]) if b[0] == "raw" else b[2]; continue
        mode = (b[3] if len(b) > 3 else {}).get("lit", "raw")
        op, hOff, carry, done, lp, slid = pos, 0, 0, 0, 0, False
        while done < len(seqs):
            win = seqs[done:done + k.batch_seqs]
            cnt, acc = 0, 0
            for ll, ml, _ in win:
                if acc + ll + ml + carry > A - hOff: break
                acc += ll + ml; cnt += 1
            if cnt == 0:
                op += win[0][0] + win[0][1]; lp += win[0][0]; carry = 0; done += 1; hOff = 0; slid = False
                continue
            ob, rel, U, items = op - carry, carry, 0, []
            for j, (ll, ml, of) in enumerate(win[:cnt]):
                if mode != "rle" and ll > k.lit_short:
                    items.append(dict(lane=j, kind="lit", len=ll, first=U, n=units(ll), src=lp, dst=rel)); U += units(ll)
                lp += ll
                mRel = rel + ll
                sAbs = ob + mRel - of
                far = sAbs + ml <= ob
                pre = not far and sAbs < ob
                lenMi = ml if far else ob - sAbs if pre else 0
                if (far or pre) and lenMi > k.far_short and not sAbs < 0 < sAbs + lenMi:
                    where = "dictionary" if sAbs < 0 else "inside" if sAbs >= ob - hOff else "one before" if sAbs == ob - hOff - 1 else "straddles" if sAbs + lenMi > ob - hOff else "below"
                    items.append(dict(lane=j, kind="far" if far else "pre", len=lenMi, first=U, n=units(lenMi), src=sAbs, dst=mRel, where=where if hOff or sAbs < 0 else "no history"))
                    U += units(lenMi)
                rel = mRel + ml
            out.append(dict(U=U, items=items, hOff=hOff, carry=carry, ob=ob, end=hOff + rel, after_slide=slid, lit=mode, lit_size=len(b[1])))
            whole = (acc + carry) & ~15
            carry = acc + carry - whole; op += acc; done += cnt; hOff += whole; slid = False
            if hOff > SLIDE: hOff = KEEP; slid = True
        pos = op + len(b[1]) - lp
    return out


def _opened(rng, k):
    """behind a big item: no LDS history, no carried tail, and k.asm_bytes + 48 bytes of the frame to read from global memory"""
    return F.Builder(rng).seq(k.asm_bytes + 40, 8, 11)


def _batch(b, items, n=64, align=True):
    """one batch of n sequences at b: `items` = {lane: (ll, ml, src)} (src: the match's absolute source, or None for a short match of offset 3 behind at
    least three literals), every other lane a plain sequence of 1 literal + 3 match bytes that makes no unit; align: the last plain lane takes the
    literals that make the batch a multiple of 16 bytes, so the next batch starts without a carried tail"""
    start = b.pos
    plain = [j for j in range(n) if j not in items]
    for j in range(n):
        if j in items:
            ll, ml, src = items[j]
            if src is None: b.seq(ll, ml, 3)
            else: b.at(ll, ml, src)
        else:
            ll = 1
            if align and j == plain[-1]:
                rest = sum(items[i][0] + items[i][1] for i in items if i > j)
                ll += (-(b.pos - start + 4 + rest)) % 16
            b.seq(ll, 3, min(b.pos + ll, 300))
    return b


def _composition(total):
    """item lengths from ITEM_LENGTHS in turn whose units add up to `total` (an item has two units at least)"""
    out, left, i = [], total, 0
    while left:
        n = ITEM_LENGTHS[i % len(ITEM_LENGTHS)]; i += 1
        if units(n) > left or left - units(n) == 1: n = 33 if left == 3 else 17
        out.append(n); left -= units(n)
    return out


def _case(name, blocks, **kw):
    return F.Case(FAMILY, name, blocks, **kw)


def unit_counts(k=K3, seed=41):
    """2, 63, 64, 65, 127, 128, 129 units in one batch, literal runs and far matches from global memory in turn, one item per lane and both in one lane;
    the shapes around unit 64 (the second trip of the unit pass); the most a batch admits"""
    rng = np.random.default_rng(seed)
    A = k.asm_bytes
    cases = []
    for U in (2, 63, 64, 65, 127, 128, 129):
        for both in (False, True):
            if both and U < 63: continue
            b = _opened(rng, k)
            lens = _composition(U)
            items, lane = {}, 0
            src = 50
            while lens:
                if both and len(lens) >= 2: items[lane] = (lens.pop(0), lens.pop(0), src)
                elif (lane & 1) or both: items[lane] = (2, lens.pop(0), src)
                else: items[lane] = (lens.pop(0), 3, None)
                src += 37; lane += 1
            _batch(b, items)
            cases.append(_case("%d units in one batch, %s" % (U, "a literal run and a far match in every item lane" if both else "one item per lane"), [b.block(rest=2)]))
    # the last item starts at unit 62 of 64; an item over units 63 | 64; an item that starts at unit 64 and one above
    for name, head, tail in (("64 units, the last item from unit 62", 62, (17,)), ("65 units, one item over units 63 and 64", 63, (17,)),
                             ("an item from unit 64 on and one from 66", 64, (31, 33)), ("an item over units 63 to 65 and one from 66", 63, (48, 17))):
        b = _opened(rng, k)
        items = {0: (1, 16 * head, 100)}
        for i, n in enumerate(tail): items[1 + i] = (n, 3, None) if i % 2 == 0 else (1, n, 700)
        _batch(b, items)
        cases.append(_case(name, [b.block()]))
    # the most a batch admits: the whole buffer as one literal run (256 literal units, the record's largest count) ...
    cases.append(_case("one literal run of the buffer's size less three", [F.Builder(rng).seq(A - 3, 3, 1).fill(64, 512).block(rest=1)]))
    # ... one far match of exactly the buffer's size (the record's length field at its largest) ...
    cases.append(_case("one far match of the buffer's size", [_opened(rng, k).at(0, A, 20).fill(64, 512).block(rest=1)]))
    # ... and one item that ends with the buffer, behind a history and a carried tail of 15
    for kind in ("lit", "far"):
        b = _opened(rng, k).fill(64, 16 * 16 + 15)
        room = A - 16 * 16 - 15
        if kind == "lit": b.seq(room - 3, 3, 900)
        else: b.at(2, room - 2, 60)
        b.fill(64, 512)
        cases.append(_case("one %s item that ends exactly at the buffer's end behind a tail of 15" % ("literal" if kind == "lit" else "far-match"), [b.block(rest=3)]))
    return cases


def item_shapes(k=K3, seed=42):
    """lanes 0 and 63 as long items (both kinds each), every length of ITEM_LENGTHS as a literal run and as a far match next to each other, a pre-batch
    part above 16 bytes beside long items"""
    rng = np.random.default_rng(seed)
    cases = []
    b = _opened(rng, k)
    _batch(b, {0: (33, 48, 10), 63: (48, 17, 4000), 31: (17, 3, None), 32: (2, 31, 2000)})
    _batch(b, {0: (17, 17, b.pos - 600), 63: (31, 32, 3)})                       # (sources in the history the first batch left, and at the frame's third byte)
    cases.append(_case("lanes 0 and 63 with a long literal run and a long far match each", [b.block(rest=1)]))
    b = _opened(rng, k)
    items = {}
    for i, n in enumerate(ITEM_LENGTHS):
        items[3 + 2 * i] = (n, 3, None); items[4 + 2 * i] = (1, n, 200 + 50 * i); items[40 + i] = (n, ITEM_LENGTHS[-1 - i], 1000 + 70 * i)
    _batch(b, items)
    cases.append(_case("literal runs and far matches of 17, 31, 32, 33 and 48 bytes", [b.block()]))
    for p in (17, 40):
        b = F.Builder(rng).fill(64, 512)
        _batch(b, {0: (2, p + 30, b.pos + 2 - p), 1: (33, 3, None), 2: (1, 48, 20), 63: (17, 17, 100)})      # lane 0: a near match whose first p bytes precede the batch
        cases.append(_case("a pre-batch part of %d bytes beside long items" % p, [b.block(rest=2)]))
    return cases


def record_fields(k=K3, seed=43):
    """a long literal run that starts above 65 535 in its block's literals and one that ends with a literal section of nearly the block maximum (the
    sequences and the section's header take the rest of a block's 128 KiB)"""
    rng = np.random.default_rng(seed)
    b = F.Builder(rng).seq(66000, 4, 10)
    _batch(b, {0: (40, 3, None), 5: (17, 5, 2000), 63: (100, 33, 30000)})
    b.seq(63000, 5, 9)
    _batch(b, {1: (33, 17, 100000), 62: (48, 3, None), 63: (17, 3, None)}, align=False)
    return [_case("literal runs in units from above 65 535 and at the end of %d literals" % b.nlit, [b.block(rest=0)])]


def history(k=K3, seed=44):
    """long far matches whose source lies wholly inside the LDS history, starts one byte before it, straddles its first byte, lies wholly below it:
    behind two batches of history, and again behind a slide"""
    rng = np.random.default_rng(seed)
    b = _opened(rng, k).fill(64, 1024)
    h0 = b.pos - 1024

    def quartet(h):
        return {2: (1, 48, h + 100), 7: (33, 33, h - 1), 20: (2, 40, h - 20), 41: (17, 17, 100), 63: (1, 200, h + 16)}
    _batch(b, quartet(h0))
    while not batches([("seq", b"", b.seqs + [(1, 3, 4)], {})], k)[-1]["after_slide"]:      # plain batches until the next one starts behind a slide
        b.fill(64, 1024)
    _batch(b, quartet(b.pos - k.hist_keep))
    return [_case("long far matches inside, at, across and below the history, before and after a slide", [b.block(rest=2)])]


def distant_sources(k=K3, seed=45):
    """far matches in units whose sources lie above 2^17 and above 2^20: raw blocks of 128 KiB of noise in front (frames of several blocks)"""
    rng = np.random.default_rng(seed)
    cases = []
    for name, lead in (("2^17", [("raw", bytes(rng.integers(0, 256, 1000, dtype=np.uint8))), ("raw", bytes(rng.integers(0, 256, 131072, dtype=np.uint8)))]),
                       ("2^20", [("raw", bytes(rng.integers(0, 256, 1000, dtype=np.uint8)))] + [("rle", 0x41 + i, 131072) for i in range(7)] +
                                [("raw", bytes(rng.integers(0, 256, 131072, dtype=np.uint8)))])):
        pos = sum(len(x[1]) if x[0] == "raw" else x[2] for x in lead)
        b = F.Builder(rng, pos)
        _batch(b, {0: (33, 48, pos - 400), 9: (2, 17, pos - 17), 10: (17, 31, pos - 900), 30: (1, 100, 500), 63: (1, 33, pos - 33 - 64)})
        _batch(b, {0: (2, 48, pos - 200), 63: (31, 32, pos - 1000)})
        c = _case("far matches in units from above " + name, lead + [b.block(rest=1)], header={"window_log": 21})
        c.above = pos - 1000
        cases.append(c)
    return cases


def dictionary_cases(k=K3, seed=46):
    """raw-content dictionary: long far matches wholly inside it (a negative source through the record), one that ends at the frame's first byte, a
    straddler beside long items, with and without an LDS history"""
    rng = np.random.default_rng(seed)
    dd = bytes(rng.integers(0, 256, 3000, dtype=np.uint8))
    cases = []
    for hist in (False, True):
        b = F.Builder(rng)
        if hist: b.fill(64, 1024)
        else: b.seq(5, 4, 100)
        n = 64 if hist else 63
        _batch(b, {0: (2, 40, -2000), 1: (33, 17, -17), 2: (1, 300, -100), 3: (17, 48, -3000), n - 1: (48, 33, -900)}, n=n)
        cases.append(F.Case(FAMILY, "long far matches inside the dictionary, a straddler beside them, %s history" % ("behind a" if hist else "no"), [b.block(rest=1)],
                            dict_data=dd, raw_dict=True))
    return cases


def small_slots(k=K3, seed=47):
    """frames of 0 to 40 bytes in slots of exactly their size: below 32 bytes the short loads have no slack and take their exact form, from 32 on the
    slack form; behind a raw block (the several-block form) the match source is a pre-batch part at the slot's first byte"""
    rng = np.random.default_rng(seed)
    cases = []
    for n in list(range(0, 34)) + [40]:
        if n < 4: blk = F.Builder(rng).block(rest=n)
        elif n < 12: blk = F.Builder(rng).seq(n - 3, 3, 1).block()
        else: blk = F.Builder(rng).seq(n - 9, 3, 2).seq(1, 3, n - 8).block(rest=2)
        cases.append(_case("%d bytes in a slot of %d" % (n, n), [blk]))
    return cases


def in_mode(c, mode):
    """the case with the literals of every compressed block in `mode` (tests/k3litmodes.py's form)"""
    v = F.Case(c.family, "%s [%s literals]" % (c.name, mode), F.lit_variant(c.blocks, mode), c.dict_data, c.raw_dict, c.fcs, c.checksum, c.start_reps, dict(c.header), c.cap, c.short_by)
    v.base_name, v.lit_mode = c.name, mode
    return v


def block_modes(c):
    return [(b[3] if len(b) > 3 else {}).get("lit", "raw") for b in c.blocks if b[0] == "seq"]


def one_block_cases(k=K3):
    """the cases of one block, in the three literal modes, with the slot-edge family (short far matches and far units within 32 bytes of the slot's end)"""
    base = unit_counts(k) + item_shapes(k) + record_fields(k) + history(k) + small_slots(k) + F.slot_edges(k)
    return [in_mode(c, m) for c in base for m in MODES]


def all_batches(c, k=K3):
    return batches(c.blocks, k, c.start_reps)


FIXTURE = "tests/golden/k3_units.bin"


def fixture_cases(k=K3):
    """what the stand-alone sanitizer program of tests/emu/emu_k3_units.cpp decodes: every family above once, the literal modes in turn, as frames of one block
    and behind a raw block, the frame of several blocks with sources above 2^17, the dictionary cases (the frame with 128 KiB of raw literals and the one above
    2^20 stay out: the file is committed)"""
    base = unit_counts(k) + item_shapes(k) + history(k) + small_slots(k)[::3]
    cases = [in_mode(c, MODES[i % 3]) for i, c in enumerate(base)] + [in_mode(record_fields(k)[0], "huf")]
    plain = [(0, c) for c in cases] + [(1, c.with_lead()) for c in cases[::2]] + [(1, distant_sources(k)[0])]
    dicts = [in_mode(c, MODES[i % 3]) for i, c in enumerate(dictionary_cases(k))]
    return plain + [(2, c) for c in dicts] + [(3, c.with_lead()) for c in dicts]


def fixture_blob(ref, oracle):
    import struct
    from tests.seqmodel import check_model
    items = fixture_cases()
    dd = next(c.dict_data for g, c in items if g & 2)
    out = [b"K3U1", struct.pack("<I", len(dd)), dd, struct.pack("<I", len(items))]
    for flags, c in items:
        c.build(oracle.xxh64)
        check_model(ref, c.frame, c.want, c.cap, c.dict_data, c.raw_dict)
        h = 0xcbf29ce484222325
        for x in c.want or b"": h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        out.append(struct.pack("<IIIIQ", flags, len(c.frame), c.cap, 0xFFFFFFFF if c.want is None else len(c.want), h) + c.frame)
    return len(items), b"".join(out)


def write_fixture(path=FIXTURE):
    from tests import reflib
    n, blob = fixture_blob(reflib.RefZstd(), reflib.Oracle())
    with open(path, "wb") as f: f.write(blob)
    return n, len(blob)


if __name__ == "__main__":
    import sys
    if "--write-fixture" in sys.argv: print("%d frames, %d bytes" % write_fixture())
