"""What a frame described by explicit sequences decodes to, and which of K3's paths it walks (test infrastructure).

* execute() is RFC 8878's sequence semantics in straight Python -- literal copy, the repeat-offset rules with the `ll == 0` shift and "repeat
  offset 1 minus one", byte-wise match copy -- over the block descriptions tests/craft.py's write_frame() turns into bytes. It is the expected
  value of tests/test_emu_sequences.py and tests/test_gpu_sequences.py; libzstd is asked too, and must agree first (check_model).
* census() restates the batching of zp_exec_block (python-zstandard_amd/csrc/zhip_decode_pipeline.hpp): batches of at most 64 sequences behind a
  history of hOff bytes, the carried tail, the slide, "big" items, own-lane and unit staging, near matches and their dependency rounds. It
  returns the set of named events a frame reaches and is used ONLY to assert coverage, never for expected bytes.

The kernel constants are stated once, in K3Consts; test_emu_sequences.py::test_census_constants_match_the_kernel_headers pins them against the
header text."""
import collections

BLOCK_MAX = 131072


class Invalid(Exception):
    """the frame must be refused; .reason says why"""
    def __init__(self, reason):
        Exception.__init__(self, reason); self.reason = reason


class K3Consts(collections.namedtuple("K3Consts", "asm_bytes coop_len lit_short far_short batch_seqs")):
    """ZD_ASM_BYTES (ZP_ASM_BYTES), ZD_COOP_LEN, ZP_LIT_SHORT, ZP_FAR_SHORT and the 64 lanes of a batch; hist_keep / hist_slide are the headers' formulas"""
    @property
    def hist_keep(self): return (self.asm_bytes * 5 // 16) & ~15

    @property
    def hist_slide(self): return 2 * self.hist_keep + 16


K3 = K3Consts(asm_bytes=4096, coop_len=32, lit_short=16, far_short=16, batch_seqs=64)
K3_SMALL = K3._replace(asm_bytes=2048)                                     # the -DZP_ASM_BYTES=2048 variant build


def next_reps(reps, ll, ofv):
    """(offset, new history) of one sequence with offset VALUE ofv (1..3 repeat codes, n + 3 = offset n); offset 0 = 'repeat offset 1 minus one' reached 0"""
    r0, r1, r2 = reps
    if ofv > 3: return ofv - 3, (ofv - 3, r0, r1)
    k = ofv - 1 + (1 if ll == 0 else 0)
    if k == 0: return r0, reps
    if k == 1: return r1, (r1, r0, r2)
    if k == 2: return r2, (r2, r0, r1)
    return r0 - 1, (r0 - 1, r0, r1)


def execute(blocks, dict_content=b"", start_reps=(1, 4, 8), block_max=BLOCK_MAX):
    """the bytes `blocks` decode to, or raises Invalid(reason)"""
    out = bytearray(dict_content)
    base = len(out)
    reps = tuple(start_reps)
    for b in blocks:
        if b[0] == "raw":
            if len(b[1]) > block_max: raise Invalid("raw block above the block maximum")
            out += b[1]; continue
        if b[0] == "rle":
            if b[2] > block_max: raise Invalid("RLE block above the block maximum")
            out += bytes([b[1]]) * b[2]; continue
        lits, seqs = b[1], b[2]
        lp, start = 0, len(out)
        for ll, ml, ofv in seqs:
            if lp + ll > len(lits): raise Invalid("literal lengths past the section")
            out += lits[lp:lp + ll]; lp += ll
            off, reps = next_reps(reps, ll, ofv)
            if off == 0: raise Invalid("repeat offset 1 minus one is zero")
            if off > len(out): raise Invalid("offset beyond the history")
            if len(out) + ml - start > block_max: raise Invalid("block output above the block maximum")
            s = len(out) - off
            if off >= ml: out += out[s:s + ml]
            else:
                for _ in range(ml): out.append(out[s]); s += 1
        out += lits[lp:]
        if len(out) - start > block_max: raise Invalid("block output above the block maximum")
    return bytes(out[base:])


def final_reps(blocks, start_reps=(1, 4, 8)):
    reps = tuple(start_reps)
    for b in blocks:
        if b[0] == "seq":
            for ll, ml, ofv in b[2]: _, reps = next_reps(reps, ll, ofv)
    return reps


def check_model(ref, frame, want, cap, dict_data=None, raw_dict=False):
    """libzstd's verdict on `frame` against the executor's (`want`: bytes, or None for a frame that must be refused): a disagreement is a failure
    of the test's MODEL, raised as such, before any kernel is looked at"""
    try:
        got = ref.decompress_advanced(frame, cap, dict_data=dict_data, dict_type=1 if raw_dict else 0) if dict_data else ref.decompress(frame, cap)
        if dict_data is not None and len(got) != cap: got = None
    except RuntimeError:
        got = None
    if got != want:
        raise AssertionError("TEST MODEL, not a kernel: the executor and libzstd disagree (libzstd %s, executor %s)" % (
            "refuses" if got is None else "%d bytes" % len(got), "refuses" if want is None else "%d bytes" % len(want)))


def resolved(blocks, start_reps=(1, 4, 8)):
    """per block: None, or its sequences as (ll, ml, offset) with the repeat codes resolved"""
    reps = tuple(start_reps); res = []
    for b in blocks:
        if b[0] != "seq": res.append(None); continue
        q = []
        for ll, ml, ofv in b[2]:
            off, reps = next_reps(reps, ll, ofv); q.append((ll, ml, off))
        res.append(q)
    return res


def canonical(blocks, start_reps=(1, 4, 8)):
    """`blocks` with every offset value rewritten to the form libzstd's ZSTD_c_searchForExternalRepcodes leaves: walking the repeat-offset history (it starts
    at the format's 1, 4, 8, or at the dictionary's), an offset that IS one of the three history entries is written as that entry's repeat code -- with
    literals in front, codes 1, 2, 3 name entries one, two, three; with NO literals the codes shift, 1 and 2 name entries two and three, and 3 names "entry
    one minus one" --, the first that applies in the order entry one (only with literals), two, three, one-minus-one (only without); any other offset is
    offset + 3. The sequences resolve to the same offsets before and after (resolved())."""
    reps, out = tuple(start_reps), []
    for b, res in zip(blocks, resolved(blocks, start_reps)):
        if res is None: out.append(b); continue
        q = []
        for ll, ml, off in res:
            names = ([(1, reps[0])] if ll else []) + [(2 if ll else 1, reps[1]), (3 if ll else 2, reps[2])] + ([] if ll else [(3, reps[0] - 1)])
            code = next((c for c, v in names if v == off), off + 3)
            back, reps = next_reps(reps, ll, code)
            assert back == off
            q.append((ll, ml, code))
        out.append(("seq", b[1], q) + tuple(b[3:]))
    return out


def plain(blocks, start_reps=(1, 4, 8)):
    """`blocks` with every offset written as offset + 3, none as a repeat code (libzstd with ZSTD_c_searchForExternalRepcodes disabled)"""
    return [b if res is None else ("seq", b[1], [(ll, ml, off + 3) for ll, ml, off in res]) + tuple(b[3:]) for b, res in zip(blocks, resolved(blocks, start_reps))]


def census(blocks, k=K3, dict_size=0, start_reps=(1, 4, 8)):
    """the set of named events the VALID frame `blocks` reaches in zp_exec_block, block by block (each compressed block starts with an empty
    history, at its own output position)"""
    ev = set()
    A, KEEP, SLIDE = k.asm_bytes, k.hist_keep, k.hist_slide
    pos = 0
    total = sum(len(b[1]) if b[0] == "raw" else b[2] if b[0] == "rle" else len(b[1]) + sum(q[1] for q in b[2]) for b in blocks)
    if total < 32: ev.add("frame below 32 bytes")
    had_seqs, reps_only = False, 0                  # a compressed block with sequences came before; compressed blocks in a row that use repeat codes only
    for bi, (b, seqs) in enumerate(zip(blocks, resolved(blocks, start_reps))):
        more = any(x[0] == "seq" and x[2] for x in blocks[bi + 1:])
        if had_seqs and more and (seqs is None or not seqs):
            ev.add(("raw block" if b[0] == "raw" else "RLE block" if b[0] == "rle" else "block without sequences") + " between compressed blocks")
        if seqs:
            raw = b[2]
            if had_seqs and len(raw) >= 3:
                ev.add("opening after a block boundary: " + " ".join("%s/%s" % (v if v <= 3 else "new", "0" if ll == 0 else "+") for ll, _, v in raw[:3]))
            chain = 0
            while chain < len(raw) and raw[chain][0] == 0 and raw[chain][2] == 3: chain += 1
            if had_seqs and chain >= 2: ev.add("'repeat offset 1 minus one' after a block boundary: %s times" % (chain if chain < 4 else "4 and more"))
            reps_only = reps_only + 1 if all(v <= 3 for _, _, v in raw) else 0
            if reps_only >= 3: ev.add("three blocks in a row of repeat codes only")
            for ll, ml, v in raw:
                if ll in (65535, 65536): ev.add("literal length %d" % ll)
                if ml in (65538, 65539, 131072): ev.add("match length %d" % ml)
                if 32768 <= ll < 65536 and ml >= 65539 and v.bit_length() - 1 >= 20: ev.add("LL code 34, ML code 52 and an offset code of 20 or more in one sequence")
            had_seqs = True
        if seqs is None:
            pos += len(b[1]) if b[0] == "raw" else b[2]; continue
        mode = (b[3] if len(b) > 3 else {}).get("lit", "raw")
        kind = "rle" if mode == "rle" else "raw" if mode == "raw" else "huf"
        if not seqs: ev.add("block without sequences")
        op, hOff, carry, done, after_big, after_slide = pos, 0, 0, 0, False, False
        while done < len(seqs):
            win = seqs[done:done + k.batch_seqs]
            room = A - hOff
            cnt, acc = 0, 0
            for ll, ml, _ in win:
                if acc + ll + ml + carry > room:
                    if cnt and acc + ll + ml + carry == room + 1: ev.add("first sequence left out is one byte above the room")
                    break
                acc += ll + ml; cnt += 1
            if cnt == 0:
                ll, ml, of = win[0]
                if of > 131072 and op + ll - of == 0: ev.add("offset above 128 KiB back to the frame's first byte")
                ev.add("big item: literals" if ml <= 32 else "big item: match" if ll <= 32 else "big item: both")
                if hOff: ev.add("big item after a history")
                op += ll + ml; carry = 0; done += 1; hOff = 0; after_big = True; after_slide = False
                continue
            ev.add("batch of 64 sequences" if cnt == k.batch_seqs else "batch cut by bytes" if cnt < len(win) else "batch: the block's last")
            if cnt < len(win) and acc + carry == room: ev.add("batch fills the room exactly")
            ob = op - carry
            rel = carry; U = 0
            near = []                                   # (index, mBeg, mEnd, a0, b0)
            depth = {}
            for j, (ll, ml, of) in enumerate(win[:cnt]):
                ev.add("%s literals: %s" % (kind, "0" if ll == 0 else "1..15" if ll < 16 else "16" if ll == 16 else "17..32" if ll <= 32 else "above 32"))
                if kind != "rle" and ll > k.lit_short: U += (ll + 15) >> 4
                mRel = rel + ll
                sAbs = ob + mRel - of
                if of > 131072 and sAbs == 0: ev.add("offset above 128 KiB back to the frame's first byte")
                far = sAbs + ml <= ob
                pre = (not far) and sAbs < ob
                lenMi = ml if far else (ob - sAbs if pre else 0)
                if far or pre:
                    strad = sAbs < 0 < sAbs + lenMi
                    inH = sAbs >= ob - hOff
                    if sAbs + lenMi <= 0: ev.add("dictionary: source wholly inside" + (", ending at the frame's first byte" if sAbs + lenMi == 0 else ""))
                    if strad: ev.add("dictionary straddler: " + ("self-overlapping" if of < ml else "short" if lenMi <= 16 else "long"))
                    if not strad and lenMi > k.far_short: U += (lenMi + 15) >> 4
                    if not inH and sAbs >= 0 and sAbs + 32 > total and lenMi <= k.far_short: ev.add("short far match within 32 bytes of the slot's end")
                    if sAbs >= 0 and sAbs + lenMi + 32 > total and lenMi > k.far_short: ev.add("far units within 32 bytes of the slot's end")
                    what = "far match" if far else "pre-batch part"
                    ev.add("%s: %s" % (what, "up to 16" if lenMi <= k.far_short else "17 and up"))
                    if far:
                        if sAbs + ml == ob: ev.add("far match ends exactly at the batch")
                        if hOff:
                            ev.add("far match: " + ("source starts at the history's first byte" if sAbs == ob - hOff else "source one byte before the history" if sAbs == ob - hOff - 1
                                                    else "source inside the history" if inH else "source below the history"))
                        else: ev.add("far match: no history")
                        if after_big and sAbs >= ob - A: ev.add("match into what a big item wrote")
                        if after_slide: ev.add("after a slide: source " + ("in the kept region" if inH else "just outside it" if sAbs >= ob - hOff - KEEP else "below"))
                    else:
                        if sAbs + ml == ob + 1: ev.add("near match: source ends one byte past the batch's start")
                        ev.add("pre-batch part: " + ("1" if lenMi == 1 else "2..16" if lenMi <= 16 else "above 16"))
                if not far:
                    nLen = ml - lenMi
                    ev.add("near match: offset " + ("below" if of < nLen else "equal to" if of == nLen else "above") + " the length")
                    ev.add("near match: length " + ("up to 32" if ml <= k.coop_len else "33" if ml == k.coop_len + 1 else "long"))
                    if ml > k.coop_len: ev.add("whole-wave near match: offset " + ("below 64" if of < 64 else "64 and up"))
                    ev.add("near match: offset %s" % (of if of <= 33 or of in (63, 64, 65) else "other"))
                    a0 = max(sAbs - ob, 0); b0 = min(sAbs + ml - ob, mRel)
                    d = 0; fed_by_lits_only = a0 < b0
                    for (i, mb, me) in near:
                        if me > a0 and mb < b0:
                            d = max(d, depth[i]); fed_by_lits_only = False
                            if a0 == me - 1: ev.add("near match reads an earlier one's last byte")
                            if b0 == mb + 1: ev.add("near match reads an earlier one's first byte")
                    if fed_by_lits_only and near and any(me <= a0 for (_, _, me) in near) and sAbs >= ob: ev.add("near match reads only this batch's literals")
                    depth[j] = d + 1
                    near.append((j, mRel, mRel + ml))
                rel = mRel + ml
            if depth:
                dm = max(depth.values())
                ev.add("dependency depth " + ("1" if dm == 1 else "2..8" if dm <= 8 else "9..62" if dm < 63 else "63 and up"))
            ev.add("units in a batch: " + ("0" if U == 0 else "1" if U == 1 else "2..63" if U < 64 else "64" if U == 64 else "65" if U == 65 else "66..128" if U <= 128 else "above 128"))
            totB = acc + carry
            whole = totB & ~15
            carry = totB - whole
            op += acc; done += cnt
            ev.add("carry %d" % carry)
            if done == len(seqs): ev.add("carry %d at the block's end" % carry)
            hOff += whole
            after_big = False; after_slide = False
            if hOff == SLIDE: ev.add("history exactly at the slide mark")
            if hOff > SLIDE:
                ev.add("slide" + (" 16 bytes past the mark" if hOff == SLIDE + 16 else ""))
                hOff = KEEP; after_slide = True
        lp = sum(q[0] for q in seqs)
        ev.add("last literals: " + ("none" if lp == len(b[1]) else "some"))
        if 0 < len(b[1]) - lp > A: ev.add("last literals above a batch's room")
        pos = op + len(b[1]) - lp
    if dict_size: ev.add("dictionary in use")
    return ev
