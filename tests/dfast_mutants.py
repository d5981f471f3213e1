"""One-token changes of decisions inside the double-fast searches (python-zstandard_amd/csrc/zhip_encode_kernel.hpp: ze_dfast_flat_np in its one-block and its block form,
ze_dfast_g, ze_dfast_ext), and what the aimed sources of tests/dfast_sources.py must do with each: (name, old text, new text, the forms it must be KILLED in | "equivalent: reason").
Only decision flips: comparison operators, constants, dropped table writes; none of them can make a search read outside a buffer (each one probes, inserts or extends LESS, or
at positions the unchanged code reads too).

Mutated code is compiled for the HOST only, by tests/test_emu_dfast_mutants.py, into a temporary directory, and run there in a child process. It is never compiled for, copied
to or run on a GPU; nothing here carries the `gpu` mark.

"Killed in a form" = at least one aimed source whose parse in that form (tests/test_emu_dfast.py's entry points) differs from libzstd 1.5.7's. A mutant marked equivalent must
SURVIVE every source in every form: if it is killed, the written reason was wrong.

ze_dfast_ext has its entry (emu_dfast_ext: a raw-content dictionary digested by the product's kernels, sources above the attach cutoff) and its mutants. The attach-mode
dictionary forms (ze_dfast_dict, ze_dfast_dict_flat) have no sequence-level entry and no mutants here: they are compared as whole frames (test_dictionary_forms_on_whole_frames).

Each mutant is run against the family AIMED at it alone (family_of): step_sources for the step decisions, end_sources for ilimit, insertion_sources for the insertions,
equal_cell_sources for the forwarding, and so on -- a family that lost its aim fails its mutant even where another source would have killed it.

The first source of its family that kills each (a full run here; flat = every flat and block form named, serial = ze_dfast and ze_dfast_g):
  flat / serial step < 5: "step 4 lead 0 first from pad + 0"; step < 3: "step 3 lead 0 first from pad + 0"; step raised late / every 257: "step 2 lead 0 inner from pad + 0"
  flat / serial `ip <= ilimit` -> `<`: "end 18 rep -8"; flat loop exit `>` -> `>=`: "end 23 chain -8"; serial loop `<=` -> `<`: "end 18 rep -8"; last probe dropped: "end 20 late -9"
  equal long match a step ahead: "short 10 then long 10 pad 0"; catch-up short of position 0: "catch-up of 1"
  insertions dropped: "insertion curr+2 long", "insertion curr+2 short", "insertion end-2" (ip - 2 and ip - 1: the decoy's short cell), "insertion rep long" (both of the loop's)
  forwarding dropped: long "alphabet of 3, 3001", short "alphabet of 2, 64"; off1 > 1: "alphabet of 2, 64"; off2 > 1: "second offset empty at the start"
  parked offset not restored: "first block with none match, second opens with the first offset" (the repeat offsets handed on, compared as numbers)
  the lowest index: `idxl1 >= LOW` "long candidate one step ahead at the lowest index"; `idxl0 > LOW` and `idxs0 > LOW` "long candidate at the lowest index"
  ze_dfast_ext: step "ext: step 1 lead 0 inner from pad + 0"; ilimit "ext: end 4095 rep -8", "ext: end 4095 late -9"; insertions "ext: insertion curr+2 short", "ext: insertion end-2",
  "ext: insertion rep long", "ext: step 2 lead 0 first from pad + 0", "ext: alphabet of 2, 777" (which also kills the long cell of ip + 1 and the refused short match)

As a program -- python -m tests.dfast_mutants LIBRARY FORMS [FAMILY] -- it runs the aimed sources (of one family) against one built library and prints, as JSON, {form: the first source that kills it}."""
import json
import sys

FLAT = ("flat2", "flat3", "flat4")
BLK = ("blocks2", "blocks4")
SERIAL = ("serial", "g")
EXT = ("ext",)

# ze_dfast_ext shares lines with ze_dfast_dict: its patches carry the lines around them, up to one only it has (the repeat-offset test `off2 <= ip - DS`)
_EXT_INS = ("if (ip <= ilimit) {\n                const uint32_t ins = curr + 2;\n                hashLong[ze_hash(ZE_SRC(ins), hl, 8)] = ins;\n"
            "                hashLong[ze_hash(ZE_SRC(ip - 2), hl, 8)] = ip - 2;\n                hashSmall[ze_hash(ZE_SRC(ins), hs, mls)] = ins;\n"
            "                hashSmall[ze_hash(ZE_SRC(ip - 1), hs, mls)] = ip - 1;\n                while (ip <= ilimit) {\n                    const uint32_t rep2 = ip - off2;\n"
            "                    if (!((((uint32_t)((CE - 1) - rep2) >= 3) & (off2 <= ip - DS))")
_EXT_REP = ("& (off2 <= ip - DS)) && ze_sp_rd32(sp, rep2) == zh_ld32(ZE_SRC(ip)))) break;\n                    const uint32_t r = ze_sp_count(sp, ip + 4, rep2 + 4) + 4;\n"
            "                    const uint32_t t = off2; off2 = off1; off1 = t;\n                    ZE_STORE(0, 1, r);\n"
            "                    hashSmall[ze_hash(ZE_SRC(ip), hs, mls)] = ip;\n                    hashLong[ze_hash(ZE_SRC(ip), hl, 8)] = ip;")

MUTANTS = [
    # ---- ze_dfast_flat_np
    ("flat: long cell of ip + step written up to step 4", "if (stepP < 4) hashLong[hl1] = newL1;", "if (stepP < 5) hashLong[hl1] = newL1;", FLAT + BLK),
    ("flat: long cell of ip + step written up to step 2", "if (stepP < 4) hashLong[hl1] = newL1;", "if (stepP < 3) hashLong[hl1] = newL1;", FLAT + BLK),
    ("flat: no insertions behind a match that ends at ilimit", "if (ip <= ilimit) {\n                const uint64_t wI", "if (ip < ilimit) {\n                const uint64_t wI", FLAT + BLK),
    ("flat: repeat-offset loop leaves at ilimit", "if (ip > ilimit) break;\n                    wr = zh_ld64(src + ip); r2 = zh_ld32(src + ip - off2);", "if (ip >= ilimit) break;\n                    wr = zh_ld64(src + ip); r2 = zh_ld32(src + ip - off2);", FLAT + BLK),
    ("flat: a speculative probe whose successor is ilimit is not real", "if (R == (uint32_t)k && pos[k + 1] <= ilimit) R", "if (R == (uint32_t)k && pos[k + 1] < ilimit) R",
     "equivalent: R only says how many of a trip's probes are examined in THIS trip. A probe cut off here is probe 0 of the next trip (`pos[1] > ilimit` lets it in, its long "
     "cell and candidate are carried in cellL0 / pl0 / cl0, its step and nextStep in st / nx), where it sees the same tables: the trips are cut differently, the probes are the same"),
    ("flat: long candidate one step ahead at position 0", "if (found == 3 && pl1 && idxl1 > 2 && cl1 == w1)", "if (found == 3 && pl1 && idxl1 >= 2 && cl1 == w1)",
     "equivalent: a cell holds position + 2, and position 0 is never inserted (the search starts at 1, in the block form too when the block starts the frame), so no cell ever holds 2; "
     "the lowest index is above the first byte only in ze_dfast_g under a window, where the same flip is killed below"),
    ("flat: step raised one probe late", "if (pos[k + 1] >= nx[k]) { st[k + 1]++;", "if (pos[k + 1] > nx[k]) { st[k + 1]++;", FLAT + BLK),
    ("flat: step raised every 257 bytes", "if (fresh) { step = 1; nextStep = ip + 256; }", "if (fresh) { step = 1; nextStep = ip + 257; }", FLAT + BLK),
    ("flat: an equal long match one step ahead taken", "if (l1 > mLength) { ipm = ipP1;", "if (l1 >= mLength) { ipm = ipP1;", FLAT + BLK),
    ("flat: last probe dropped", "if (pos[1] > ilimit) break;", "if (pos[1] >= ilimit) break;", FLAT + BLK),
    ("flat: insertion of curr + 2, long, dropped", "hashLong[qI >> shL] = (pI + 2) | ZE_TL(qI);", ";", FLAT + BLK),
    ("flat: insertion of curr + 2, short, dropped", "hashSmall[ZE_PS(wI) >> shS] = (pI + 2) | ZE_TS(wI);", ";", FLAT + BLK),
    ("flat: insertion of ip - 2 dropped", "hashLong[qE >> shL] = ip | ZE_TL(qE);", ";", FLAT + BLK),
    ("flat: insertion of ip - 1 dropped", "hashSmall[ZE_PS(wE1) >> shS] = (ip + 1) | ZE_TS(wE1);", ";", FLAT + BLK),
    ("flat: repeat-offset loop's short insertion dropped", "hashSmall[ZE_PS(wr) >> shS] = (ip + 2) | ZE_TS(wr);", ";", FLAT + BLK),
    ("flat: repeat-offset loop's long insertion dropped", "hashLong[qr >> shL] = (ip + 2) | ZE_TL(qr);", ";", FLAT + BLK),
    ("flat: catch-up stops one byte short of position 0", "while (ipm > anchor && mpos > 0) {                      // catch up (zstd.c:31182", "while (ipm > anchor && mpos > 1) {                      // catch up (zstd.c:31182", FLAT + BLK),
    ("flat: long cells not forwarded inside a trip", "if (hl[k] == hl[j]) cL[k] = newL[j];", ";", FLAT + BLK),
    ("flat: short cells not forwarded inside a trip", "if (k < NP && hs[k < NP ? k : 0] == hs[j]) cS[k < NP ? k : 0] = newS[j];", ";", ("flat2", "flat3", "flat4")),
    ("flat: repeat offset at ip + 1 needs no first offset", "fnd[k] = (off1 > 0 && rp[k] ==", "fnd[k] = (off1 > 1 && rp[k] ==", FLAT),
    ("flat: second repeat offset of 1 ignored", "while (off2 > 0 && (uint32_t)wr == r2) {", "while (off2 > 1 && (uint32_t)wr == r2) {", FLAT),
    # ---- the block form's entry and exit
    ("block: parked second offset not restored", "rep[0] = off1 ? off1 : saved1; rep[1] = off2 ? off2 : saved2;\n    }\n    return nseq;", "rep[0] = off1 ? off1 : saved1; rep[1] = off2;\n    }\n    return nseq;", BLK),
    ("block: second offset not parked", "if (off2 > ip) { saved2 = off2; off2 = 0; }", "if (off2 > ip + 8) { saved2 = off2; off2 = 0; }",
     "equivalent: only a frame's first block can park (ip = 1 against the 4 of {1, 4}). An unparked 4 lives until the first match: one from the tables overwrites it (off2 = off1); one "
     "at the first repeat offset (1: a run of one byte, four or more long) is followed by the loop's test at offset 4 -- against the run's own bytes, which would have made the run longer; and with "
     "no match at all the exit writes the same 4 back"),
    # ---- ze_dfast_g (ze_dfast is ze_dfast_g over one block)
    ("serial: long cell of ip + step written up to step 4", "if (step < 4) hashLong[hl1] = (uint32_t)(ip1 - base);", "if (step < 5) hashLong[hl1] = (uint32_t)(ip1 - base);", SERIAL),
    ("serial: long cell of ip + step written up to step 2", "if (step < 4) hashLong[hl1] = (uint32_t)(ip1 - base);", "if (step < 3) hashLong[hl1] = (uint32_t)(ip1 - base);", SERIAL),
    ("serial: no insertions behind a match that ends at ilimit", "        }\n        ip += mLength; anchor = ip;\n        if (ip <= ilimit) {\n            const uint32_t ins = curr + 2;\n            hashLong[ze_hash(base + ins, hl, 8)] = ins;\n            hashLong[ze_hash(ip - 2, hl, 8)] = (uint32_t)(ip - 2 - base);\n            hashSmall[ze_hash(base + ins, hs, mls)] = ins;\n            hashSmall[ze_hash(ip - 1, hs, mls)] = (uint32_t)(ip - 1 - base);\n            while (ip <= ilimit && off2 > 0 && zh_ld32(ip)",
     "        }\n        ip += mLength; anchor = ip;\n        if (ip < ilimit) {\n            const uint32_t ins = curr + 2;\n            hashLong[ze_hash(base + ins, hl, 8)] = ins;\n            hashLong[ze_hash(ip - 2, hl, 8)] = (uint32_t)(ip - 2 - base);\n            hashSmall[ze_hash(base + ins, hs, mls)] = ins;\n            hashSmall[ze_hash(ip - 1, hs, mls)] = (uint32_t)(ip - 1 - base);\n            while (ip <= ilimit && off2 > 0 && zh_ld32(ip)", SERIAL),
    ("serial: repeat-offset loop leaves at ilimit", "while (ip <= ilimit && off2 > 0 && zh_ld32(ip) == zh_ld32(ip - off2)) {", "while (ip < ilimit && off2 > 0 && zh_ld32(ip) == zh_ld32(ip - off2)) {", SERIAL),
    ("serial: last probe dropped", "        } while (ip1 <= ilimit);\n        if (!found) break;\n        if (found == 2) {\n            off2 = off1; off1 = offset;\n            if (step < 4)", "        } while (ip1 < ilimit);\n        if (!found) break;\n        if (found == 2) {\n            off2 = off1; off1 = offset;\n            if (step < 4)", SERIAL),
    ("serial: step raised one probe late", "            if (ip1 >= nextStep) { step++; nextStep += 256; }\n            ip = ip1; ip1 += step;\n            hl0 = hl1; idxl0 = idxl1;\n        } while (ip1 <= ilimit);\n        if (!found) break;\n        if (found == 2) {\n            off2 = off1; off1 = offset;\n            if (step < 4)",
     "            if (ip1 > nextStep) { step++; nextStep += 256; }\n            ip = ip1; ip1 += step;\n            hl0 = hl1; idxl0 = idxl1;\n        } while (ip1 <= ilimit);\n        if (!found) break;\n        if (found == 2) {\n            off2 = off1; off1 = offset;\n            if (step < 4)", SERIAL),
    ("serial: an equal long match one step ahead taken", "if (l1 > mLength) { ip = ip1; mLength = l1; offset = (uint32_t)(ip - m1); m = m1; }", "if (l1 >= mLength) { ip = ip1; mLength = l1; offset = (uint32_t)(ip - m1); m = m1; }", SERIAL),
    ("serial: long candidate one step ahead at the lowest index", "if (idxl1 > LOW && zh_ld64(base + idxl1) == zh_ld64(ip1)) {", "if (idxl1 >= LOW && zh_ld64(base + idxl1) == zh_ld64(ip1)) {", ("g",)),
    ("serial: short candidate at the lowest index refused", "if (idxs0 >= LOW && zh_ld32(base + idxs0) == zh_ld32(ip)) {", "if (idxs0 > LOW && zh_ld32(base + idxs0) == zh_ld32(ip)) {", ("g",)),
    ("serial: long candidate at the lowest index refused", "if (idxl0 >= LOW && zh_ld64(base + idxl0) == zh_ld64(ip)) {", "if (idxl0 > LOW && zh_ld64(base + idxl0) == zh_ld64(ip)) {", ("g",)),
    ("serial: parked second offset not restored", "    if (saved1 != 0 && off1 != 0) saved2 = saved1;\n    rep[0] = off1 ? off1 : saved1; rep[1] = off2 ? off2 : saved2;\n    return nseq;\n}\nZH_DEV uint32_t ze_dfast(",
     "    if (saved1 != 0 && off1 != 0) saved2 = saved1;\n    rep[0] = off1 ? off1 : saved1; rep[1] = off2;\n    return nseq;\n}\nZH_DEV uint32_t ze_dfast(", ("g",)),
    # ---- ze_dfast_ext (the table-copy mode against a dictionary)
    ("ext: step grows every 128 bytes", "} else { ip += ((ip - anchor) >> 8) + 1; continue; }\n                off2 = off1; off1 = offset;\n                ZE_STORE(ip - anchor, offset + 3, mLength);", "} else { ip += ((ip - anchor) >> 7) + 1; continue; }\n                off2 = off1; off1 = offset;\n                ZE_STORE(ip - anchor, offset + 3, mLength);", EXT),
    ("ext: long cell of ip + 1 behind a short match dropped", "hashLong[h3] = curr + 1;", ";", EXT),
    ("ext: no insertions behind a match that ends at ilimit", _EXT_INS, _EXT_INS.replace("if (ip <= ilimit) {", "if (ip < ilimit) {"), EXT),
    ("ext: repeat-offset loop leaves at ilimit", "while (ip <= ilimit) {\n                    const uint32_t rep2 = ip - off2;\n                    if (!((((uint32_t)((CE - 1) - rep2) >= 3) & (off2 <= ip - DS))", "while (ip < ilimit) {\n                    const uint32_t rep2 = ip - off2;\n                    if (!((((uint32_t)((CE - 1) - rep2) >= 3) & (off2 <= ip - DS))", EXT),
    ("ext: last probe dropped", "while (ip < ilimit) {\n            const uint32_t hSmall = ze_hash(ZE_SRC(ip), hs, mls), hLong", "while (ip + 1 < ilimit) {\n            const uint32_t hSmall = ze_hash(ZE_SRC(ip), hs, mls), hLong", EXT),
    ("ext: insertion of curr + 2, long, dropped", _EXT_INS, _EXT_INS.replace("hashLong[ze_hash(ZE_SRC(ins), hl, 8)] = ins;", ";"), EXT),
    ("ext: insertion of curr + 2, short, dropped", _EXT_INS, _EXT_INS.replace("hashSmall[ze_hash(ZE_SRC(ins), hs, mls)] = ins;", ";"), EXT),
    ("ext: insertion of ip - 2 dropped", _EXT_INS, _EXT_INS.replace("hashLong[ze_hash(ZE_SRC(ip - 2), hl, 8)] = ip - 2;", ";"), EXT),
    ("ext: insertion of ip - 1 dropped", _EXT_INS, _EXT_INS.replace("hashSmall[ze_hash(ZE_SRC(ip - 1), hs, mls)] = ip - 1;", ";"), EXT),
    ("ext: repeat-offset loop's short insertion dropped", _EXT_REP, _EXT_REP.replace("hashSmall[ze_hash(ZE_SRC(ip), hs, mls)] = ip;", ";"), EXT),
    ("ext: repeat-offset loop's long insertion dropped", _EXT_REP, _EXT_REP.replace("hashLong[ze_hash(ZE_SRC(ip), hl, 8)] = ip;", ";"), EXT),
    ("ext: short match refused", "} else if (matchIndex > DS && ze_sp_rd32(sp, matchIndex) == zh_ld32(ZE_SRC(ip))) {\n                    const uint32_t h3", "} else if (matchIndex > CE && ze_sp_rd32(sp, matchIndex) == zh_ld32(ZE_SRC(ip))) {\n                    const uint32_t h3", EXT),
]


def apply(text, old, new):
    """the header with the one place changed; None when `old` is not there exactly once (the list is stale)"""
    if text.count(old) != 1: return None
    return text.replace(old, new)


def family_of(name):
    """the family of tests/dfast_sources.py that is AIMED at a mutant, by the mutant's name: the mutants test runs that family alone, so a generator that lost its aim is
    noticed even where some other source happens to kill the mutant too. None: every family runs (the mutants marked equivalent)."""
    if name.startswith("ext:"): return "ext_sources"
    what = name.split(": ", 1)[1]
    if "lowest index" in what: return "lowest_index_sources"
    if "parked" in what: return "block_sources"
    if what.startswith("long cell of ip + step") or what.startswith("step raised"): return "step_sources"
    if "ilimit" in what or "last probe" in what: return "end_sources"
    if "insertion" in what: return "insertion_sources"
    if "equal long match" in what: return "candidate_sources"
    if "catch-up" in what: return "catch_up_sources"
    if "forwarded" in what or "needs no first offset" in what: return "equal_cell_sources"
    if "second repeat offset" in what: return "repeat_offset_sources"
    return None


def kills(library, forms, family=None):
    """{form: name of the first aimed source whose parse differs from libzstd's}, over one family or all of them; stops as soon as every form in `forms` has one (forms = all
    of them: runs everything)"""
    from tests import dfast_sources as ds
    from tests.dfast_check import FORMS, Emu, Lz, differences
    lz, emu = Lz(), Emu(library)
    want = set(forms)
    run_all = want == set(FORMS)
    out = {}
    cases = [c for fam in (ds.FAMILIES if family is None else (family,)) for c in getattr(ds, fam)()]
    if family is not None and any(c.expect or c.absent for c in cases):
        cases = [c for c in cases if c.expect or c.absent or c.last is not None]          # of a family with properties, only the sources that assert one: the aimed ones
    cases.sort(key=lambda c: len(c.raw) > 8192)                   # the small ones first
    for c in cases:
        for d in differences(c, lz, emu, [f for f in (FORMS if run_all else forms) if f not in out]):
            out.setdefault(d[0], c.name)
        if not run_all and want <= set(out): break
    return out


if __name__ == "__main__":
    print(json.dumps(kills(sys.argv[1], sys.argv[2].split(","), sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] != "all" else None)))
