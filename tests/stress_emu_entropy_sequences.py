"""Open-ended form of tests/test_emu_entropy_sequences.py (not collected by pytest): the families of tests/entropy_families.py from other seeds, and blocks of
random sequences with random literal kinds, through the emulated loader, entropy kernel and trailer kernel against libzstd's ZSTD_compressSequences.

    python tests/stress_emu_entropy_sequences.py SEED [ROUNDS]     one round = every family from a fresh seed + 200 random blocks; stops at the first mismatch
    python tests/stress_emu_entropy_sequences.py --write-fixture   rewrites tests/golden/entropy_sequences.bin, the stand-alone emulator program's input
                                                                  (tests/emu/build_asan.sh builds that program; it needs no Python)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path: sys.path.insert(0, ROOT)

from tests import entropy_families as E      # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "entropy_sequences.bin")
KINDS = ("rle", "two", "uniform", "skew", "geom", ("alphabet", 2), ("alphabet", 129), ("alphabet", 256))


def fixture_items(ref, dicts, cases=None):
    """a few members of every family without a dictionary, sources of up to 5 000 bytes, levels and frame flags only (what the program's fixture format holds):
    (level, flags, source, packed list, status, libzstd's frame) in both forms"""
    items = []
    for c in cases if cases is not None else E.plain_families():          # (cases: E.plain_families() already built)
        cfg = c.cfg
        if cfg.params or cfg.magicless or cfg.dict_name: continue
        if c.source is None: c.build(dicts)
        if len(c.source) > 5000: continue
        if c.refused is not None:
            items.append((cfg.level, cfg.flags(), c.source, c.packed("plain"), c.refused, b"")); continue
        if c.family in ("table modes", "normalisation", "frame forms", "block verdicts") and len(items) % 5: continue      # (a fifth of the large families)
        for form in ("canonical", "plain"):
            items.append((cfg.level, cfg.flags(), c.source, c.packed(form), 0,
                          ref.compress_sequences(c.source, c.seqs, c.tail, level=cfg.level, flags=cfg.flags(), rep_search=form == "canonical")))
    return items


def fixture_bytes(ref, dicts, cases=None):
    import tempfile
    with tempfile.NamedTemporaryFile() as f:
        E.write_fixture(f.name, fixture_items(ref, dicts, cases))
        return open(f.name, "rb").read()


def random_blocks(rng, n):
    cases = []
    for i in range(n):
        count = int(rng.choice([0, 1, 2, 3, 7, 8, 9, 40, 127, 128, 300, 1200]))
        wide = rng.random() < 0.3
        seqs = E.plain_seqs(rng, count, ll=(0, 40 if wide else 6), ml=(3, 60 if wide else 8), lead=int(rng.integers(1, 80))) if count else []
        cfg = E.Config(level=int(rng.choice([-5, -1, 1, 2, 3])), checksum=bool(rng.integers(0, 2)), content_size=bool(rng.integers(0, 4)))
        cases.append(E.mk("random blocks", "block %d" % i, seqs, rng, kind=KINDS[int(rng.integers(0, len(KINDS)))], tail=int(rng.choice([0, 1, 5, 70, 2000])), cfg=cfg))
    return cases


def main(argv):
    from tests import emulib, reflib
    from tests import test_emu_entropy_sequences as T
    ref = reflib.checker()
    dicts = E.load_dicts(ROOT)
    if argv[1:] == ["--write-fixture"]:
        E.write_fixture(FIXTURE, fixture_items(ref, dicts))
        print("wrote %s (%d bytes)" % (FIXTURE, os.path.getsize(FIXTURE)))
        return 0
    seed, rounds = int(argv[1]), int(argv[2]) if len(argv) > 2 else 1 << 30
    emu = emulib.Emu()
    for r in range(rounds):
        s = seed * 1000003 + r * 101
        cases = [c for k, f in enumerate(E.PLAIN.values()) for c in f(seed=s + k)]
        cases += [c for k, (name, (d, off, reps, raw)) in enumerate(dicts.items()) for c in E.dictionary(name, len(d) - off, reps, seed=s + 50 + k, raw=raw)]
        cases += random_blocks(np.random.default_rng(s + 99), 200)
        T.reference_frames(ref, cases, dicts)
        n = T.run_cases(emu, cases, dicts)
        print("seed %d round %d: %d cases, %d kernel answers, all libzstd's" % (seed, r, len(cases), n), flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) < 2:
        print(__doc__); sys.exit(2)
    sys.exit(main(sys.argv))
