"""Emulator stress of the DECODERS on frames written from explicit sequences: python tests/stress_emu_sequences.py SEED [depth].
The exhaustive sizes of tests/test_emu_sequences.py: every family of tests/seqfamilies.py generated from SEED (other literal bytes, other filler
offsets), the repeat-offset openings at `depth` (default 4: 4 096 openings behind predecessors that left other histories), and blocks of random
sequences -- lengths drawn around K3's thresholds, every literals mode, up to 3 000 sequences -- through the emulated pipeline as frames of one
block, behind a raw block in its several-block mode, and through the generic kernel. libzstd judges every frame first (a disagreement with the
executor is printed as MODEL); every valid frame must decode to the executor's bytes and every other one be refused. Runs under the
AddressSanitizer build too (ZHIP_EMU_SO, tests/emu/build_asan.sh). Not collected by pytest."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tests import emulib, reflib, seqmodel
from tests import seqfamilies as F
from tests.seqmodel import K3

emu = emulib.Emu(); ref = reflib.RefZstd(); oracle = reflib.Oracle()
seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
depth = int(sys.argv[2]) if len(sys.argv) > 2 else 4
rng = np.random.default_rng(seed)
EDGE = (0, 1, 3, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def random_block(rng, nseq, mode):
    b = F.Builder(rng).seq(int(rng.integers(1, 80)), 3, 1)
    for _ in range(nseq):
        ll = int(rng.choice(EDGE)) if rng.integers(0, 3) else int(rng.integers(0, 200))
        ml = max(3, int(rng.choice(EDGE))) if rng.integers(0, 3) else int(rng.integers(3, 900 if rng.integers(0, 8) else 6000))
        if b.pos + ll + ml > 120000: break
        k = int(rng.integers(0, 10))
        if k < 2: b.rep(ll, ml, int(rng.integers(1, 4)))
        elif k < 6:
            of = int(rng.choice(EDGE[1:]))
            b.seq(ll, ml, of if of <= b.pos + ll else 1)
        else: b.seq(ll, ml, int(rng.integers(1, b.pos + ll + 1)))
    return F.lit_variant([b.block(rest=int(rng.integers(0, 3)) * 7)], mode)


cases = []
for gen in (F.literal_runs, F.far_matches, F.near_matches, F.batch_shapes, F.slot_edges, F.invalid_frames):
    cases += gen(K3, seed=1000 * seed + len(cases))
cases += F.repeat_offsets(K3, seed=seed, depth=depth) + F.header_forms(K3, seed=seed, longest=True)
for i in range(40):
    cases.append(F.Case("random", "random block %d" % i, random_block(rng, int(rng.choice([5, 64, 65, 300, 3000])), str(rng.choice(["raw", "huf", "rle", "raw3"])))))
led = [c.with_lead() for c in cases]
t0 = time.time()
bad = 0
keep = []
for c in cases + led:
    c.build(oracle.xxh64)
    try:
        if not c.unjudged: seqmodel.check_model(ref, c.frame, c.want, c.cap)
    except AssertionError as e:
        print("MODEL", seed, c.family, "|", c.name, "|", e); bad += 1


def check(label, cs, outs, st):
    n = 0
    for c, o, s in zip(cs, outs, st):
        if (c.want is None) != (s != 0) or (c.want is not None and o != c.want):
            print(label, "MISMATCH", seed, c.family, "|", c.name, "| status", s, "| expected", "refusal: %s" % c.why if c.want is None else "%d bytes" % len(c.want)); n += 1
    return n


outs, st, nfb = emu.decompress_pipeline([c.frame for c in cases], [c.cap for c in cases], n_blocks=3, chunk=int(rng.choice([0, 7])))
bad += check("PIPELINE", cases, outs, st)
emu.set_blocks(16)
outs, st, nfb2 = emu.decompress_pipeline([c.frame for c in led], [c.cap for c in led], n_blocks=3, chunk=int(rng.choice([0, 7])))
emu.set_blocks(0)
bad += check("BLOCK-MODE", led, outs, st)
outs, st = emu.decompress_batch([c.frame for c in led], [c.cap for c in led], n_blocks=2)
bad += check("GENERIC", led, outs, st)
print("sequence stress", seed, "frames", len(cases), "+", len(led), "bad", bad, "fallback", nfb, nfb2, "%.1fs" % (time.time() - t0))
sys.exit(1 if bad or nfb2 else 0)
