"""Cases for K3's copies by literal mode (test infrastructure for tests/test_emu_k3_literal_modes.py and tests/test_gpu_k3_literal_modes.py).

zp_exec_block exists once per literal mode (zhip_decode_pipeline.hpp, ZP_LM_*): decoded literals (Huffman, treeless), raw literals, RLE literals; the
dictionary instantiations keep one copy with the mode as a run-time value. tests/seqfamilies.py aims at every threshold of the batch loop, but only
its "literal runs" family varies the literal mode -- the other K3 families write raw literals, so they would hold their thresholds against one copy
only. Here those families (far matches, near matches, batch shape, slot edges) are taken through lit_variant in all three modes, the raw-content
dictionary family in the two modes it does not have, and two things no family has: a frame whose compressed blocks change the mode from block to
block, and one batch with the three modes' frames interleaved. Expected bytes are seqmodel.execute's, as everywhere."""
import numpy as np

from tests import seqfamilies as F
from tests.seqmodel import K3

MODES = ("raw", "huf", "rle")
FAMILIES = {"far matches": F.far_matches, "near matches": F.near_matches, "batch shape": F.batch_shapes, "slot edges": F.slot_edges}
# "4 bytes of output" has one literal: no Huffman table describes a single value, lit_variant leaves it raw
STAYS_RAW_IN_HUF = {"4 bytes of output"}
# RLE literal runs are filled, not staged as 16-byte units: far_matches' "above 128" case gets there with a long literal run (1 040 bytes) beside the far match
NOT_REACHED_IN_RLE = {"far matches": ["units in a batch: above 128"]}


def _in_mode(c, mode):
    v = F.Case(c.family, "%s [%s literals]" % (c.name, mode), F.lit_variant(c.blocks, mode), c.dict_data, c.raw_dict, c.fcs, c.checksum, c.start_reps,
               dict(c.header), c.cap, c.short_by)
    v.base_name, v.lit_mode = c.name, mode
    return v


def family_cases(mode, k=K3, families=None):
    """the four families with the literals of every compressed block in `mode`"""
    return [_in_mode(c, mode) for name, gen in FAMILIES.items() if families is None or name in families for c in gen(k)]


def block_modes(c):
    return [(b[3] if len(b) > 3 else {}).get("lit", "raw") for b in c.blocks if b[0] == "seq"]


def in_its_mode(c):
    """whether every compressed block of the case really is written in the mode it was asked for"""
    want = {"raw": ("raw",), "huf": ("huf1", "huf4"), "rle": ("rle",)}[c.lit_mode]
    return all(m in want for m in block_modes(c))


def dictionary_cases(mode, k=K3):
    return [_in_mode(c, mode) for c in F.raw_dictionaries(k)]


def changing_modes(k=K3, seed=21):
    """A frame of four compressed blocks behind a raw one: Huffman in four streams, treeless, RLE, raw. Each block opens with matches into the block
    before it (its last bytes, its middle, the frame's first bytes), runs enough batches of 64 to pass the slide mark, so the LDS history is rebuilt
    and slid in every copy inside one wave, and ends with literal runs above 16 bytes, which every copy stages its own way."""
    rng = np.random.default_rng(seed)
    lead = bytes(rng.integers(0, 256, 600, dtype=np.uint8))
    blocks, pos = [("raw", lead)], len(lead)
    per = 1024 if k.asm_bytes >= 4096 else 512
    nfill = k.hist_slide // per + 2
    table_syms = None
    for mode in ("huf4", "treeless4", "rle", "raw"):
        b = F.Builder(rng, pos)
        start = pos
        b.at(3, 20, start - 20).at(0, 5, start - 300).at(2, 40, 10).at(1, 16, start - 1)      # the first sequences reach into the previous block's output
        for _ in range(nfill): b.fill(64, per)
        b.at(2, 17, start - 40).at(1, 300, start + 100).seq(40, 6, 30).seq(100, 4, 50).seq(17, 3, 2)      # (long literal runs: units, or the RLE fill)
        blk = b.block(rest=5)
        lits = blk[1]
        if mode == "huf4": table_syms = sorted(set(lits))
        elif mode == "treeless4": lits = bytes(x if x in table_syms else table_syms[0] for x in lits)      # the inherited table has no code for other values
        elif mode == "rle": lits = bytes([lits[0] | 1]) * len(lits)
        blocks.append(("seq", lits, blk[2], {"lit": mode} if mode != "raw" else {}))
        pos = b.pos
    c = F.Case("changing modes", "Huffman, treeless, RLE and raw literals in one frame, each block reading the one before", blocks)
    c.lit_mode = "mixed"
    return [c]


def interleaved(k=K3, families=None):
    """the three modes' frames in turn (raw, huf, rle, raw, ...): a persistent wave runs one copy after the other"""
    sets = [family_cases(m, k, families) for m in MODES]
    return [c for trio in zip(*sets) for c in trio]
