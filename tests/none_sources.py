"""Sources aimed at the decisions a LITERALS-ONLY frame goes through (match_finder="none": ze_none_body, ze_compress_literals and the block assembly with the whole source
as the literals and no sequences). Seeded and built with numpy only (the text is the test corpus'). Shared by tests/test_emu_none_finder.py and
tests/test_gpu_none_finder.py.

Every entry carries the PROPERTY it is there for -- what libzstd 1.5.7's own frame of it (ZSTD_compressSequences, a list that is only the block delimiter, level 3)
must say: the block type, and for a compressed block the literals type (0 raw, 1 RLE, 2 Huffman) and the stream count. The tests assert the property from libzstd's
frame before they compare anything (``check_property``), so a source that no longer aims where it should fails on its own."""
import heapq

import numpy as np

from tests import entropy_families

BLOCK_MAX = 131072
# The sizes at which a decision flips when the literals are the whole source: 7 (below it libzstd stores raw without looking), 12 (the 4-stream coder's floor), 64 (minLits
# without a previous table: below it the literals stay raw), 256 (one Huffman stream below, four from there on), 1 024 and 16 384 (literals header of 3, 4, 5 bytes),
# 40 960 (from there on the literal coder samples the first and the last 4 KiB of a block without sequences before it counts anything), the block maximum.
SIZES = (0, 1, 6, 7, 11, 12, 63, 64, 255, 256, 1023, 1024, 16383, 16384, 40959, 40960, 131071, 131072)
REFUSED_SIZE = BLOCK_MAX + 1

RAW = {"block": "raw"}


def huffman(streams, size_format=None):
    """Huffman literals in `streams` streams; size_format: the literals header's size format (0 and 1: 3 bytes, 2: 4 bytes, 3: 5 bytes)"""
    prop = {"block": "compressed", "lit_type": 2, "streams": streams}
    if size_format is not None:
        prop["lit_format"] = size_format
    return prop


RLE_LITERALS = {"block": "compressed", "lit_type": 1}


def _rng(k):
    return np.random.default_rng(7100 + k)


def text(corpus, n, frame=9):
    return corpus.frame_bytes(frame)[:n]


def random_bytes(n, k=0):
    return _rng(k).integers(0, 256, n, dtype=np.uint8).tobytes()


def two_values(n=5000):
    return np.where(_rng(20).integers(0, 4, n) == 0, 0x37, 0xC2).astype(np.uint8).tobytes()


def random_ends(corpus, n):
    """the first and the last 4 KiB random, text between: from 40 960 bytes on the two samples say "uncompressible" and libzstd stores the block raw; one byte below it
    counts the whole source and compresses it"""
    body = bytearray(text(corpus, n))
    body[:4096] = random_bytes(4096, 30); body[n - 4096:] = random_bytes(4096, 31)
    return bytes(body)


def text_ends(corpus, n=65536):
    """text in the first and the last 4 KiB, random between: the samples pass, the count of the whole source decides"""
    body = bytearray(random_bytes(n, 32))
    body[:4096] = text(corpus, 4096); body[n - 4096:] = text(corpus, 4096, frame=10)
    return bytes(body)


def skewed_256(n=65536):
    """all 256 byte values, geometrically skewed: an unlimited Huffman code of it is deeper than the 11 bits libzstd's literal tables stop at (``huffman_depth``),
    so the depth-limiting step of the table builder has work to do"""
    r = _rng(40)
    v = np.minimum(r.geometric(0.045, n) - 1, 255).astype(np.uint8)
    v[:256] = np.arange(256, dtype=np.uint8)                                 # every value at least once
    return v.tobytes()


def huffman_depth(raw):
    """depth of the deepest leaf of an unlimited Huffman code of raw's byte histogram"""
    counts = [int(c) for c in np.bincount(np.frombuffer(raw, dtype=np.uint8), minlength=256) if c]
    heap = [(c, 0) for c in counts]
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1]


def bf16_planes(n_elements=BLOCK_MAX, seed=1, std=0.02, relu=False):
    """(mantissa plane, exponent plane) of n_elements bf16 values N(0, std): the low and the high byte of float32.view(uint32) >> 16 (truncation), as the typed
    seekable stream lays them out"""
    x = np.random.default_rng(seed).normal(0.0, std, n_elements).astype(np.float32)
    if relu:
        x = np.maximum(x, 0)
    h = (x.view(np.uint32) >> 16).astype(np.uint16)
    return (h & 0xFF).astype(np.uint8).tobytes(), (h >> 8).astype(np.uint8).tobytes()


def bf16_bytes(n_elements, seed=1, std=0.02):
    """n_elements bf16 values N(0, std) as the tensor's own bytes (little-endian elements)"""
    x = np.random.default_rng(seed).normal(0.0, std, n_elements).astype(np.float32)
    return (x.view(np.uint32) >> 16).astype(np.uint16).tobytes()


def size_sources(corpus):
    """corpus text at every boundary size: [(name, bytes, property)]"""
    out = []
    for n in SIZES:
        # below 64 bytes the literals stay raw and a block of raw literals gains nothing: a raw block (the empty source: a raw block of no bytes)
        prop = RAW if n < 64 else huffman(1 if n < 256 else 4, 0 if n < 256 else 1 if n < 1024 else 2 if n < 16384 else 3)
        out.append(("text %d" % n, text(corpus, n), prop))
    return out


def kind_sources(corpus):
    mant, expo = bf16_planes()
    return [
        ("one value 7", b"\x5a" * 7, RAW),                                                # (7 bytes of RLE literals are a 4-byte block: not below 7 - minGain)
        ("one value 1000", b"\x5a" * 1000, RLE_LITERALS),
        ("one value 131072", b"\x00" * BLOCK_MAX, RLE_LITERALS),
        ("two values", two_values(), huffman(4)),
        ("random 20000", random_bytes(20000, 1), RAW),
        ("random 131072", random_bytes(BLOCK_MAX, 2), RAW),
        ("random ends 40959", random_ends(corpus, 40959), huffman(4)),
        ("random ends 40960", random_ends(corpus, 40960), RAW),
        ("random ends 65536", random_ends(corpus, 65536), RAW),
        ("text ends 65536", text_ends(corpus), RAW),                                      # (7/8 of it is random: the table of the whole count gains less than ZSTD_minGain)
        ("skewed 256 values", skewed_256(), huffman(4)),
        ("bf16 exponent plane", expo, huffman(4)),
        ("bf16 mantissa plane", mant, RAW),                                               # (the exponent's lowest bit and seven near-uniform mantissa bits)
    ]


def aimed_sources(corpus):
    """[(name, bytes, property)]: the whole aimed set in a fixed order, every source of one block"""
    return size_sources(corpus) + kind_sources(corpus)


def refused_source(corpus):
    """one byte above a block: status 40 at its own index"""
    return (corpus.frame_bytes(9) + corpus.frame_bytes(10))[:REFUSED_SIZE]


def corpus_class_sources(corpus, sizes=(20000, BLOCK_MAX), per_size=14):
    """per size the first `per_size` corpus frames that between them hold every class of the corpus twice: [(name, bytes)]"""
    import torch
    from tests.corpus import CLASS_NAMES
    cls = corpus.classes(torch.arange(0, 400, dtype=torch.int64)).tolist()
    present = sorted(set(cls))
    picks, have = [], {c: 0 for c in present}
    for i, c in enumerate(cls):
        if have[c] < 2 and len(picks) < per_size:
            picks.append(i); have[c] += 1
    i = 0
    while len(picks) < per_size:                                                           # (a class the default mix does not draw: more of the others)
        if i not in picks: picks.append(i)
        i += 1
    picks.sort()
    return [("%s %d (frame %d)" % (CLASS_NAMES[cls[i]], n, i), corpus.frame_bytes(i)[:n]) for n in sizes for i in picks]


def check_property(name, frame, prop):
    """asserts from libzstd's frame that the source aims where it is meant to"""
    got = entropy_families.frame_census(frame)
    for k, v in prop.items():
        assert got.get(k) == v, "%s: libzstd's frame says %r, the source is there for %r" % (name, got, prop)
    if got["block"] == "compressed":
        assert got["nb_seq"] == 0, (name, got)
