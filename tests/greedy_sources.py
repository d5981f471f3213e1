"""Sources aimed at the decision points of the greedy search with the row match finder (ze_greedy_row), shared by the host test of the search
(test_emu_greedy_row.py) and the GPU test of level 5 (test_gpu_greedy.py). Every source is 16 385 ... 131 072 bytes: the size class whose level-5 row is greedy."""
import numpy as np

LEVEL5_ROW = dict(window_log=17, chain_log=16, hash_log=17, search_log=3, min_match=4, target_length=2, strategy=3)     # ZSTD_defaultCParameters[2][5]: sources of 16 385 ... 131 072 bytes
STRATEGY_GREEDY = 3
# what the tests run: level 5 as it is, then explicit greedy parameters laid over it
PARAM_SETS = [dict()] + [dict(strategy=STRATEGY_GREEDY, search_log=s) for s in (1, 2, 3, 4)] + [dict(strategy=STRATEGY_GREEDY, min_match=m) for m in (3, 5, 6, 7)]
TAIL_SIZES = (16385, 16392, 16400, 16401)


def tail_sources(corpus):
    """text with a 40-byte match placed at the very end: the search loop stops 16 bytes before the end, a match found before that runs into the last byte"""
    text = corpus.frame_bytes(9)
    out = []
    for n in TAIL_SIZES:
        body = text[: n - 40]
        out.append(body + body[100:140])
    return out


def constant_sources():
    return [b"\x5a" * 16385, b"\x00" * 131072]


def lazy_skipping_source():
    """(lit 9 000, match 1 000), (lit 2 500, match 40), 5 000 last literals: lazy skipping entered and left twice, a catch-up backwards from a position inside the match (where skipping begins and what a pending stretch
    inserts are pinned by the sources further down: both copies here come from bytes inserted before any skipping)"""
    rng = np.random.default_rng(31)
    first = rng.bytes(6000)
    return first + rng.bytes(3000) + first[100:1100] + rng.bytes(2500) + first[1500:1540] + rng.bytes(5000)


def _first_search_at_or_after(target):
    """the first position at or after `target` that the search loop visits in a stretch without matches that starts at the source's first byte (ip = 1, step = (ip >> 8) + 1)"""
    ip = 1
    while ip < target: ip += (ip >> 8) + 1
    return ip


def skipped_region_source():
    """copies of bytes that were passed under lazy skipping: 2 100 random bytes, 6 000 random bytes B, then twelve times 2 300 random bytes and 14 bytes from inside B. Every copy
    lies where lazy skipping is on again and points at positions of which only one in `step` was inserted: libzstd finds none of them (a search that inserted every position
    would find most)"""
    rng = np.random.default_rng(34)
    head, b = rng.bytes(2100), rng.bytes(6000)
    out = head + b
    for k in range(12): out += rng.bytes(2300) + b[400 + 450 * k: 414 + 450 * k]
    return out + rng.bytes(3000)


def lazy_threshold_source():
    """where lazy skipping begins, to the position. P = the first searched position 2 048 bytes or more past the anchor: its step is 9, the first above 8, so P is the last
    position inserted with everything before it, and the next one in the tables is P + 9. After a 64-byte match has ended the skipping, Y = the 8 bytes at P + 1 ... P + 8
    (never inserted) must not be found and X = the 8 bytes at P - 7 ... P (all inserted) must. Returns (source, P, gap between Y and X)"""
    rng = np.random.default_rng(35)
    a = rng.bytes(4000)
    p = _first_search_at_or_after(2048)
    gap = 40
    return a + a[:64] + a[p + 1: p + 9] + rng.bytes(gap) + a[p - 7: p + 1] + rng.bytes(13000), p, gap


def pending_stretch_source():
    """the first 96 and the last 32 of a pending stretch longer than 384. 1 500 random bytes A, then M = A[0:600] at 1 500: found at the first searched position S >= 1 500, so the
    next search, at 2 100, has S + 1 ... 2 099 pending and inserts S + 1 ... S + 96 and 2 068 ... 2 099 only. Four 8-byte probes follow, copies of A[k:k + 8] = M[k:k + 8]: where
    1 500 + k was inserted the newest candidate is M's and the offset points into M, where it was not the offset points into A. k = the last of the 96, the first after them,
    the one before the last 32, the first of the 32. Returns (source, [(probe position, expected offset)])"""
    rng = np.random.default_rng(36)
    a = rng.bytes(1500)
    s = _first_search_at_or_after(1500)
    out = a + a[:600] + rng.bytes(20)
    probes = []
    for k, inserted in ((s + 96 - 1500, True), (567, False), (s + 97 - 1500, False), (568, True)):
        probes.append((len(out), len(out) - (1500 + k if inserted else k)))
        out += a[k: k + 8] + rng.bytes(24)
    return out + rng.bytes(15000), probes


def skip_threshold_sources():
    """the threshold itself: the same construction with M of the two lengths that leave exactly 385 and exactly 384 positions pending at the next search, and one probe at M's
    middle -- skipped at 385 (the offset points into A), inserted with everything else at 384 (into M). Returns [(source, probe position, expected offset)] for 385, 384"""
    out = []
    s = _first_search_at_or_after(1500)
    for pending in (385, 384):
        rng = np.random.default_rng(38)
        a = rng.bytes(1500)
        m = pending + s + 1 - 1500
        src = a + a[:m] + rng.bytes(20)
        k = 200
        pos = len(src)
        src += a[k: k + 8] + rng.bytes(16000)
        out.append((src, pos, pos - (k if pending > 384 else 1500 + k)))
    return out


def last_position_source(corpus):
    """the repeat-offset loop at ip == ilimit (its test is `<=`, the main loop's `<`): a match ends exactly 16 bytes before the end and the 12 bytes there repeat at the offset
    before last. Returns the source; libzstd ends with (litLength 0, matchLength 12) and 4 last literals"""
    rng = np.random.default_rng(37)
    text = corpus.frame_bytes(9)[:16300]
    r = rng.bytes(300)
    return text + r + r[20:50] + rng.bytes(10) + r[100:130] + r[90:102] + rng.bytes(4)


GRAM_COUNT = 40


def full_row_sources():
    """one 4-byte gram 40 times, 64 bytes apart: its row fills, wraps past slot 0 and holds more equal tags than a search may visit. Second source: after the gram a
    shared prefix of 0 ... 5 bytes and then a byte of the occurrence's own, so that candidates with equal tags have different lengths, and occurrences at
    varying distances, so that the row search and not the repeat offset finds them"""
    rng = np.random.default_rng(32)
    gram, shared = b"\xc3\x17\x88\x41", b"\x90\x05\xfe\x33\x6b"
    plain = b"".join(gram + rng.bytes(60) for _ in range(GRAM_COUNT))
    varied = b"".join(gram + shared[: (k * 7) % 6] + bytes([k]) + rng.bytes(55 + (k * 5) % 11) for k in range(GRAM_COUNT))
    return [plain + rng.bytes(16384), varied + rng.bytes(16384)]


def gram_positions(raw, gram):
    return [i for i in range(2800) if raw[i:i + 4] == gram]


def repeat_offset_source():
    """records of one period with one byte changed per record: the second repeat offset hits right after a match"""
    rng = np.random.default_rng(33)
    base = bytearray(rng.bytes(72))
    out = bytearray()
    for k in range(300):
        rec = bytearray(base); rec[(k * 29) % 72] = int(rng.integers(0, 256))
        if k % 7 == 3: rec = rec[:40] + bytes(rng.bytes(3)) + rec[40:]               # a shifted record: another offset comes into play, the old one returns
        out += rec
    return bytes(out)


def corpus_sources():
    """two sources of every class of tests/corpus.py at 20 000 and at 131 072 bytes"""
    import torch
    from tests.corpus import Corpus, CLASS_NAMES
    out = []
    for size in (20000, 131072):
        c = Corpus(frame_size=size, mix="silesia")
        cls = c.classes(torch.arange(400, dtype=torch.int64)).tolist()
        for k in range(len(CLASS_NAMES)):
            idx = [i for i, x in enumerate(cls) if x == k][:2]
            assert len(idx) == 2, (CLASS_NAMES[k], size)
            out += [c.frame_bytes(i) for i in idx]
    return out


def aimed_sources(corpus):
    """every aimed source, as (name, bytes)"""
    out = [("tail %d" % n, r) for n, r in zip(TAIL_SIZES, tail_sources(corpus))]
    out.append(("text 131072", corpus.frame_bytes(9)))
    out += [("constant %d" % len(r), r) for r in constant_sources()]
    out.append(("lazy skipping", lazy_skipping_source()))
    out += [("full row", full_row_sources()[0]), ("full row, varied", full_row_sources()[1])]
    out.append(("repeat offsets", repeat_offset_source()))
    out += [("skipped region", skipped_region_source()), ("lazy threshold", lazy_threshold_source()[0]), ("pending stretch", pending_stretch_source()[0]), ("pending 385", skip_threshold_sources()[0][0]), ("pending 384", skip_threshold_sources()[1][0]),
            ("last position", last_position_source(corpus))]
    out += [("corpus %d" % i, r) for i, r in enumerate(corpus_sources())]
    return out
