"""match_finder="auto" (ZHIP_FINDER_AUTO, python-zstandard_amd/csrc/zhip_encode_auto.hpp) restated in numpy, independent of the library: the
classifier's sample layout, its integer log2, the probe of the 4-byte hash table and the rule, in integer arithmetic throughout -- choice bytes and statistics
must equal the kernel's exactly. Also the seeded data sets the rule is judged on (against libzstd's two sizes per frame, tests/test_auto_rule.py).
tests/test_emu_auto_finder.py and tests/test_gpu_auto_finder.py check the kernels and the calls against this."""
import numpy as np

from tests import delta_model as dm
from tests import planes_model as pm

BLOCK_MAX = 131072
MIN = 64                     # below this: the search, unsampled
ALL = 8192                   # up to this: one window, the whole source
NWIN, WIN = 4, 1536          # above: NWIN windows of WIN bytes, window w at (n - WIN) * (w + 1) / NWIN
FEED, STRIDE = 4096, 8       # the stretch in front of a window that feeds the table, and at which stride
HLOG = 12                    # table cells, log2
CAP = 32                     # a candidate's length is measured up to this
SEQ_BITS = 14                # what a sequence costs beside its offset's extra bits
NUM, DEN = 1, 64             # the search where credit * DEN > literal bits * NUM
SEARCH, LITERALS = 0, 1


def log2fp(x):
    """log2 of x >= 1 in 1/256 bit: the exponent, and for the mantissa f = x / 2^e - 1 in 1/256 the polynomial f + 88 f (256 - f) / 65536"""
    x = int(x)
    e = x.bit_length() - 1
    f = ((x << 8) >> e) - 256
    return (e << 8) + f + ((88 * f * (256 - f)) >> 16)


def windows(n):
    """[(feed first, feed count, window start, window length)] of a source of 64 <= n <= 131072 bytes"""
    if n <= ALL:
        return [(0, 0, 0, n)]
    out, end = [], 0
    for w in range(NWIN):
        start = (n - WIN) * (w + 1) // NWIN
        lo = max(start - FEED, end)
        cnt = (start - lo) // STRIDE
        out.append((start - cnt * STRIDE, cnt, start, WIN))
        end = start + WIN
    return out


def classify(raw):
    """(choice, [window bytes, literal bits (1/256), credit (1/256 bit), hits]) of one source"""
    a = np.frombuffer(bytes(raw), dtype=np.uint8)
    n = a.size
    if n < MIN or n > BLOCK_MAX:
        return SEARCH, [0, 0, 0, 0]
    wins = windows(n)
    hist = np.zeros(256, dtype=np.int64)
    for _, _, s, ln in wins:
        hist += np.bincount(a[s:s + ln], minlength=256)
    total = int(hist.sum())
    lt = log2fp(total)
    bits = sum(int(c) * (lt - log2fp(c)) for c in hist if c)
    bits = max(bits, total * 256)                          # (a Huffman code spends a bit per byte at the least)
    hb = bits // total
    v = a.astype(np.uint32)
    v32 = v[:n - 3] | (v[1:n - 2] << 8) | (v[2:n - 1] << 16) | (v[3:] << 24)
    hsh = ((v32.astype(np.uint64) * 2654435761) & 0xFFFFFFFF) >> (32 - HLOG)
    table = np.zeros(1 << HLOG, dtype=np.int64)           # a cell: (position + 1) * 2 + (fed sparsely), the highest wins
    credit = hits = 0
    ks = np.arange(CAP)
    for first, cnt, s, ln in wins:
        if cnt:
            q = first + STRIDE * np.arange(cnt)
            np.maximum.at(table, hsh[q], (q + 1) * 2 + 1)
        for base in range(s, s + ln, 64):
            p = np.arange(base, min(base + 64, s + ln))
            p = p[p + 4 <= n]
            if not p.size:
                continue
            cell = table[hsh[p]].copy()                    # every lane reads before any lane publishes
            np.maximum.at(table, hsh[p], (p + 1) * 2)
            ok = cell != 0
            p, cell = p[ok], cell[ok]
            if not p.size:
                continue
            c = (cell >> 1) - 1
            lim = np.minimum(CAP, n - p)
            eq = a[np.minimum(p[:, None] + ks, n - 1)] == a[np.minimum(c[:, None] + ks, n - 1)]
            eq &= ks[None, :] < lim[:, None]
            ln_m = np.cumprod(eq, axis=1).sum(axis=1)
            for pi, ci, L, sparse in zip(p.tolist(), c.tolist(), ln_m.tolist(), (cell & 1).tolist()):
                if L < 4:
                    continue
                hits += 1
                cost = (SEQ_BITS + (pi - ci).bit_length() - 1) << 8
                lit = L * hb
                if lit > cost:
                    credit += (lit - cost) // L * (min(L, STRIDE) if sparse else 1)
    choice = SEARCH if credit * DEN > bits * NUM else LITERALS
    return choice, [total, bits, credit, hits]


# ---- the data sets (4 groups of 131 072 elements; frames of 131 072 bytes)
ELEMENTS = 4 * BLOCK_MAX


def text_frames(count=24, start=0):
    """frames start ... of the bench corpus (its "silesia" mix)"""
    from tests.corpus import Corpus
    return Corpus(frame_size=BLOCK_MAX, mix="silesia").frame_list(start, count)


def _normal(seed, n=ELEMENTS):
    return np.random.default_rng(seed).normal(0.0, 0.02, n).astype(np.float32)


def bf16_values(seed=1, n=ELEMENTS):
    return (_normal(seed, n).view(np.uint32) >> 16).astype(np.uint16)


def fp32_values(seed=1, n=ELEMENTS):
    return _normal(seed, n)


def sums_values(seed=1, n=ELEMENTS):
    return np.cumsum(np.random.default_rng(seed).integers(0, 1000, n)).astype(np.int64)


def sorted_values(seed=1, n=ELEMENTS):
    return np.sort(np.random.default_rng(seed).integers(0, 1 << 31, n)).astype(np.uint32)


def data_sets(seed=1):
    """[(name, [frame bytes])] of the table in DESIGN.md 4.2 (seed 1; another seed: other draws, and the corpus frames behind the first 24)"""
    return [("text", text_frames(24, 24 * (seed - 1))),
            ("bf16 planes", pm.planes(bf16_values(seed), 2, BLOCK_MAX)),
            ("fp32 planes", pm.planes(fp32_values(seed), 4, BLOCK_MAX)),
            ("int64 sums planes", pm.planes(sums_values(seed), 8, BLOCK_MAX)),
            ("int64 sums planes, delta", dm.planes(sums_values(seed), 8, BLOCK_MAX)),
            ("uint32 sorted planes", pm.planes(sorted_values(seed), 4, BLOCK_MAX))]


def both_sizes(ref, raw, level=3):
    """(literals only, search): libzstd's two frame sizes"""
    return len(ref.compress_sequences(raw, [], len(raw), level=level)), len(ref.compress(raw, level=level))
