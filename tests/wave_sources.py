"""Sources for the wave-parallel match finder's tests (tests/test_emu_wave_finder.py, tests/test_gpu_wave_finder.py, tests/emu/wave_bounds_main.cpp through
tests/emu/build_wave_bounds.sh): every size at which the search's trips, its tail rule (no match starts in the last 7 bytes) or the dispatch change path, and contents aimed
at each part of the search -- the repeat-offset test inside a trip, the capped per-lane extension and the wave-wide one, catch-up, sequence-count pressure, colliding cells.
Seeded: the same bytes on every run."""
import numpy as np

SIZES = (0, 1, 6, 7, 8, 63, 64, 65, 127, 128, 129, 4095, 4096, 16384, 16385, 65536, 131071, 131072)
PERIODS = (1, 2, 3, 63, 64, 65, 200)
SEED = 20261019


def _rng(k):
    return np.random.default_rng(SEED + k)


def periodic(period, n, glitches=(), k=0):
    """n bytes of a random unit of `period` bytes repeated; at every position of `glitches` the byte is changed (the match running there ends and the next one resumes
    with the same offset: a repeat code)"""
    unit = _rng(1000 + 7 * period + k).integers(0, 256, period, dtype=np.uint8)
    if period > 1:
        unit[0] = unit[1] ^ 0x55                                  # (never a shorter period by accident)
    a = np.tile(unit, n // period + 1)[:n].copy()
    for g in glitches:
        a[g] ^= 0xFF
    return a.tobytes()


def half_copy(n=131072):
    """the second half copies the first: ONE match at offset n / 2, found by a lane's capped extension and finished by the whole wave"""
    h = _rng(2).integers(0, 256, n // 2, dtype=np.uint8).tobytes()
    return h + h


def match_to_the_last_byte(n=5000):
    """random bytes whose last 30 are a copy of bytes [100, 130): a match below the per-lane cap that ends exactly at the last byte"""
    a = bytearray(_rng(3).integers(0, 256, n, dtype=np.uint8).tobytes())
    a[n - 30:] = a[100:130]
    return bytes(a)


def match_past_the_end(n=5003):
    """random bytes whose last 301 are a copy of bytes [100, 401), and the history goes on behind byte 401: the match would run past the end of the source -- the
    wave-wide extension's last trip has lanes whose 8 bytes straddle the end and lanes beyond it"""
    a = bytearray(_rng(4).integers(0, 256, n, dtype=np.uint8).tobytes())
    a[n - 301:] = a[100:401]
    return bytes(a)


def four_bytes_at_the_fourth_last(n=3000):
    """random bytes whose last four are a copy of bytes [500, 504), nothing before them matches: a match there would need a load across the end -- it is literals"""
    a = bytearray(_rng(5).integers(0, 256, n, dtype=np.uint8).tobytes())
    a[n - 4:] = a[500:504]
    return bytes(a)


def far_match(n=100000):
    """random bytes whose last 5 are a copy of the first 5: a single match at offset n - 5, the largest a source admits; its loads would cross the end, so the wave
    finder leaves it as literals (libzstd finds it)"""
    a = bytearray(_rng(6).integers(0, 256, n, dtype=np.uint8).tobytes())
    a[n - 5:] = a[0:5]
    return bytes(a)


FAR_FOUND = (100000, 100000 - 72)             # (size, offset) of far_match_found


def far_match_found(n=FAR_FOUND[0]):
    """64 random bytes, zeros (ONE long match: the positions inside it are never published, so the first trip's cells survive), the 64 bytes again, 8 other bytes:
    a match at offset n - 72, which no table with fewer cells than positions would keep on a source that publishes every position"""
    a = np.zeros(n, dtype=np.uint8)
    a[:64] = _rng(9).integers(1, 256, 64, dtype=np.uint8)
    a[n - 72:n - 8] = a[:64]
    a[n - 8:] = _rng(10).integers(1, 256, 8, dtype=np.uint8)
    return a.tobytes()


def sequence_pressure(n=40000):
    """about n bytes of 4-byte matches separated by one literal: 4 bytes taken from a 256-entry table of distinct grams, then a byte that breaks the match
    (sequence-count pressure where the search takes 4-byte matches: min_match 4 -- level 3's rows ask for 5)"""
    r = _rng(7)
    grams = r.integers(0, 256, (256, 4), dtype=np.uint8)
    grams[:, 0] = np.arange(256, dtype=np.uint8)                   # distinct first bytes: distinct grams
    out = [grams.reshape(-1).tobytes()]
    order = r.integers(0, 256, n // 5)
    sep = r.integers(0, 256, n // 5, dtype=np.uint8)
    body = np.zeros((n // 5, 5), dtype=np.uint8)
    body[:, :4] = grams[order]
    body[:, 4] = sep
    out.append(body.reshape(-1).tobytes())
    return b"".join(out)


def colliding_regions(n=20000):
    """two regions whose every 4-byte window recurs with DIFFERENT bytes after it: the same 4 bytes (one hash cell) followed by different bytes, over and over -- the cell's
    candidate matches 4 bytes and no more, or belongs to the other continuation"""
    r = _rng(8)
    key = bytes(r.integers(0, 256, 4, dtype=np.uint8))
    out = bytearray()
    while len(out) < n:
        out += key + bytes(r.integers(0, 256, int(r.integers(1, 9)), dtype=np.uint8))
    return bytes(out[:n])


def text(corpus, n, frame=9):
    return corpus.frame_bytes(frame)[:n]


def random_bytes(n, k=0):
    return _rng(100 + k).integers(0, 256, n, dtype=np.uint8).tobytes()


def glitches_for(n, period):
    """a changed byte about every n / 8 bytes, never in the first two periods or the last 64 bytes"""
    return [g for g in range(max(2 * period + 70, n // 8), n - 64, n // 8)]


def all_sources(corpus):
    """[(name, bytes)]: the whole set, in a fixed order"""
    out = []
    for n in SIZES:
        out.append(("text %d" % n, text(corpus, n)))
    for n in SIZES:
        out.append(("constant %d" % n, bytes([0x41 + n % 7]) * n))
    for p in PERIODS:
        out.append(("period %d" % p, periodic(p, 20000)))
        out.append(("period %d glitched" % p, periodic(p, 20000, glitches_for(20000, p))))
    out.append(("period 3 one block", periodic(3, 131072, glitches_for(131072, 3), k=1)))
    for k, n in enumerate((64, 129, 4096, 16385, 131072)):
        out.append(("random %d" % n, random_bytes(n, k)))
    out.append(("half copy", half_copy()))
    out.append(("match to the last byte", match_to_the_last_byte()))
    out.append(("match past the end", match_past_the_end()))
    out.append(("four bytes at the fourth-last", four_bytes_at_the_fourth_last()))
    out.append(("far match", far_match()))
    out.append(("far match found", far_match_found()))
    out.append(("sequence pressure", sequence_pressure()))
    out.append(("colliding regions", colliding_regions()))
    return out


def small_sources(corpus):
    """the sources of the committed fixture (tests/golden/wave_finder.json): about two dozen of at most 20 000 bytes that between them take every path"""
    keep = {"text 7", "text 8", "text 63", "text 64", "text 65", "text 127", "text 128", "text 129", "text 4095", "text 4096", "text 16384", "text 16385",
            "constant 8", "constant 65", "constant 4096", "period 1 glitched", "period 2 glitched", "period 3 glitched", "period 63 glitched", "period 64 glitched",
            "period 65 glitched", "period 200 glitched", "random 4096", "match to the last byte", "match past the end", "four bytes at the fourth-last", "colliding regions"}
    return [(name, raw) for name, raw in all_sources(corpus) if name in keep]
