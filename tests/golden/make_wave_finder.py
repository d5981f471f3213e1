"""Writes tests/golden/wave_finder.json: size and SHA-256 of the frame the wave-parallel match finder (ZHIP_FINDER_WAVE) makes of each source of
tests/wave_sources.py (the small ones under "frames", the others under "all_frames") at level 3 with the default frame flags, from the host emulator's build of the kernel body (tests/emu/emu_wave_finder.cpp). The GPU test
asserts that the MI355X writes the same frames. Run from the repository root:  python tests/golden/make_wave_finder.py"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import wave_emu, wave_sources            # noqa: E402
from tests.corpus import Corpus                     # noqa: E402


def main():
    corpus = Corpus()
    srcs = wave_sources.all_sources(corpus)
    small = {name for name, _ in wave_sources.small_sources(corpus)}
    with tempfile.TemporaryDirectory() as tmp:
        lib = wave_emu.build(tmp)
        got, st = wave_emu.frames(lib, [r for _, r in srcs], level=3)
    assert not any(st), st
    rows = [dict(name=name, src_size=len(raw), src_sha256=hashlib.sha256(raw).hexdigest(), size=len(f), sha256=hashlib.sha256(f).hexdigest()) for (name, raw), f in zip(srcs, got)]
    # frames: the small sources; all_frames: the rest of the set (the large sources: the wave-wide extension, whole blocks)
    json.dump(dict(level=3, table_log=12, frames=[r for r in rows if r["name"] in small], all_frames=[r for r in rows if r["name"] not in small]),
              open(os.path.join(HERE, "wave_finder.json"), "w"), indent=1)
    print("%d frames" % len(rows))


if __name__ == "__main__":
    main()
