"""Compressed size of the wave-parallel match finder's frames against libzstd's, on the CPU: the finder's output is deterministic and the host emulator runs the
kernel's own body (tests/emu/emu_wave_finder.cpp), so the ratio needs no GPU. Sources: 256 corpus sources of 131 072 bytes and 256 of 20 000 (the sources of
tests/test_gpu_greedy.py). Prints, per size class, the total of the finder's frames at one level and table size and its ratio to libzstd's totals at levels -1, 1 and 3.
A reported number, not a pass mark. One (level, table size) per run, so that several can run side by side:
Usage: python tests/tools/wave_finder_ratio.py LEVEL HLOG [sources per class]"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import reflib, wave_emu
from tests.corpus import Corpus

level, hlog = int(sys.argv[1]), int(sys.argv[2])
N = int(sys.argv[3]) if len(sys.argv) > 3 else 256
ref = reflib.checker()
with tempfile.TemporaryDirectory() as tmp:
    lib = wave_emu.build(tmp)
    for cls, raws in (("131072", Corpus().frame_list(2000, N)), ("20000", Corpus(frame_size=20000, mix="silesia").frame_list(0, N))):
        total = 0
        for k in range(0, len(raws), 32):
            got, st = wave_emu.frames(lib, raws[k:k + 32], level=level, hlog=hlog)
            assert not any(st)
            total += sum(len(f) for f in got)
        raw_total = sum(len(r) for r in raws)
        lz = {lv: sum(len(ref.compress(r, level=lv)) for r in raws) for lv in (-1, 1, 3)}
        print("%d sources of %s bytes, wave finder level %d H=%d: %d (ratio %.3f); libzstd level -1 / 1 / 3: %d / %d / %d (ratio %.3f / %.3f / %.3f); size / libzstd's: %.4f / %.4f / %.4f" % (
            len(raws), cls, level, hlog, total, raw_total / total, lz[-1], lz[1], lz[3], raw_total / lz[-1], raw_total / lz[1], raw_total / lz[3],
            total / lz[-1], total / lz[1], total / lz[3]), flush=True)
