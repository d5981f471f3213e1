"""The wave-parallel match finder (DeviceBatchContext(match_finder="wave")) beside the default finder on the same build and the same device-resident sources:
time per compress step, per-kernel time and compressed total at levels 1 and 3, the wave finder at each table size (ZHIP_WAVE_HLOG = 12, 13, 14), for
    16 384 x 128 KiB and 262 144 x 4 KiB of the bench corpora, and the small batches 1, 64 and 1 024 x 128 KiB,
and libzstd's compressed totals at levels -1, 1 and 3 for the two large batches. Every configuration is visited in two passes over the whole list (A B C ... A B C ...),
a fresh context each visit, one warm-up call and two timed steps, so that drift of the device shows as a difference between the passes, not between configurations.
Not a test: nothing is gated on the rates.
Usage: python tests/tools/wave_finder_rate.py [--out FILE] [--quick]      (--quick: an eighth of the two large batches)"""
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from zstandard_amd.device import DeviceBatchContext
from tests.corpus import Corpus
from tests import reflib
import bench

WAVE_TIMER = 10
KERNELS = bench.ENC_KERNELS + (WAVE_TIMER,)
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
quick = "--quick" in sys.argv
dev = torch.device("cuda", 0)
job = bench.Job(1, dev)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if out_path:
        open(out_path, "w").write("\n".join(lines) + "\n")


def configs():
    for level in (1, 3):
        yield ("default", level, 0)
        for h in (12, 13, 14):
            yield ("wave", level, h)


def measure(name, raw, item):
    """raw: (F, item) uint8 on the device"""
    F = raw.shape[0]
    bound = (item + (item >> 8) + 64 + 15) & ~15
    src_segs = bench.segs(np.arange(F, dtype=np.int64) * item, np.full(F, item, dtype=np.int64), dev)
    dst_segs = bench.segs(np.arange(F, dtype=np.int64) * bound, np.full(F, bound, dtype=np.int64), dev)
    dst = torch.zeros(F * bound, dtype=torch.uint8, device=dev); osz = torch.zeros(F, dtype=torch.int64, device=dev); st = torch.zeros(F, dtype=torch.int32, device=dev)
    src = raw.reshape(-1)
    say("== %s: %d x %d bytes (%.1f MiB)" % (name, F, item, F * item / 2 ** 20))
    res = {}
    for rnd in range(2):
        for finder, level, h in configs():
            if h: os.environ["ZHIP_WAVE_HLOG"] = str(h)
            else: os.environ.pop("ZHIP_WAVE_HLOG", None)
            ctx = DeviceBatchContext(level=level, match_finder="wave" if finder == "wave" else "libzstd")       # (the table size is read when the context is created)
            try:
                el, kt = job.timed(lambda: ctx.compress(src, src_segs, dst, dst_segs, osz, st), ctx, KERNELS, 2, 1)
                assert int(st.abs().max().item()) == 0, (finder, level, h)
                total = int(osz.sum().item())
                ks = {ctx.kernel_name(k).replace("zhip_encode_", "").replace("_kernel", ""): round(v[0] * v[1] / 2, 3) for k, v in kt.items() if v[1]}      # ms per step
            finally:
                ctx.close()
            res.setdefault((finder, level, h), []).append((el / 2 * 1e3, ks, total))
    for (finder, level, h), passes in res.items():
        ms = [p[0] for p in passes]
        say("%-8s level %d %s  step %9.3f ms / %9.3f ms  %7.2f GB/s  compressed %12d (ratio %.3f)  kernels ms/step %s" % (
            finder, level, ("H=%d" % h) if h else "    ", ms[0], ms[1], F * item / (min(ms) / 1e3) / 1e9, passes[0][2], F * item / passes[0][2], json.dumps(passes[-1][1])))
        assert passes[0][2] == passes[1][2], "the compressed total changed between two runs"
    del dst


def libzstd_totals(name, raw_np):
    ref = reflib.checker()
    F = raw_np.shape[0]
    for level in (-1, 1, 3):
        with ThreadPoolExecutor(16) as pool:                     # (ctypes drops the GIL)
            total = sum(pool.map(lambda i: len(ref.compress(raw_np[i].tobytes(), level=level)), range(F)))
        say("libzstd  level %2d       %s  compressed %12d (ratio %.3f)" % (level, name, total, raw_np.size / total))


say("wave_finder_rate on %s" % torch.cuda.get_device_name(0))
F128 = 16384 // (8 if quick else 1)
raw128 = Corpus(device=dev, mix="silesia").frames(0, F128, chunk=256)
for n in (1, 64, 1024):
    measure("small batch", raw128[:n].contiguous(), bench.FRAME)
measure("128 KiB batch", raw128, bench.FRAME)
libzstd_totals("128 KiB batch", raw128.cpu().numpy())
del raw128
F4 = 262144 // (8 if quick else 1)
raw4 = Corpus(frame_size=bench.DOC, device=dev).json_docs(0, F4)
measure("4 KiB batch", raw4, bench.DOC)
libzstd_totals("4 KiB batch", raw4.cpu().numpy())
