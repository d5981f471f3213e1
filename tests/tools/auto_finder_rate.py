"""match_finder="auto" (DeviceBatchContext(match_finder="auto"): a classify kernel chooses per source between the literals-only frame and the default search) beside
the two finders it chooses between, on the same build and the same device-resident data, through seekable_compress:
    (a) 1 GiB of bf16 N(0, 0.02) as a typed stream (element_size 2, groups of 131 072 elements),
    (b) 1 GiB of int64 running sums of [0, 1000) as a typed stream (element_size 8),
    (c) 16 384 x 128 KiB of the bench corpus (plain, frames of 131 072),
    (d) half of (a)'s planes and half of (c)'s frames in one plain stream,
each visited in two passes over the three finders (auto, none, libzstd, auto, none, libzstd), a fresh context each visit, one warm-up call and two timed steps, so that
drift of the device shows as a difference between the passes, not between finders. Per visit: ms per step (host clock around calls that end in a device synchronise),
the per-kernel timers (12: the classify kernel), and the stream's size. What a step of "auto" spends outside the timed kernels -- the partition, gather and scatter
kernels, the one host wait for the two counts, launch gaps -- is reported as the step less the kernel timers' sum, beside the same remainder of the pure finders'
steps: named for what it is, not a kernel time. The classify kernel alone is also timed per GiB through DeviceBatchContext.classify on (a)'s planes and on (c).
Not a test: nothing is gated on the rates.
Usage: python tests/tools/auto_finder_rate.py [--out FILE] [--quick]      (--quick: a sixteenth of every workload)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from zstandard_amd.device import DeviceBatchContext, planes_split
from tests.corpus import Corpus
import bench

KERNELS = (5, 6, 8, 11, 12)
FINDERS = ("auto", "none", "libzstd")
STEPS = 2
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
quick = "--quick" in sys.argv
dev = torch.device("cuda", 0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if out_path:
        open(out_path, "w").write("\n".join(lines) + "\n")


def visit(finder, src, frame_size, element_size):
    ctx = DeviceBatchContext(level=3, match_finder=finder)
    try:
        stream = ctx.seekable_compress(src, frame_size=frame_size, element_size=element_size)          # warm-up: reservations, the default finder's placement pick
        torch.cuda.synchronize()
        for k in KERNELS:
            ctx.kernel_time(k)
        t0 = time.perf_counter()
        for _ in range(STEPS):
            stream = ctx.seekable_compress(src, frame_size=frame_size, element_size=element_size)      # (waits for the stream's size)
        torch.cuda.synchronize()
        step_ms = (time.perf_counter() - t0) / STEPS * 1e3
        kt = {k: ctx.kernel_time(k) for k in KERNELS}
        ks = {ctx.kernel_name(k).replace("zhip_encode_", "").replace("_kernel", ""): round(v[0] * v[1] / STEPS, 3) for k, v in kt.items() if v[1]}      # ms per step
        size = int(stream.numel())
    finally:
        ctx.close()
    return step_ms, ks, size


def measure(name, src, frame_size, element_size):
    say("== %s: %d bytes (%.1f MiB), frame_size %d, element_size %d" % (name, src.numel(), src.numel() / 2 ** 20, frame_size, element_size))
    res = {}
    for rnd in range(2):
        for finder in FINDERS:
            try:
                res.setdefault(finder, []).append(visit(finder, src, frame_size, element_size))
            except Exception as e:                                                                     # noqa: BLE001 ("none" refuses nothing here; kept so one refusal does not lose the rest)
                res.setdefault(finder, []).append(None); say("%-8s %s" % (finder, e))
    for finder in FINDERS:
        a, b = res[finder]
        if a is None or b is None:
            continue
        best = a if a[0] <= b[0] else b
        say("%-8s step %9.3f ms / %9.3f ms  %7.2f GB/s  stream %12d bytes (ratio %.4f)  kernels ms/step %s  step less kernels %.3f ms" % (
            finder, a[0], b[0], src.numel() / (best[0] / 1e3) / 1e9, a[2], src.numel() / a[2], json.dumps(best[1]), best[0] - sum(best[1].values())))
    step = {f: min(r[0] for r in res[f]) for f in FINDERS if None not in res[f]}
    size = {f: res[f][0][2] for f in FINDERS if None not in res[f]}
    say("auto / none: step %.3f, size %.4f;  auto / libzstd: step %.3f, size %.4f" % (step["auto"] / step["none"], size["auto"] / size["none"], step["auto"] / step["libzstd"], size["auto"] / size["libzstd"]))


def classify_alone(name, src, frame_size):
    n = src.numel() // frame_size
    segs = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    segs[:, 0] = torch.arange(n, device=dev) * frame_size; segs[:, 1] = frame_size
    ctx = DeviceBatchContext()
    try:
        choice = ctx.classify(src, segs); torch.cuda.synchronize()
        ctx.kernel_time(12)
        t0 = time.perf_counter()
        for _ in range(5):
            choice = ctx.classify(src, segs)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / 5 * 1e3
        ms, launches = ctx.kernel_time(12)
    finally:
        ctx.close()
    gib = n * frame_size / 2 ** 30
    say("classify alone, %s: %d sources of %d bytes, %.3f ms per call by the kernel timer (%d launches a call), %.3f ms by the host clock; per GiB %.3f ms; literals only chosen for %d sources"
        % (name, n, frame_size, ms * launches / 5, launches // 5, wall, ms * launches / 5 / gib, int(choice.sum())))


say("auto_finder_rate on %s" % torch.cuda.get_device_name(0))
scale = 16 if quick else 1
gen = torch.Generator(device=dev); gen.manual_seed(1)
bf16 = (torch.randn((1 << 29) // scale, generator=gen, device=dev, dtype=torch.float32) * 0.02).to(torch.bfloat16).view(torch.uint8).reshape(-1)
sums = torch.cumsum(torch.randint(0, 1000, ((1 << 27) // scale,), generator=gen, device=dev, dtype=torch.int64), 0).view(torch.uint8).reshape(-1)
corpus = Corpus(device=dev, mix="silesia").frames(0, 16384 // scale, chunk=256).reshape(-1)
planar = planes_split(bf16, 131072, 2)
classify_alone("bf16 planes", planar, 131072)
classify_alone("bench corpus", corpus, 131072)
measure("(a) bf16 N(0, 0.02), typed", bf16, 131072, 2)
measure("(b) int64 running sums, typed", sums, 131072, 8)
measure("(c) bench corpus", corpus, bench.FRAME, 1)
mix = torch.cat([planar[:planar.numel() // 2], corpus[:corpus.numel() // 2]])
del bf16, sums, planar
measure("(d) half bf16 planes, half bench corpus", mix, 131072, 1)
