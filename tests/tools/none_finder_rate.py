"""match_finder="none" (DeviceBatchContext(match_finder="none"): literals-only frames, no match search) beside the default finder and the wave finder on the same build
and the same device-resident data, through seekable_compress:
    1 GiB of bf16 N(0, 0.02) typed (element_size 2) and plain, at frame sizes 131 072 and 4 096,
    16 384 x 128 KiB of the bench corpus (plain, frames of 131 072),
each visited in two passes over the three finders (none, libzstd, wave, none, libzstd, wave), a fresh context each visit, one warm-up call and two timed steps, so that
drift of the device shows as a difference between the passes, not between finders. Per visit: ms per step (host clock around calls that end in a device synchronise),
the per-kernel timers, the stream's size, and the time to read the whole stream back through SeekableStream.read with the context's decode_fallbacks().
Not a test: nothing is gated on the rates. The comparison that matters is "none" against the default finder's step on the same workload.
Usage: python tests/tools/none_finder_rate.py [--out FILE] [--quick]      (--quick: a sixteenth of every workload)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from zstandard_amd.device import DeviceBatchContext, SeekableStream
from tests.corpus import Corpus
import bench

KERNELS = (5, 6, 8, 10, 11)
FINDERS = ("none", "libzstd", "wave")
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
        stream = stream.clone()
        with SeekableStream(ctx, stream) as st:
            out = st.read()                                                                             # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = st.read()
            torch.cuda.synchronize()
            read_ms = (time.perf_counter() - t0) * 1e3
            same = bool(torch.equal(out, src))
        fallbacks = ctx.decode_fallbacks()
    finally:
        ctx.close()
    assert same, "the stream does not read back to the source"
    return step_ms, ks, size, read_ms, fallbacks


def measure(name, src, frame_size, element_size):
    say("== %s: %d bytes (%.1f MiB), frame_size %d, element_size %d" % (name, src.numel(), src.numel() / 2 ** 20, frame_size, element_size))
    res = {}
    for rnd in range(2):
        for finder in FINDERS:
            res.setdefault(finder, []).append(visit(finder, src, frame_size, element_size))
    for finder in FINDERS:
        a, b = res[finder]
        assert a[2] == b[2], "the stream's size changed between two runs"
        say("%-8s step %9.3f ms / %9.3f ms  %7.2f GB/s  stream %12d bytes (ratio %.4f)  read back %8.3f ms / %8.3f ms, decode fallbacks %d  kernels ms/step %s" % (
            finder, a[0], b[0], src.numel() / (min(a[0], b[0]) / 1e3) / 1e9, a[2], src.numel() / a[2], a[3], b[3], b[4], json.dumps(b[1])))
    d, n = min(r[0] for r in res["libzstd"]), min(r[0] for r in res["none"])
    say("none / libzstd: step %.3f, stream size %.4f" % (n / d, res["none"][0][2] / res["libzstd"][0][2]))


say("none_finder_rate on %s" % torch.cuda.get_device_name(0))
scale = 16 if quick else 1
gen = torch.Generator(device=dev); gen.manual_seed(1)
elements = (1 << 29) // scale
bf16 = (torch.randn(elements, generator=gen, device=dev, dtype=torch.float32) * 0.02).to(torch.bfloat16).view(torch.uint8).reshape(-1)
for frame in (131072, 4096):
    measure("bf16 N(0, 0.02), typed", bf16, frame, 2)
    measure("bf16 N(0, 0.02), plain", bf16, frame, 1)
del bf16
corpus = Corpus(device=dev, mix="silesia").frames(0, 16384 // scale, chunk=256).reshape(-1)
measure("bench corpus", corpus, bench.FRAME, 1)
