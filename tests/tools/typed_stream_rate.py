"""Typed seekable streams (one byte plane per frame) beside what they replace, in one process on one GPU, level 3, groups of 131 072 elements.

  kernels   planes_split and planes_join of SIZE random bytes for element sizes 2, 4 and 8  against  a device-to-device copy_ of the same bytes: device events
            around each call, five alternating repetitions after a warm-up, medians
  streams   on bf16 N(0, 0.02) weights and on the bench corpus viewed as uint16, SIZE bytes each: typed against plain seekable_compress (128 KiB frames), typed
            against plain whole read, 256 random ranges of 1 MiB typed against plain, and the stream sizes: host wall clock around the call + a device
            synchronize, three alternating repetitions after a warm-up; every typed read is compared with the source

One JSON line per section on stdout and, with --out FILE, in that file. Usage: python tests/tools/typed_stream_rate.py [--size BYTES] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from zstandard_amd.device import DeviceBatchContext, SeekableStream
from tests.corpus import Corpus

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1 << 30)
ap.add_argument("--out", default=None)
args = ap.parse_args()
SIZE, G = args.size // (8 * 131072) * (8 * 131072), 131072
assert SIZE > 0, "at least one group of 8-byte elements"
dev = torch.device("cuda", 0)
lines = []


def emit(section, body):
    body = dict(section=section, bytes=SIZE, device=torch.cuda.get_device_name(0), **body)
    lines.append(json.dumps(body)); print(lines[-1], flush=True)


def by_events(pairs, reps=5):
    for _, fn in pairs:
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in pairs}
    for _ in range(reps):
        for name, fn in pairs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ms[name].append(round(a.elapsed_time(b), 4))
    return {"ms": ms, "median_ms": {k: sorted(v)[len(v) // 2] for k, v in ms.items()}}


def by_clock(pairs, reps=3):
    for _, fn in pairs:
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in pairs}
    for _ in range(reps):
        for name, fn in pairs:
            torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize()
            ms[name].append(round((time.perf_counter() - t) * 1e3, 3))
    return {"ms": ms, "median_ms": {k: sorted(v)[len(v) // 2] for k, v in ms.items()}}


ctx = DeviceBatchContext(level=3)

# ---------------------------------------------------------------------------------------------- the kernels against a copy
src = torch.randint(0, 256, (SIZE,), dtype=torch.uint8, device=dev)
planar = torch.empty_like(src); back = torch.empty_like(src); copied = torch.empty_like(src)
for k in (2, 4, 8):
    r = by_events([("split", lambda: ctx.planes_split(src, G, k, out=planar)), ("join", lambda: ctx.planes_join(planar, G, k, out=back)), ("copy_", lambda: copied.copy_(src))])
    assert torch.equal(back, src)
    m = r["median_ms"]
    r.update(element_size=k, GBps={n: round(SIZE / v / 1e6, 1) for n, v in m.items()}, split_over_copy=round(m["split"] / m["copy_"], 3), join_over_copy=round(m["join"] / m["copy_"], 3))
    emit("kernels", r)
del planar, back, copied, src

# ---------------------------------------------------------------------------------------------- streams
rng = np.random.default_rng(13)


def data_sets():
    yield "bf16 N(0, 0.02) weights", (torch.randn(SIZE // 2, device=dev, generator=torch.Generator(device=dev).manual_seed(13)) * 0.02).to(torch.bfloat16).view(torch.uint8).reshape(-1)
    yield "bench corpus as uint16", Corpus(device=dev).frames(0, SIZE // 131072, chunk=256).reshape(-1)


for name, data in data_sets():
    out = {}

    def plain():
        out["plain"] = ctx.seekable_compress(data, frame_size=G)

    def typed():
        out["typed"] = ctx.seekable_compress(data, frame_size=G, element_size=2)

    r = {"data": name, "compress": by_clock([("plain", plain), ("typed", typed)])}
    r["stream_bytes"] = {k: int(v.numel()) for k, v in out.items()}
    r["typed_over_plain_bytes"] = round(out["typed"].numel() / out["plain"].numel(), 4)
    dst = torch.empty(SIZE, dtype=torch.uint8, device=dev)
    ranges = [(int(o), 1 << 20) for o in rng.integers(0, SIZE - (1 << 20), 256)]
    dst_r = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    with SeekableStream(ctx, out["plain"]) as sp, SeekableStream(ctx, out["typed"]) as st:
        assert st.element_size == 2 and sp.element_size == 1
        r["whole_read"] = by_clock([("plain", lambda: sp.read(out=dst)), ("typed", lambda: st.read(out=dst))])
        assert torch.equal(dst, data)
        r["ranges_256x1MiB"] = by_clock([("plain", lambda: sp.read_ranges(ranges, out=dst_r)), ("typed", lambda: st.read_ranges(ranges, out=dst_r))])
        assert all(torch.equal(dst_r[i << 20:(i + 1) << 20], data[o:o + n]) for i, (o, n) in list(enumerate(ranges))[::37])
        r["typed_read_stats"] = st.last_gather_stats
    for what in ("compress", "whole_read", "ranges_256x1MiB"):
        m = r[what]["median_ms"]
        r[what]["typed_over_plain"] = round(m["typed"] / m["plain"], 3)
    emit("streams", r)
    del dst, dst_r, out, data
ctx.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
