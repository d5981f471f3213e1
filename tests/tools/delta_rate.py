"""The delta filter of typed seekable streams beside the unfiltered typed stream, in one process on one GPU, groups of 131 072 elements.
Everything is device-resident, warmed, and timed with device events around the call; alternating repetitions, medians.

  kernels   planes_split against planes_split(filter="delta"), planes_join against the delta join's three launches, of SIZE random bytes for element sizes 2,
            4 and 8, next to a device-to-device copy_ of the same bytes: five alternating repetitions
  streams   int64 running sums of uniform [0, 1000) and int32 sorted ids drawn from [0, 2^31), SIZE bytes each, at level 3 and under match_finder="none":
            compress, whole read and 256 random reads of 1 MiB without and with the filter in three alternating pairs, and the stream sizes; every read of
            the last repetition is compared with the source
  held      (--section held, also what --root PARENT_TREE runs on a tree from before the filter) the UNFILTERED typed compress and whole read of SIZE bytes
            of bf16 N(0, 0.02) weights: the figures an existing caller sees, for a parent / this build comparison in alternating processes

One JSON line per section on stdout and, with --out FILE, appended to that file.
Usage: python tests/tools/delta_rate.py [--size BYTES] [--section kernels,streams,held] [--root TREE] [--out FILE]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1 << 30)
ap.add_argument("--section", default="kernels,streams")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--label", default="this build")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, args.root)
import numpy as np
import torch
from zstandard_amd.device import DeviceBatchContext, SeekableStream

G = 131072
SIZE = args.size // (8 * G) * (8 * G)
assert SIZE > 0, "at least one group of 8-byte elements"
sections = args.section.split(",")
dev = torch.device("cuda", 0)
lines = []


def emit(section, body):
    body = dict(section=section, label=args.label, bytes=SIZE, device=torch.cuda.get_device_name(0), **body)
    lines.append(json.dumps(body)); print(lines[-1], flush=True)


def by_events(pairs, reps):
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


if "kernels" in sections:
    ctx = DeviceBatchContext(level=3)
    src = torch.randint(0, 256, (SIZE,), dtype=torch.uint8, device=dev)
    planar = torch.empty_like(src); filtered = torch.empty_like(src); back = torch.empty_like(src); copied = torch.empty_like(src)
    for k in (2, 4, 8):
        r = by_events([("split", lambda: ctx.planes_split(src, G, k, out=planar)), ("split_delta", lambda: ctx.planes_split(src, G, k, out=filtered, filter="delta")),
                       ("join", lambda: ctx.planes_join(planar, G, k, out=back)), ("join_delta", lambda: ctx.planes_join(filtered, G, k, out=back, filter="delta")),
                       ("copy_", lambda: copied.copy_(src))], 5)
        assert torch.equal(back, src)
        m = r["median_ms"]
        r.update(element_size=k, split_delta_over_split=round(m["split_delta"] / m["split"], 3), join_delta_over_join=round(m["join_delta"] / m["join"], 3),
                 over_copy={n: round(v / m["copy_"], 3) for n, v in m.items()})
        emit("kernels", r)
    del planar, filtered, back, copied, src
    ctx.close()

if "streams" in sections:
    gen = torch.Generator(device=dev).manual_seed(7)
    rng = np.random.default_rng(13)

    def data_sets():
        yield "int64 running sums of uniform [0, 1000)", 8, torch.cumsum(torch.randint(0, 1000, (SIZE // 8,), device=dev, generator=gen), 0).view(torch.uint8).reshape(-1)
        yield "int32 sorted ids from [0, 2^31)", 4, torch.sort(torch.randint(0, 1 << 31, (SIZE // 4,), device=dev, generator=gen).to(torch.int32)).values.view(torch.uint8).reshape(-1)

    for name, k, data in data_sets():
        for finder in ("libzstd", "none"):
            ctx = DeviceBatchContext(level=3, match_finder=finder)
            out = {}
            r = {"data": name, "element_size": k, "match_finder": finder}
            r["compress"] = by_events([("planes", lambda: out.__setitem__("planes", ctx.seekable_compress(data, frame_size=G, element_size=k))),
                                       ("delta", lambda: out.__setitem__("delta", ctx.seekable_compress(data, frame_size=G, element_size=k, filter="delta")))], 3)
            r["stream_bytes"] = {n: int(v.numel()) for n, v in out.items()}
            r["delta_over_planes_bytes"] = round(out["delta"].numel() / out["planes"].numel(), 4)
            dst = torch.empty(SIZE, dtype=torch.uint8, device=dev)
            ranges = [(int(o), 1 << 20) for o in rng.integers(0, SIZE - (1 << 20), 256)]
            dst_r = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
            with SeekableStream(ctx, out["planes"]) as sp, SeekableStream(ctx, out["delta"]) as sd:
                assert sp.filter is None and sd.filter == "delta"
                r["whole_read"] = by_events([("planes", lambda: sp.read(out=dst)), ("delta", lambda: sd.read(out=dst))], 3)
                assert torch.equal(dst, data)
                r["ranges_256x1MiB"] = by_events([("planes", lambda: sp.read_ranges(ranges, out=dst_r)), ("delta", lambda: sd.read_ranges(ranges, out=dst_r))], 3)
                assert all(torch.equal(dst_r[i << 20:(i + 1) << 20], data[o:o + n]) for i, (o, n) in list(enumerate(ranges))[::37])
                r["delta_read_stats"] = sd.last_gather_stats
            for what in ("compress", "whole_read", "ranges_256x1MiB"):
                m = r[what]["median_ms"]
                r[what]["delta_over_planes"] = round(m["delta"] / m["planes"], 3)
            emit("streams", r)
            del dst, dst_r, out
            ctx.close()
        del data

if "held" in sections:
    ctx = DeviceBatchContext(level=3)
    data = (torch.randn(SIZE // 2, device=dev, generator=torch.Generator(device=dev).manual_seed(13)) * 0.02).to(torch.bfloat16).view(torch.uint8).reshape(-1)
    out = {}
    r = {"data": "bf16 N(0, 0.02) weights, unfiltered typed stream"}
    r["compress"] = by_events([("typed", lambda: out.__setitem__("typed", ctx.seekable_compress(data, frame_size=G, element_size=2)))], 3)
    r["stream_bytes"] = int(out["typed"].numel())
    dst = torch.empty(SIZE, dtype=torch.uint8, device=dev)
    with SeekableStream(ctx, out["typed"]) as st:
        r["whole_read"] = by_events([("typed", lambda: st.read(out=dst))], 3)
        assert torch.equal(dst, data)
    emit("held", r)
    ctx.close()

if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
