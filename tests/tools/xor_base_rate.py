"""The xor-with-base filter of typed seekable streams beside the unfiltered typed stream, in one process on one GPU, groups of 131 072 elements.
Everything is device-resident, warmed, and timed with device events around the call; alternating repetitions, medians.

  kernels   planes_split against planes_split(base=), planes_join against planes_join(base=), of SIZE random bytes (the base: other random bytes) for element
            sizes 2 and 4, next to a device-to-device copy_ of the same bytes: five alternating repetitions. With a base the kernels read twice the bytes and
            write the same
  streams   two versions of a tensor, SIZE bytes each as bf16 and as fp32: w0 = N(0, 1) * 0.02 in fp32, w1 = w0 + N(0, 1) * 0.02 * 1e-3, both rounded to the
            storage type; w1 compressed without a filter and against w0 under match_finder "libzstd" (the default), "none" and "auto" at level 3: compress,
            whole read and 256 random reads of 1 MiB in three alternating pairs, and the stream sizes; every read of the last repetition is compared with w1
  held      (--section held, also what --root PARENT_TREE runs on a tree from before the filter) the calls an existing caller makes: planes_split and
            planes_join without a filter and under "delta" (element size 4), and the unfiltered typed compress and whole read of bf16 N(0, 0.02) weights --
            for a parent / this build comparison in alternating processes

One JSON line per section on stdout and, with --out FILE, appended to that file.
Usage: python tests/tools/xor_base_rate.py [--size BYTES] [--section kernels,streams,held] [--root TREE] [--label NAME] [--out FILE]"""
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
    src = torch.randint(0, 256, (SIZE,), dtype=torch.uint8, device=dev); base = torch.randint(0, 256, (SIZE,), dtype=torch.uint8, device=dev)
    planar = torch.empty_like(src); filtered = torch.empty_like(src); back = torch.empty_like(src); back_base = torch.empty_like(src); copied = torch.empty_like(src)
    for k in (2, 4):
        r = by_events([("split", lambda: ctx.planes_split(src, G, k, out=planar)), ("split_base", lambda: ctx.planes_split(src, G, k, out=filtered, base=base)),
                       ("join", lambda: ctx.planes_join(planar, G, k, out=back)), ("join_base", lambda: ctx.planes_join(filtered, G, k, out=back_base, base=base)),
                       ("copy_", lambda: copied.copy_(src))], 5)
        assert torch.equal(back, src) and torch.equal(back_base, src)
        m = r["median_ms"]
        r.update(element_size=k, split_base_over_split=round(m["split_base"] / m["split"], 3), join_base_over_join=round(m["join_base"] / m["join"], 3),
                 over_copy={n: round(v / m["copy_"], 3) for n, v in m.items()})
        emit("kernels", r)
    del planar, filtered, back, back_base, copied, src, base
    ctx.close()

if "streams" in sections:
    rng = np.random.default_rng(13)

    def versions(dtype):
        """(w0, w1) as uint8 tensors of SIZE bytes"""
        gen = torch.Generator(device=dev).manual_seed(7)
        n = SIZE // torch.empty(0, dtype=dtype).element_size()
        w0 = torch.randn(n, device=dev, generator=gen) * 0.02
        w1 = w0 + torch.randn(n, device=dev, generator=gen) * (0.02 * 1e-3)
        return tuple(w.to(dtype).contiguous().view(torch.uint8).reshape(-1) for w in (w0, w1))

    for name, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        w0, w1 = versions(dtype)
        k = torch.empty(0, dtype=dtype).element_size()
        for finder in ("libzstd", "none", "auto"):
            ctx = DeviceBatchContext(level=3, match_finder=finder)
            out = {}
            r = {"data": "%s, w1 = w0 + N(0, 0.02 * 1e-3), w0 ~ N(0, 0.02)" % name, "element_size": k, "match_finder": finder}
            r["compress"] = by_events([("planes", lambda: out.__setitem__("planes", ctx.seekable_compress(w1, frame_size=G, element_size=k))),
                                       ("base", lambda: out.__setitem__("base", ctx.seekable_compress(w1, frame_size=G, element_size=k, base=w0)))], 3)
            r["stream_bytes"] = {n: int(v.numel()) for n, v in out.items()}
            r["of_raw"] = {n: round(v.numel() / SIZE, 4) for n, v in out.items()}
            r["base_over_planes_bytes"] = round(out["base"].numel() / out["planes"].numel(), 4)
            dst = torch.empty(SIZE, dtype=torch.uint8, device=dev)
            ranges = [(int(o), 1 << 20) for o in rng.integers(0, SIZE - (1 << 20), 256)]
            dst_r = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
            with SeekableStream(ctx, out["planes"]) as sp, SeekableStream(ctx, out["base"], base=w0) as sb:
                assert sp.filter is None and sb.filter == "xor_base"
                r["whole_read"] = by_events([("planes", lambda: sp.read(out=dst)), ("base", lambda: sb.read(out=dst))], 3)
                assert torch.equal(dst, w1)
                r["ranges_256x1MiB"] = by_events([("planes", lambda: sp.read_ranges(ranges, out=dst_r)), ("base", lambda: sb.read_ranges(ranges, out=dst_r))], 3)
                assert all(torch.equal(dst_r[i << 20:(i + 1) << 20], w1[o:o + n]) for i, (o, n) in list(enumerate(ranges))[::37])
                r["base_read_stats"] = sb.last_gather_stats
            for what in ("compress", "whole_read", "ranges_256x1MiB"):
                m = r[what]["median_ms"]
                r[what]["base_over_planes"] = round(m["base"] / m["planes"], 3)
            emit("streams", r)
            del dst, dst_r, out
            ctx.close()
        del w0, w1

if "held" in sections:
    ctx = DeviceBatchContext(level=3)
    src = torch.randint(0, 256, (SIZE,), dtype=torch.uint8, device=dev)
    planar = torch.empty_like(src); filtered = torch.empty_like(src); back = torch.empty_like(src)
    r = {"kernels": by_events([("split", lambda: ctx.planes_split(src, G, 4, out=planar)), ("split_delta", lambda: ctx.planes_split(src, G, 4, out=filtered, filter="delta")),
                               ("join", lambda: ctx.planes_join(planar, G, 4, out=back)), ("join_delta", lambda: ctx.planes_join(filtered, G, 4, out=back, filter="delta"))], 5)}
    assert torch.equal(back, src)
    del src, planar, filtered, back
    data = (torch.randn(SIZE // 2, device=dev, generator=torch.Generator(device=dev).manual_seed(13)) * 0.02).to(torch.bfloat16).view(torch.uint8).reshape(-1)
    out = {}
    r["data"] = "bf16 N(0, 0.02) weights, unfiltered typed stream"
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
