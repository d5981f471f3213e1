"""Reads through a chain of xor-with-base streams beside the same results obtained by hand with the single-stream calls, in one process on one
GPU, groups of 131 072 elements, level 3. Everything is device-resident, warmed, and timed with device events around the call; alternating repetitions, medians.

  held      what profiles/r16_xor_base_rate.txt timed, again, before anything of the chain runs in the process: seekable_compress(base=) of w1 against w0 and
            the whole read and 256 reads of 1 MiB through SeekableStream(base=), bf16 and fp32, match_finder "libzstd" -- existing calls must not move
  kernels   the chain join alone on 2, 4 and 8 planar buffers of SIZE random bytes with a base, next to planes_join(base=) and a device-to-device copy_ of the
            same bytes, element sizes 2 and 4: five alternating repetitions. Traffic per element byte: nLinks planar reads + the base read + one write
  chains    versions w0 = N(0, 1) * 0.02, w(i) = w(i-1) + N(0, 1) * 0.02 * 1e-3 kept in fp32 and rounded to the storage type (bf16, fp32), SIZE bytes each; w0
            as a full unfiltered typed stream, every w(i) compressed against w(i-1). For chains of 2, 4 and 8 deltas behind the full stream: a whole read and 256
            random reads of 1 MiB (disjoint, not aligned to groups) through SeekableChain, ALTERNATED with the same results by hand -- SeekableStream(base=)
            link by link through two full-size ping-pong tensors, the ranges of every link but the last placed at their content offsets so that the next link
            finds its base bytes there. Three alternating pairs, medians; every result of the last repetition is compared with the version. Also the sizes of
            the streams: every delta against its predecessor, and the last version against w0

One JSON line per result on stdout and, with --out FILE, appended to that file.
Usage: python tests/tools/chain_rate.py [--size BYTES] [--section held,kernels,chains] [--out FILE]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1 << 30)
ap.add_argument("--section", default="held,kernels,chains")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, args.root)
import numpy as np
import torch
from zstandard_amd.device import DeviceBatchContext, SeekableChain, SeekableStream

G = 131072
MIB = 1 << 20
SIZE = args.size // (8 * G) * (8 * G)
assert SIZE >= 8 * MIB, "at least 8 MiB"
N_READS = min(256, SIZE // MIB - 1)
sections = args.section.split(",")
dev = torch.device("cuda", 0)
lines = []


def emit(section, body):
    body = dict(section=section, bytes=SIZE, device=torch.cuda.get_device_name(0), **body)
    lines.append(json.dumps(body)); print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(lines[-1] + "\n")


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


def version_steps(dtype, steps):
    """yields w0, w1, ..., w(steps) as uint8 tensors of SIZE bytes; the walk is kept in fp32"""
    gen = torch.Generator(device=dev).manual_seed(7)
    n = SIZE // torch.empty(0, dtype=dtype).element_size()
    w = torch.randn(n, device=dev, generator=gen) * 0.02
    yield w.to(dtype, copy=True).contiguous().view(torch.uint8).reshape(-1)      # (a copy: the walk goes on in place, and to() of fp32 to fp32 would alias it)
    for _ in range(steps):
        w += torch.randn(n, device=dev, generator=gen) * (0.02 * 1e-3)
        yield w.to(dtype, copy=True).contiguous().view(torch.uint8).reshape(-1)


rng = np.random.default_rng(13)
# disjoint reads of 1 MiB that start inside an element and inside a group
read_ranges = [(int(i) * MIB + 4099, MIB) for i in rng.choice(SIZE // MIB - 1, N_READS, replace=False)]

if "held" in sections:
    ctx = DeviceBatchContext(level=3)
    for name, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        w0, w1 = list(version_steps(dtype, 1))
        k = torch.empty(0, dtype=dtype).element_size()
        out = {}
        r = {"data": "%s, w1 against w0, match_finder libzstd (profiles/r16_xor_base_rate.txt, part 2, the base columns)" % name, "element_size": k}
        r["compress"] = by_events([("base", lambda: out.__setitem__("base", ctx.seekable_compress(w1, frame_size=G, element_size=k, base=w0)))], 3)
        r["stream_bytes"] = int(out["base"].numel())
        dst = torch.empty(SIZE, dtype=torch.uint8, device=dev); dst_r = torch.empty(N_READS * MIB, dtype=torch.uint8, device=dev)
        ranges = [(int(o), MIB) for o in np.random.default_rng(13).integers(0, SIZE - MIB, N_READS)]      # (that tool's ranges: they may overlap)
        with SeekableStream(ctx, out["base"], base=w0) as sb:
            r["whole_read"] = by_events([("base", lambda: sb.read(out=dst))], 3)
            assert torch.equal(dst, w1)
            r["ranges_256x1MiB"] = by_events([("base", lambda: sb.read_ranges(ranges, out=dst_r))], 3)
        emit("held", r)
        del w0, w1, dst, dst_r, out
    ctx.close()

if "kernels" in sections:
    ctx = DeviceBatchContext(level=3)
    planars = [torch.randint(0, 256, (SIZE,), dtype=torch.uint8, device=dev) for _ in range(8)]
    base = torch.randint(0, 256, (SIZE,), dtype=torch.uint8, device=dev)
    out = torch.empty(SIZE, dtype=torch.uint8, device=dev); one = torch.empty(SIZE, dtype=torch.uint8, device=dev); copied = torch.empty(SIZE, dtype=torch.uint8, device=dev)
    for k in (2, 4):
        r = by_events([("join_base", lambda: ctx.planes_join(planars[0], G, k, out=one, base=base)), ("chain_1", lambda: ctx.planes_join_chain(planars[:1], G, k, out=out, base=base)),
                       ("chain_2", lambda: ctx.planes_join_chain(planars[:2], G, k, out=out, base=base)), ("chain_4", lambda: ctx.planes_join_chain(planars[:4], G, k, out=out, base=base)),
                       ("chain_8", lambda: ctx.planes_join_chain(planars[:8], G, k, out=out, base=base)), ("copy_", lambda: copied.copy_(planars[0]))], 5)
        ctx.planes_join_chain(planars[:1], G, k, out=out, base=base)
        assert torch.equal(out, one)
        m = r["median_ms"]
        # GiB moved: nLinks planar reads + the base + the write; the join with a base moves 3, the copy 2
        r.update(element_size=k, traffic_units={"join_base": 3, "chain_1": 3, "chain_2": 4, "chain_4": 6, "chain_8": 10, "copy_": 2},
                 ms_per_unit={n: round(v / {"join_base": 3, "chain_1": 3, "chain_2": 4, "chain_4": 6, "chain_8": 10, "copy_": 2}[n], 4) for n, v in m.items()},
                 by_hand_units={"chain_2": 6, "chain_4": 12, "chain_8": 24}, by_hand_ms={"chain_%d" % n: round(n * m["join_base"], 4) for n in (2, 4, 8)})
        emit("kernels", r)
    del planars, base, out, one, copied
    ctx.close()

if "chains" in sections:
    ctx = DeviceBatchContext(level=3)
    for name, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        k = torch.empty(0, dtype=dtype).element_size()
        streams, keep, sizes_vs_first, prev, w0 = [], {}, {}, None, None
        for i, v in enumerate(version_steps(dtype, 8)):
            if i == 0:
                w0 = v
                streams.append(ctx.seekable_compress(v, frame_size=G, element_size=k))
            else:
                streams.append(ctx.seekable_compress(v, frame_size=G, element_size=k, base=prev))
                if i in (2, 4, 8):
                    keep[i] = v
                    sizes_vs_first[i] = int(ctx.seekable_compress(v, frame_size=G, element_size=k, base=w0).numel())
            prev = v
        del prev
        emit("sizes", {"data": name, "element_size": k, "full_stream_bytes": int(streams[0].numel()), "delta_vs_predecessor_bytes": [int(s.numel()) for s in streams[1:]],
                       "of_raw_vs_predecessor": [round(s.numel() / SIZE, 4) for s in streams[1:]], "version_vs_w0_bytes": sizes_vs_first,
                       "of_raw_vs_w0": {i: round(b / SIZE, 4) for i, b in sizes_vs_first.items()}})
        ping = [torch.empty(SIZE, dtype=torch.uint8, device=dev), torch.empty(SIZE, dtype=torch.uint8, device=dev)]
        dst = torch.empty(SIZE, dtype=torch.uint8, device=dev); dst_r = torch.empty(N_READS * MIB, dtype=torch.uint8, device=dev)
        at_content = [o for o, _ in read_ranges]
        for n in (2, 4, 8):
            want = keep[n]
            # by hand: link i reads into ping[i % 2] with ping[(i - 1) % 2] as its base; the last link reads into the caller's destination
            hand = [SeekableStream(ctx, streams[0])] + [SeekableStream(ctx, streams[i], base=ping[(i - 1) % 2]) for i in range(1, n + 1)]

            def whole_by_hand():
                for i, st in enumerate(hand):
                    st.read(out=dst if i == n else ping[i % 2])

            def ranges_by_hand():
                for i, st in enumerate(hand):
                    if i == n:
                        st.read_ranges(read_ranges, out=dst_r)
                    else:
                        st.read_ranges(read_ranges, out=ping[i % 2], out_offsets=at_content)

            with SeekableChain(ctx, streams[:n + 1]) as chain:
                r = {"data": name, "element_size": k, "deltas": n, "links": n + 1}
                r["whole_read"] = by_events([("chain", lambda: chain.read(out=dst)), ("by_hand", whole_by_hand)], 3)
                assert torch.equal(dst, want)
                chain.read(out=dst)
                assert torch.equal(dst, want)
                r["chain_whole_stats"] = chain.last_gather_stats
                r["ranges_256x1MiB"] = by_events([("chain", lambda: chain.read_ranges(read_ranges, out=dst_r)), ("by_hand", ranges_by_hand)], 3)
                assert all(torch.equal(dst_r[j * MIB:(j + 1) * MIB], want[o:o + ln]) for j, (o, ln) in enumerate(read_ranges))
                chain.read_ranges(read_ranges, out=dst_r)
                assert all(torch.equal(dst_r[j * MIB:(j + 1) * MIB], want[o:o + ln]) for j, (o, ln) in enumerate(read_ranges))
                r["chain_ranges_stats"] = chain.last_gather_stats
                for what in ("whole_read", "ranges_256x1MiB"):
                    m = r[what]["median_ms"]
                    r[what]["chain_over_by_hand"] = round(m["chain"] / m["by_hand"], 3)
                emit("chains", r)
            for st in hand:
                st.close()
        del streams, keep, ping, dst, dst_r, w0
    ctx.close()
