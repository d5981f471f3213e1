"""Many ranges in one decode batch (zhip_seekable_decompress_ranges_device) beside a loop of single-range calls (zhip_seekable_decompress_device) of the same
build, in one process, on the stream of tests/tools/seekable_rate.py: F x 128 KiB of the bench corpus taken as ONE buffer (default 8 192: 1 GiB), level 3.

  (a) 256 random 1 MiB ranges     one call  against  256 single-range calls
  (b) 4 096 random 4 KiB records  one call at the default scratch limit, one call at a 64 MiB limit  against  4 096 single-range calls
  (c) the whole content           as one range  against  zhip_seekable_decompress_device(0, contentSize)

Times are host wall clock around the call(s) + a device synchronize, three alternating repetitions each; every result is compared with the source.
Usage: python tests/tools/seekable_gather_rate.py [frames] [checksum 0/1]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from zstandard_amd import _lib
from zstandard_amd.device import DeviceBatchContext, SeekableStream
from tests.corpus import Corpus
import bench

F = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
CHECKSUM = int(sys.argv[2]) if len(sys.argv) > 2 else 0
dev = torch.device("cuda", 0)
item = bench.FRAME
src = Corpus(device=dev, mix="silesia").frames(0, F, chunk=256).reshape(-1)
total = F * item
ctx = DeviceBatchContext(level=3)
L = ctx.L
stream0 = torch.cuda.current_stream().cuda_stream
stream_t = ctx.seekable_compress(src, frame_size=item, checksum=bool(CHECKSUM))
sk = SeekableStream(ctx, stream_t)
assert sk.content_size == total and sk.n_frames == F
status2 = torch.zeros(2, dtype=torch.int32, device=dev)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def table(ranges):
    arr = (_lib.SeekableRange * max(len(ranges), 1))()
    for k, (o, l, d) in enumerate(ranges):
        arr[k].offset, arr[k].length, arr[k].dstOffset = o, l, d
    return arr


def workload(ranges, out, limits):
    """ranges [(offset, length, dstOffset)] -> ms of three alternating repetitions of {the loop of single-range calls, one gather call per limit}"""
    arr, n = table(ranges), len(ranges)
    status = torch.zeros(2 + 2 * n, dtype=torch.int32, device=dev)
    stats = _lib.SeekableGatherStats()
    seen = {}

    def loop():
        for o, l, d in ranges:
            assert L.zhip_seekable_decompress_device(ctx.ctx, sk.handle, o, l, out.data_ptr() + d, status2.data_ptr(), stream0) == 0

    def gather(limit):
        def run():
            L.zhip_seekable_set_scratch_limit(sk.handle, limit)
            assert L.zhip_seekable_decompress_ranges_device(ctx.ctx, sk.handle, arr, n, out.data_ptr(), out.numel(), status.data_ptr(), C.byref(stats), stream0) == 0
            seen[limit] = {k: int(getattr(stats, k)) for k, _ in stats._fields_}
        return run

    def check(what):
        torch.cuda.synchronize()
        assert not status.cpu().numpy().any() and status2.cpu().tolist() == [0, 0], what
        for o, l, d in ranges[:: max(1, n // 64)] + ranges[-1:]:
            assert torch.equal(out[d:d + l], src[o:o + l]), (what, o, l)

    runs = [("loop", loop)] + [("gather@%s" % ("default" if not lim else "%dMiB" % (lim >> 20)), gather(lim)) for lim in limits]
    for name, fn in runs:                          # warm-up: scratch and pinned slots grow here
        out.zero_(); fn(); check(name)
    ms = {name: [] for name, _ in runs}
    for _ in range(3):
        for name, fn in runs:
            ms[name].append(round(timed(fn) * 1e3, 3))
    L.zhip_seekable_set_scratch_limit(sk.handle, 0)
    res = {"ms": ms, "stats": {("default" if not lim else "%dMiB" % (lim >> 20)): seen[lim] for lim in limits}}
    med = {k: sorted(v)[1] for k, v in ms.items()}
    res["median_ms"] = med
    res["loop_over_gather"] = {k: round(med["loop"] / v, 2) for k, v in med.items() if k != "loop"}
    return res


result = {"frames": F, "bytes": total, "checksum": CHECKSUM, "stream_bytes": stream_t.numel()}
rng = np.random.default_rng(9)

# (a) 256 random 1 MiB ranges
R = 1 << 20
ranges = [(int(o), R, k * R) for k, o in enumerate(rng.integers(0, total - R, size=256))]
out = torch.zeros(256 * R, dtype=torch.uint8, device=dev)
a = workload(ranges, out, [0])
a["ms_per_range"] = {k: round(v / 256, 4) for k, v in a["median_ms"].items()}
result["a_256_x_1MiB"] = a

# (b) 4 096 random 4 KiB records
R = 4096
ranges = [(int(o), R, k * R) for k, o in enumerate(rng.integers(0, total - R, size=4096))]
out = torch.zeros(4096 * R, dtype=torch.uint8, device=dev)
b = workload(ranges, out, [0, 64 << 20])
b["ms_per_range"] = {k: round(v / 4096, 5) for k, v in b["median_ms"].items()}
result["b_4096_x_4KiB"] = b
del out

# (c) the whole content as one range
back = torch.zeros(total, dtype=torch.uint8, device=dev)
result["c_whole_content"] = workload([(0, total, 0)], back, [0])
sk.close(); ctx.close()
print(json.dumps(result))
