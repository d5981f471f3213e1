"""The level-5 compress step (greedy strategy, row match finder: the lane-serial greedy match kernel) beside level 3 on the same sources, device-resident, 128 KiB sources;
libzstd level 5 on the host's threads over the same sources (oracle/zo_mtbench.c); and the compressed-size ratio of level 5 to level 3, which is what a caller asks
level 5 for. A sample of frames of either level is compared with libzstd's.  Usage: python tests/tools/greedy_rate.py [frames]"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from zstandard_amd.device import DeviceBatchContext
from tests.corpus import Corpus
from tests import reflib
import bench

F = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
dev = torch.device("cuda", 0)
raw = Corpus(device=dev, mix="silesia").frames(0, F, chunk=256)
raw_np = raw.cpu().numpy()
ref = reflib.checker()
job = bench.Job(1, dev)
item = bench.FRAME
bound = (item + (item >> 8) + 64 + 15) & ~15
src_segs = bench.segs(np.arange(F, dtype=np.int64) * item, np.full(F, item, dtype=np.int64), dev)
dst_segs = bench.segs(np.arange(F, dtype=np.int64) * bound, np.full(F, bound, dtype=np.int64), dev)
out = {"frames": F}
total = {}
for level in (5, 3):
    n = min(F, 128)
    want = [ref.compress(raw_np[i].tobytes(), level=level) for i in range(n)]
    ctx = DeviceBatchContext(level=level)
    dst = torch.zeros(F * bound, dtype=torch.uint8, device=dev); osz = torch.zeros(F, dtype=torch.int64, device=dev); st = torch.zeros(F, dtype=torch.int32, device=dev)
    el, kt = job.timed(lambda: ctx.compress(raw.reshape(-1), src_segs, dst, dst_segs, osz, st), ctx, bench.ENC_KERNELS, 2, 1)
    assert int(st.abs().max().item()) == 0
    sizes = osz.cpu().numpy(); o = dst.view(F, bound)[:n].cpu().numpy()
    assert all(o[i, : sizes[i]].tobytes() == want[i] for i in range(n)), "level %d: frames differ from libzstd's" % level
    total[level] = float(sizes.sum())
    out["level_%d" % level] = {"ms": round(el / 2 * 1e3, 1), "GBps": round(F * item * 2 / el / 1e9, 2), "ratio": round(F * item / total[level], 3),
                              "kernels": {ctx.kernel_name(k).replace("zhip_encode_", "").replace("_kernel", ""): round(v[0], 2) for k, v in kt.items() if v[1]}}
    ctx.close(); del dst
out["compressed_size_level5_over_level3"] = round(total[5] / total[3], 4)
# libzstd level 5 on this host's threads (native threads, one context each, contiguous partition), median of three passes
threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or len(os.sched_getaffinity(0))
ns = min(F, 4096)
offs = np.arange(ns + 1, dtype=np.uint64) * np.uint64(item)
blob = np.ascontiguousarray(raw_np[:ns])
times = (C.c_double * 3)()
best = bench._mtbench().zo_mt_bench_dict(reflib.REF_SO.encode(), 0, blob.ctypes.data, offs.ctypes.data, ns, 0, 5, threads, 3, None, 0, times)
assert best > 0, "native CPU baseline failed (%r)" % best
out["libzstd_level_5_host"] = {"GBps": round(ns * item / sorted(times)[1] / 1e9, 3), "threads": threads, "frames": ns}
print(json.dumps(out))
