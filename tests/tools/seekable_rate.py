"""Seekable streams beside the batch calls they are made of, in one process, on F x 128 KiB of the bench corpus taken as ONE buffer (default 8 192: 1 GiB), level 3:

  compress     zhip_seekable_compress_device  against  zhip_compress_batch_device + the caller's prefix sum + zhip_compact_device on the same F sources, alternating, three pairs
  whole read   zhip_seekable_decompress_device(0, contentSize)  against  zhip_decompress_batch_device on the same frames, alternating, three pairs
  random reads 256 reads of 1 MiB at random offsets

The comparison is with the batch calls of the same build (a build without the feature cannot make a stream). What the seekable calls add is the scan, the table (an
XXH64 of every chunk where checksums are asked for) and, for compress, the compaction both sides run.  Usage: python tests/tools/seekable_rate.py [frames] [checksum 0/1]"""
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
from tests import seekable_cases as sc
import bench

F = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
CHECKSUM = int(sys.argv[2]) if len(sys.argv) > 2 else 0
dev = torch.device("cuda", 0)
item = bench.FRAME
src = Corpus(device=dev, mix="silesia").frames(0, F, chunk=256).reshape(-1)
total = F * item
ctx = DeviceBatchContext(level=3)
ctx._ensure_cparams()
L = ctx.L
stream0 = torch.cuda.current_stream().cuda_stream


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


# ---- compress
cap = L.zhip_seekable_bound(total, item, CHECKSUM)
dst = torch.zeros(cap, dtype=torch.uint8, device=dev)
size = torch.zeros(1, dtype=torch.int64, device=dev); status2 = torch.zeros(2, dtype=torch.int32, device=dev)


def seekable_compress():
    assert L.zhip_seekable_compress_device(ctx.ctx, src.data_ptr(), total, item, CHECKSUM, dst.data_ptr(), cap, size.data_ptr(), status2.data_ptr(), stream0) == 0


bound = (item + (item >> 8) + 64 + 15) & ~15
src_segs = bench.segs(np.arange(F, dtype=np.int64) * item, np.full(F, item, dtype=np.int64), dev)
slot_segs = bench.segs(np.arange(F, dtype=np.int64) * bound, np.full(F, bound, dtype=np.int64), dev)
slots = torch.zeros(F * bound, dtype=torch.uint8, device=dev); dense = torch.zeros(F * bound, dtype=torch.uint8, device=dev)
osz = torch.zeros(F, dtype=torch.int64, device=dev); st = torch.zeros(F, dtype=torch.int32, device=dev)


def batch_compress():
    ctx.compress(src, src_segs, slots, slot_segs, osz, st)
    offs = torch.cumsum(osz, 0) - osz
    assert L.zhip_compact_device(slots.data_ptr(), slot_segs.data_ptr(), osz.data_ptr(), st.data_ptr(), offs.data_ptr(), F, dense.data_ptr(), stream0) == 0


seekable_compress(); batch_compress()          # warm-up: scratch grows here
pairs = [(timed(seekable_compress), timed(batch_compress)) for _ in range(3)]
assert status2.cpu().tolist() == [0, 0] and int(st.abs().max().item()) == 0
n = int(size[0]); frames_bytes = int(osz.sum().item())
assert n == frames_bytes + 8 + F * (12 if CHECKSUM else 8) + 9 and torch.equal(dst[:frames_bytes], dense[:frames_bytes]), "the stream's frames are the batch's"
out = {"frames": F, "bytes": total, "checksum": CHECKSUM, "stream_bytes": n,
       "compress_ms": {"seekable": [round(a * 1e3, 1) for a, _ in pairs], "batch+scan+compact": [round(b * 1e3, 1) for _, b in pairs]},
       "compress_GBps": {"seekable": round(total / sorted(a for a, _ in pairs)[1] / 1e9, 2), "batch+scan+compact": round(total / sorted(b for _, b in pairs)[1] / 1e9, 2)}}

# ---- whole-stream read
stream_t = dst[:n]
sk = SeekableStream(ctx, stream_t)
assert sk.content_size == total and sk.n_frames == F
back = torch.zeros(total, dtype=torch.uint8, device=dev)


def seekable_read(offset=0, length=total):
    assert L.zhip_seekable_decompress_device(ctx.ctx, sk.handle, offset, length, back.data_ptr(), status2.data_ptr(), stream0) == 0


fsz = osz.cpu().numpy()
frame_segs = bench.segs(np.concatenate([[0], np.cumsum(fsz)[:-1]]), fsz, dev)
out_sizes = torch.zeros(F, dtype=torch.int64, device=dev)


def batch_read():
    ctx.decompress(stream_t, frame_segs, back, src_segs, out_sizes, st)


seekable_read(); batch_read()
pairs = [(timed(seekable_read), timed(batch_read)) for _ in range(3)]
seekable_read()
torch.cuda.synchronize()
assert status2.cpu().tolist() == [0, 0] and torch.equal(back, src)
out["read_ms"] = {"seekable": [round(a * 1e3, 2) for a, _ in pairs], "batch": [round(b * 1e3, 2) for _, b in pairs]}
out["read_GBps"] = {"seekable": round(total / sorted(a for a, _ in pairs)[1] / 1e9, 1), "batch": round(total / sorted(b for _, b in pairs)[1] / 1e9, 1)}

# ---- random reads of 1 MiB
rng = np.random.default_rng(8)
R = 1 << 20
offsets = [int(x) for x in rng.integers(0, total - R, size=256)]
seekable_read(offsets[0], R)


def random_reads():
    for o in offsets:
        seekable_read(o, R)


t = timed(random_reads)
seekable_read(offsets[-1], R)
torch.cuda.synchronize()
assert status2.cpu().tolist() == [0, 0] and torch.equal(back[:R], src[offsets[-1]:offsets[-1] + R])
out["random_1MiB_reads"] = {"reads": 256, "ms_per_read": round(t / 256 * 1e3, 3), "GBps": round(256 * R / t / 1e9, 2)}
sk.close(); ctx.close()
print(json.dumps(out))
