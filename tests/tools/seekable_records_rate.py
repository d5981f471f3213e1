"""One frame per record (zhip_seekable_compress_records_device, zhip_seekable_decompress_frames_device) beside the calls it is built from, in one process, on
the documents of BASELINE.json configs[3]: D JSON-like documents of 4 KiB (default 262 144: 1 GiB) taken as ONE buffer, their trained dictionary, level 3.

  compress   the records call  against  the same items through zhip_compress_batch_device + a prefix sum of the sizes + zhip_compact_device (the caller's own
             container, less its table) -- the yardstick, unchanged code
  read       4 096 random documents by zhip_seekable_decompress_frames_device from the records stream  against  the same bytes by
             zhip_seekable_decompress_ranges_device from the same content written with frame_size 131 072 (without the dictionary: the attach cutoff)
  sizes      the two streams' compressed sizes, with and without the dictionary

Times are host wall clock around the call(s) + a device synchronize, three alternating pairs each; every result is compared with the source.
Usage: python tests/tools/seekable_records_rate.py [documents]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from zstandard_amd import _lib
from zstandard_amd.backend_hip import ZstdError
from zstandard_amd.device import DeviceBatchContext, SeekableStream
from tests.corpus import Corpus

D = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
DOC = 4096
dev = torch.device("cuda", 0)
blob = open(os.path.join(ROOT, "tests", "golden", "dict_json4k.bin"), "rb").read()
src = Corpus(frame_size=DOC, device=dev).json_docs(0, D).reshape(-1)
total = D * DOC
stream0 = torch.cuda.current_stream().cuda_stream
records = torch.stack([torch.arange(D, dtype=torch.int64, device=dev) * DOC, torch.full((D,), DOC, dtype=torch.int64, device=dev)], dim=1).contiguous()


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def alternate(pairs):
    """[(name, fn)] -> ms lists of three alternating repetitions, after one warm-up each (scratch grows there), and the medians"""
    for _, fn in pairs:
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in pairs}
    for _ in range(3):
        for name, fn in pairs:
            ms[name].append(round(timed(fn) * 1e3, 3))
    return {"ms": ms, "median_ms": {k: sorted(v)[1] for k, v in ms.items()}}


result = {"documents": D, "bytes": total}

# ---------------------------------------------------------------------------------------------- compress
ctx = DeviceBatchContext(dict_data=blob, level=3)
ctx._ensure_cparams()
ctx.set_size_hint(DOC)                  # (what the batch calls are told by their caller; the records call says it itself and leaves this alone)
L = ctx.L
bound = L.zhip_seekable_records_bound(total, D, 0)
dst = torch.zeros(bound, dtype=torch.uint8, device=dev)
size = torch.zeros(1, dtype=torch.int64, device=dev)
status2 = torch.zeros(2, dtype=torch.int32, device=dev)
slot = (int(L.zhip_compress_bound(DOC)) + 15) & ~15
slots = torch.zeros(D * slot, dtype=torch.uint8, device=dev)
slot_segs = torch.stack([torch.arange(D, dtype=torch.int64, device=dev) * slot, torch.full((D,), slot, dtype=torch.int64, device=dev)], dim=1).contiguous()
out_sizes = torch.zeros(D, dtype=torch.int64, device=dev)
status = torch.zeros(D, dtype=torch.int32, device=dev)
dense = torch.zeros(bound, dtype=torch.uint8, device=dev)
offsets = torch.zeros(D, dtype=torch.int64, device=dev)


def records_call():
    assert L.zhip_seekable_compress_records_device(ctx.ctx, src.data_ptr(), total, records.data_ptr(), D, total, DOC, 0, dst.data_ptr(), bound, size.data_ptr(),
                                                   status2.data_ptr(), stream0) == 0


def batch_calls():
    assert L.zhip_compress_batch_device(ctx.ctx, src.data_ptr(), records.data_ptr(), D, slots.data_ptr(), slot_segs.data_ptr(), out_sizes.data_ptr(), status.data_ptr(), stream0) == 0
    torch.sub(torch.cumsum(out_sizes, 0), out_sizes, out=offsets)
    assert L.zhip_compact_device(slots.data_ptr(), slot_segs.data_ptr(), out_sizes.data_ptr(), status.data_ptr(), offsets.data_ptr(), D, dense.data_ptr(), stream0) == 0


c = alternate([("records", records_call), ("batch+scan+compact", batch_calls)])
assert status2.cpu().tolist() == [0, 0] and not status.cpu().numpy().any()
frames_bytes = int(out_sizes.sum())
stream_size = int(size[0])
assert stream_size == frames_bytes + 8 + 8 * D + 9 and torch.equal(dst[:frames_bytes], dense[:frames_bytes]), "the records stream is the batch's frames back to back, then the table"
c["GBps"] = {k: round(total / v / 1e6, 2) for k, v in c["median_ms"].items()}
c["spread_ms"] = {k: round(max(v) - min(v), 3) for k, v in c["ms"].items()}
c["records_over_batch"] = round(c["median_ms"]["records"] / c["median_ms"]["batch+scan+compact"], 4)
result["compress"] = c
rec_stream = dst[:stream_size].clone()
del slots, dense, dst

# ---------------------------------------------------------------------------------------------- sizes
plain = DeviceBatchContext(level=3)
sizes = {"records_dict": stream_size}
sizes["records_nodict"] = int(plain.seekable_compress_records(src, records, max_content_bytes=total, max_record_bytes=DOC).numel())
fixed_stream = plain.seekable_compress(src, frame_size=131072)
sizes["fixed128k_nodict"] = int(fixed_stream.numel())
try:
    sizes["fixed128k_dict"] = int(ctx.seekable_compress(src, frame_size=131072).numel())
except ZstdError as e:
    sizes["fixed128k_dict"] = "refused: %s" % e
sizes["ratio"] = {k: round(total / v, 3) for k, v in sizes.items() if isinstance(v, int)}
result["stream_bytes"] = sizes

# ---------------------------------------------------------------------------------------------- read
rng = np.random.default_rng(9)
pick = rng.integers(0, D, size=4096).astype(np.uint32)
n = len(pick)
out_a = torch.zeros(n * DOC, dtype=torch.uint8, device=dev)
out_b = torch.zeros(n * DOC, dtype=torch.uint8, device=dev)
st_a = torch.zeros(2 + 2 * n, dtype=torch.int32, device=dev)
st_b = torch.zeros(2 + 2 * n, dtype=torch.int32, device=dev)
stats_a, stats_b = _lib.SeekableGatherStats(), _lib.SeekableGatherStats()
sk_rec = SeekableStream(ctx, rec_stream)
sk_fix = SeekableStream(plain, fixed_stream)
assert sk_rec.n_frames == D and sk_fix.content_size == total
ranges = (_lib.SeekableRange * n)()
for k, f in enumerate(pick):
    ranges[k].offset, ranges[k].length, ranges[k].dstOffset = int(f) * DOC, DOC, k * DOC


def by_index():
    assert L.zhip_seekable_decompress_frames_device(ctx.ctx, sk_rec.handle, pick.ctypes.data, n, None, out_a.data_ptr(), out_a.numel(), st_a.data_ptr(), C.byref(stats_a), stream0) == 0


def by_range():
    assert L.zhip_seekable_decompress_ranges_device(plain.ctx, sk_fix.handle, ranges, n, out_b.data_ptr(), out_b.numel(), st_b.data_ptr(), C.byref(stats_b), stream0) == 0


r = alternate([("read_records", by_index), ("read_ranges@128KiB", by_range)])
assert not st_a.cpu().numpy().any() and not st_b.cpu().numpy().any()
want = src.reshape(D, DOC)[torch.from_numpy(pick.astype(np.int64)).to(dev)].reshape(-1)
assert torch.equal(out_a, want) and torch.equal(out_b, want)
r["stats"] = {"read_records": {k: int(getattr(stats_a, k)) for k, _ in stats_a._fields_}, "read_ranges@128KiB": {k: int(getattr(stats_b, k)) for k, _ in stats_b._fields_}}
r["ranges_over_records"] = round(r["median_ms"]["read_ranges@128KiB"] / r["median_ms"]["read_records"], 2)
result["read_4096_x_4KiB"] = r
whole = alternate([("records_whole", lambda: sk_rec.read()), ("fixed_whole", lambda: sk_fix.read())])
whole["GBps"] = {k: round(total / v / 1e6, 2) for k, v in whole["median_ms"].items()}
result["read_whole"] = whole
sk_rec.close(); sk_fix.close(); ctx.close(); plain.close()
print(json.dumps(result))
