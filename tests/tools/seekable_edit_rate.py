"""Editing a seekable stream (zhip_seekable_edit_device) beside what it replaces, in one process, level 3.

  move     reorder by a random permutation of a stream of 1 GiB of content in 128 KiB frames (8 192 frames)  against  a device-to-device copy_ of the same
           byte count: what the bisect per tile and the unaligned 16-byte accesses cost over a plain copy
  append   A documents of 4 KiB (default 4 096) appended IN PLACE to the stream of D JSON-like documents (default 262 144, one frame each, with their trained
           dictionary)  against  seekable_compress_records of the A documents alone (the scan over picks and the table are the difference)  and against
           recompressing all D + A; the same on a stream of D / 8 documents (an append in place must not grow with the old stream beyond its table)
  update   1 % of the D documents replaced, out of place  against  recompressing all D

Times are host wall clock around the call + a device synchronize, three alternating repetitions after a warm-up (contexts warm, scratch grown); every result
is checked: the moved frames against the old stream's, the appended and replaced streams by reading records back.
Usage: python tests/tools/seekable_edit_rate.py [documents [appended]]"""
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

D = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
A = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
DOC = 4096
dev = torch.device("cuda", 0)
blob = open(os.path.join(ROOT, "tests", "golden", "dict_json4k.bin"), "rb").read()
stream0 = torch.cuda.current_stream().cuda_stream
rng = np.random.default_rng(12)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def alternate(pairs, before=None):
    """[(name, fn)] -> ms lists of three alternating repetitions after one warm-up each, and the medians; before(name) runs untimed in front of every call"""
    for name, fn in pairs:
        if before:
            before(name)
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in pairs}
    for _ in range(3):
        for name, fn in pairs:
            if before:
                before(name)
            ms[name].append(round(timed(fn) * 1e3, 3))
    return {"ms": ms, "median_ms": {k: sorted(v)[1] for k, v in ms.items()}, "spread_ms": {k: round(max(v) - min(v), 3) for k, v in ms.items()}}


def picks_of(frames, n_records=0):
    p = np.zeros((len(frames) + n_records, 2), dtype=np.uint32)
    p[:len(frames), 1] = frames
    p[len(frames):, 0] = 1
    p[len(frames):, 1] = np.arange(n_records)
    return np.ascontiguousarray(p)


def table_of(n):
    return torch.stack([torch.arange(n, dtype=torch.int64, device=dev) * DOC, torch.full((n,), DOC, dtype=torch.int64, device=dev)], dim=1).contiguous()


result = {"documents": D, "appended": A}
size = torch.zeros(1, dtype=torch.int64, device=dev)
status = torch.zeros(2, dtype=torch.int32, device=dev)

# ---------------------------------------------------------------------------------------------- move
plain = DeviceBatchContext(level=3)
L = plain.L
docs = Corpus(frame_size=DOC, device=dev).json_docs(0, D + A).reshape(-1)
content = docs[:262144 * DOC] if D >= 262144 else docs[:D * DOC]
fixed = plain.seekable_compress(content, frame_size=131072)
sk = SeekableStream(plain, fixed)
order = rng.permutation(sk.n_frames)
pk = picks_of(order)
moved = torch.zeros(fixed.numel(), dtype=torch.uint8, device=dev)
copied = torch.zeros(fixed.numel(), dtype=torch.uint8, device=dev)


def move():
    assert L.zhip_seekable_edit_device(plain.ctx, sk.handle, pk.ctypes.data, len(pk), None, 0, None, 0, 0, 0, 0, moved.data_ptr(), moved.numel(), size.data_ptr(), status.data_ptr(), stream0) == 0


m = alternate([("reorder", move), ("copy_", lambda: copied.copy_(fixed))])
assert status.cpu().tolist() == [0, 0] and int(size[0]) == fixed.numel()
with SeekableStream(plain, moved) as back:
    f = int(order[17])
    assert torch.equal(back.read_records([17])[0], sk.read_records([f])[0])
    assert torch.equal(back.read(0, 131072), sk.read(int(order[0]) * 131072, 131072))
m["bytes"] = int(fixed.numel()); m["frames"] = int(sk.n_frames)
m["GBps"] = {k: round(fixed.numel() / v / 1e6, 1) for k, v in m["median_ms"].items()}
m["reorder_over_copy"] = round(m["median_ms"]["reorder"] / m["median_ms"]["copy_"], 3)
result["move"] = m
sk.close()
del moved, copied, fixed

# ---------------------------------------------------------------------------------------------- append, update
ctx = DeviceBatchContext(dict_data=blob, level=3)
ctx._ensure_cparams()
new_src = docs[D * DOC:(D + A) * DOC]
new_table = table_of(A)
all_table = table_of(D + A)


def append_case(n_old):
    old = ctx.seekable_compress_records(docs[:n_old * DOC], table_of(n_old), max_content_bytes=n_old * DOC, max_record_bytes=DOC)
    old_size = int(old.numel())
    pk = picks_of(np.arange(n_old), A)
    with SeekableStream(ctx, old) as opened:
        cap = int(L.zhip_seekable_edit_bound(opened.handle, pk.ctypes.data, len(pk), DOC, 0))
    room = torch.zeros(cap, dtype=torch.uint8, device=dev)
    room[:old_size] = old
    table_bytes = 8 + 8 * n_old + 9
    saved = old[old_size - table_bytes:].clone()
    small = torch.zeros(int(L.zhip_seekable_records_bound(A * DOC, A, 0)), dtype=torch.uint8, device=dev)
    state = {}

    def before(name):
        if name == "append_in_place":              # the last append overwrote the old table: put it back and open the stream again (untimed)
            if "sk" in state:
                state["sk"].close()
            room[old_size - table_bytes:old_size] = saved
            state["sk"] = SeekableStream(ctx, room[:old_size])

    def append():
        assert L.zhip_seekable_edit_device(ctx.ctx, state["sk"].handle, pk.ctypes.data, len(pk), new_src.data_ptr(), new_src.numel(), new_table.data_ptr(), A, A * DOC, DOC, 0,
                                           room.data_ptr(), cap, size.data_ptr(), status.data_ptr(), stream0) == 0

    def alone():
        assert L.zhip_seekable_compress_records_device(ctx.ctx, new_src.data_ptr(), new_src.numel(), new_table.data_ptr(), A, A * DOC, DOC, 0, small.data_ptr(), small.numel(),
                                                       size.data_ptr(), status.data_ptr(), stream0) == 0

    r = alternate([("append_in_place", append), ("records_call_of_the_new_alone", alone)], before)
    before("append_in_place"); append(); torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0]
    new_size = int(size[0])
    state["sk"].close()
    with SeekableStream(ctx, room[:new_size]) as st:
        assert st.n_frames == n_old + A
        views = st.read_records([0, n_old - 1, n_old, n_old + A - 1])
        want = [docs[:DOC], docs[(n_old - 1) * DOC:n_old * DOC], new_src[:DOC], new_src[(A - 1) * DOC:]]
        assert all(torch.equal(v, w) for v, w in zip(views, want))
    r["old_stream_bytes"] = old_size; r["new_stream_bytes"] = new_size
    return r, old


a, old = append_case(D)
big = torch.zeros(int(L.zhip_seekable_records_bound((D + A) * DOC, D + A, 0)), dtype=torch.uint8, device=dev)


def recompress(n, table):
    assert L.zhip_seekable_compress_records_device(ctx.ctx, docs.data_ptr(), n * DOC, table.data_ptr(), n, n * DOC, DOC, 0, big.data_ptr(), big.numel(), size.data_ptr(), status.data_ptr(),
                                                   stream0) == 0


a["recompress_all"] = alternate([("recompress_all_%d" % (D + A), lambda: recompress(D + A, all_table))])
result["append"] = a
result["append_to_an_eighth"] = append_case(D // 8)[0]

# update: 1 % replaced, out of place
U = max(1, D // 100)
idx = np.sort(rng.choice(D, size=U, replace=False))
pk = picks_of(np.arange(D))
pk[idx, 0] = 1
pk[idx, 1] = np.arange(U)
upd_src = new_src[:U * DOC] if U <= A else docs[:U * DOC]
upd_table = table_of(U)
sk = SeekableStream(ctx, old)
out = torch.zeros(int(L.zhip_seekable_edit_bound(sk.handle, pk.ctypes.data, len(pk), DOC, 0)), dtype=torch.uint8, device=dev)
old_table = table_of(D)


def update():
    assert L.zhip_seekable_edit_device(ctx.ctx, sk.handle, pk.ctypes.data, len(pk), upd_src.data_ptr(), upd_src.numel(), upd_table.data_ptr(), U, U * DOC, DOC, 0,
                                       out.data_ptr(), out.numel(), size.data_ptr(), status.data_ptr(), stream0) == 0


u = alternate([("replace_%d" % U, update), ("recompress_all_%d" % D, lambda: recompress(D, old_table))])
update(); torch.cuda.synchronize()
assert status.cpu().tolist() == [0, 0]
with SeekableStream(ctx, out[:int(size[0])]) as st:
    replaced = set(idx.tolist())
    kept = next(i for i in range(D) if i not in replaced)
    views = st.read_records([int(idx[U // 2]), kept])
    assert st.n_frames == D and torch.equal(views[0], upd_src[(U // 2) * DOC:(U // 2 + 1) * DOC]) and torch.equal(views[1], docs[kept * DOC:(kept + 1) * DOC])
u["speedup"] = round(u["median_ms"]["recompress_all_%d" % D] / u["median_ms"]["replace_%d" % U], 1)
result["update_1_percent"] = u
sk.close(); ctx.close(); plain.close()
print(json.dumps(result))
