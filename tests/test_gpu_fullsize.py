"""BASELINE.json configs[1] + configs[2] at FULL size inside the GPU suite (65 536-frame parity lived only in bench.py's own
asserts): 65 536 x 128 KiB Silesia-like frames per direction through the device-resident batch calls, every frame checked -- decode against
the generated input byte for byte, encode against libzstd 1.5.7's frame byte for byte (frames made by native host threads through
bench.compress_on_host, i.e. ZSTD_compressStream2(e_end) like c-ext/compressor.c:1035-1043). configs[3] the same way: 262 144 x 4 KiB
documents with the trained dictionary, at the bench's launch shape and the ones beside it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_65536_frames_both_directions_every_frame():
    import torch
    import bench
    from tests import reflib
    from tests.corpus import Corpus
    from zstandard_amd.device import DeviceBatchContext
    assert reflib.have_ref(), "no libzstd 1.5.7 to check against"
    F, item = 65536, 131072
    dev = torch.device("cuda", 0)
    raw = Corpus(device=dev, mix="silesia").frames(0, F, chunk=256)
    torch.cuda.synchronize()
    raw_np = raw.cpu().numpy()
    frames, csizes = bench.compress_on_host(raw_np, item)
    assert len(frames) == F
    job = bench.Job(1, dev)
    ctx = DeviceBatchContext()
    # decode: run_decompress asserts status == 0, sizes == 128 KiB and dst == raw for ALL frames
    bench.run_decompress(job, ctx, frames, csizes, raw, item, 1, 0)
    ctx.close()
    torch.cuda.empty_cache()
    # encode: run_compress compares every one of the 65 536 frames with libzstd's
    ctx = DeviceBatchContext()
    _, total, _ = bench.run_compress(job, ctx, raw, frames, item, 1, 0)
    assert total == int(csizes.sum())
    ctx.close()


DEC_TIMERS = (0, 2, 3, 4, 7, 9)      # zhip_kernel_name: the generic kernel, K1, K2, K3, K1b, one chunk's pipeline span


def _segs(offs, lens, dev):
    import torch
    a = np.zeros((len(lens), 2), dtype=np.int64)
    a[:, 0] = offs
    a[:, 1] = lens
    return torch.from_numpy(a).to(dev)


def test_262144_dictionary_documents_every_launch_shape(monkeypatch):
    """BASELINE.json configs[3] at FULL size through the device API, whose parity only bench.py --full's gate checked: 262 144 x 4 KiB JSON-like
    documents (their first eight pinned by tests/golden/dict_json4k.json) with the 112 640-byte trained dictionary, level 3, every frame against
    libzstd 1.5.7 with the same dictionary (bench.compress_on_host), every document back.
    * the bench's shape, a size hint of 4 KiB: the dictionary search's per-source tables are sized for 4 KiB (48 KiB), so all 262 144 sources --
      the most a launch takes -- are ONE launch; the decode is four pipeline chunks on three slot streams, the fourth on slot 0 again, with the
      dictionary's lane-per-frame pass and its K3 (bench.run_compress / run_decompress compare every frame and every byte);
    * 262 145 documents under the same hint, the last five of 4 097 ... 20 000 bytes (above the hint, so the generic kernel's): two launches;
    * no hint: the tables are the 16 KiB attach cutoff's, 192 KiB per source, and memory caps a launch at 32 GiB / 192 KiB = 174 762 sources
      (zhip_compress_batch_device; derived from the code): two launches. Those frames decoded where they lie in a context without a hint --
      four chunks on one slot stream with the side stream."""
    import hashlib
    import json
    import os
    import torch
    import bench
    from tests import reflib
    from tests.corpus import Corpus
    from zstandard_amd import _lib
    from zstandard_amd.device import DeviceBatchContext
    assert reflib.have_ref(), "no libzstd 1.5.7 to check against"
    monkeypatch.setattr(bench, "HOST_THREADS", min(bench.HOST_THREADS, 16))
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    blob = open(os.path.join(golden, "dict_json4k.bin"), "rb").read()
    meta = json.load(open(os.path.join(golden, "dict_json4k.json")))
    assert len(blob) == 112640 and hashlib.sha256(blob).hexdigest() == meta["dict_sha256"]
    F, DOC = 262144, 4096
    dev = torch.device("cuda", 0)
    raw = Corpus(frame_size=DOC, device=dev).json_docs(0, F)
    torch.cuda.synchronize()
    raw_np = raw.cpu().numpy()
    assert [hashlib.sha256(raw_np[i].tobytes()).hexdigest() for i in range(8)] == meta["probe_docs_sha256"]
    frames, csizes = bench.compress_on_host(raw_np, DOC, blob)
    assert [hashlib.sha256(frames[i]).hexdigest() for i in range(8)] == meta["probe_frames_sha256"]
    job = bench.Job(1, dev)

    # the bench's shape
    ctx = DeviceBatchContext(dict_data=blob, level=3)
    try:
        ctx.set_size_hint(DOC)
        _, total, kt = bench.run_compress(job, ctx, raw, frames, DOC, 1, 0)
        assert total == int(csizes.sum())
        assert kt[8][1] == 1, ("dictionary match launches, 4 KiB hint", kt)
        _, dk, _ = bench.run_decompress(job, ctx, frames, csizes, raw, DOC, 1, 0)
        assert {k: dk[k][1] for k in DEC_TIMERS} == {0: 1, 2: 4, 3: 4, 4: 4, 7: 4, 9: 4}, ("decode launches, 4 KiB hint", dk)
    finally:
        ctx.close()
    torch.cuda.empty_cache()

    # 262 145 documents under the hint, the last five above it
    L = _lib.lib()
    big_lens = [4097, 6000, 10007, 16385, 20000]
    bigs = [raw_np[8 * j: 8 * j + 5].reshape(-1)[:n].tobytes() for j, n in enumerate(big_lens)]
    m = F + 1 - len(bigs)
    want = frames[:m] + [reflib.RefZstd().compress(r, level=3, dict_data=blob) for r in bigs]
    lens = np.array([DOC] * m + big_lens, dtype=np.int64)
    bounds = np.array([int(L.zhip_compress_bound(DOC))] * m + [int(L.zhip_compress_bound(n)) for n in big_lens], dtype=np.int64)
    soffs, doffs = np.zeros(m + 5, dtype=np.int64), np.zeros(m + 5, dtype=np.int64)
    soffs[1:], doffs[1:] = np.cumsum(lens)[:-1], np.cumsum(bounds)[:-1]
    src = torch.cat([raw[:m].reshape(-1), torch.from_numpy(np.frombuffer(b"".join(bigs), dtype=np.uint8).copy()).to(dev)])
    dst = torch.zeros(int(bounds.sum()), dtype=torch.uint8, device=dev)
    out_sizes = torch.zeros(m + 5, dtype=torch.int64, device=dev)
    status = torch.full((m + 5,), -1, dtype=torch.int32, device=dev)
    ctx = DeviceBatchContext(dict_data=blob, level=3)
    try:
        ctx.set_size_hint(DOC)
        ctx.kernel_time(8)
        ctx.compress(src, _segs(soffs, lens, dev), dst, _segs(doffs, bounds, dev), out_sizes, status)
        torch.cuda.synchronize()
        launches = ctx.kernel_time(8)[1]
    finally:
        ctx.close()
    st, sz, got = status.cpu().numpy(), out_sizes.cpu().numpy(), dst.cpu().numpy()
    del src, dst
    assert launches == 2, ("dictionary match launches, 262 145 documents under a 4 KiB hint", launches)
    assert not st.any(), (np.nonzero(st)[0][:8], st[np.nonzero(st)[0][:8]])
    bad = [i for i in range(m + 5) if got[doffs[i]: doffs[i] + sz[i]].tobytes() != want[i]]
    assert not bad, ("frames that differ from libzstd's", len(bad), bad[:8])
    del got, want
    torch.cuda.empty_cache()

    # no hint: two launches, then the frames decoded where they lie
    ctx = DeviceBatchContext(dict_data=blob, level=3)
    outputs = {}
    try:
        _, total, kt = bench.run_compress(job, ctx, raw, frames, DOC, 1, 0, outputs=outputs)
        assert total == int(csizes.sum())
        assert kt[8][1] == 2, ("dictionary match launches, no hint", kt)
    finally:
        ctx.close()
    torch.cuda.empty_cache()
    slots, sizes = outputs["dst"], outputs["sizes"]
    bound = slots.shape[1]
    frame_segs = torch.stack([torch.arange(F, dtype=torch.int64, device=dev) * bound, sizes], dim=1).contiguous()
    back = torch.full((F * DOC,), 0xA5, dtype=torch.uint8, device=dev)
    bsz = torch.full((F,), -1, dtype=torch.int64, device=dev)
    bst = torch.full((F,), -1, dtype=torch.int32, device=dev)
    dctx = DeviceBatchContext(dict_data=blob, level=3)
    try:
        for k in DEC_TIMERS:
            dctx.kernel_time(k)
        dctx.decompress(slots.reshape(-1), frame_segs, back, _segs(np.arange(F, dtype=np.int64) * DOC, np.full(F, DOC, dtype=np.int64), dev), bsz, bst)
        torch.cuda.synchronize()
        dl = {k: dctx.kernel_time(k)[1] for k in DEC_TIMERS}
    finally:
        dctx.close()
    assert int(bst.abs().max().item()) == 0 and bool((bsz == DOC).all().item()), "a frame failed to decode"
    assert torch.equal(back.view(F, DOC), raw), "round trip differs"
    assert dl == {0: 1, 2: 4, 3: 4, 4: 4, 7: 4, 9: 4}, ("decode launches, no hint", dl)
    del raw, slots, back, outputs
    torch.cuda.empty_cache()
