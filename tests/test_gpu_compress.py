"""GPU parity tests for the compress path: frames from the HIP kernels (through the C ABI) must be bit-identical to
libzstd 1.5.7 (oracle/_ref) / the CPU oracle at the same level on the same inputs."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zstd():
    import zstandard_amd
    assert zstandard_amd._lib.lib().zhip_device_count() >= 1, "no GPU visible"
    return zstandard_amd


def _checker():
    from tests import reflib
    return reflib.checker()               # libzstd 1.5.7 itself (reference build, else the image's copy) or an error -- never the restatement


def test_reference_golden_vectors(zstd):
    # tests/test_compressor_compress.py:16-30, 216-227 of the reference (level-independent frames: empty input)
    assert zstd.ZstdCompressor(level=3).compress(b"") == bytes.fromhex("28b52ffd2000010000")
    assert zstd.ZstdCompressor(level=3, write_content_size=False).compress(b"") == bytes.fromhex("28b52ffd0000010000")
    # level 3 frame of b"foo": raw block (too small to compress), same bytes at every level
    assert zstd.ZstdCompressor(level=3, write_content_size=False).compress(b"foo") == bytes.fromhex("28b52ffd0000190000666f6f")


def test_edge_inputs_bit_exact(zstd):
    chk = _checker()
    rng = np.random.default_rng(3)
    raws = [b"", b"f", b"foo", b"foo" * 4, b"bar" * 6, b"x" * 6, b"x" * 7, b"x" * 8, b"a" * 1000, b"a" * 131072,
            bytes(range(256)) * 40, b"hello world, hello world, hello there world! " * 500, rng.bytes(1 << 17), rng.bytes(300),
            bytes(rng.integers(0, 4, 70000, dtype=np.uint8)), (rng.bytes(70000) * 2)[:131072]]
    c = zstd.ZstdCompressor(level=3)
    res = c.multi_compress_to_buffer(raws[1:])            # individual empty items are legal; an all-empty batch is not
    for i, r in enumerate(raws[1:]):
        assert res[i].tobytes() == chk.compress(r), "item %d (%d bytes)" % (i, len(r))
    for r in raws[:6]:
        assert c.compress(r) == chk.compress(r)


def test_corpus_bit_exact_and_flags(zstd, corpus):
    from tests import reflib
    chk = _checker()
    raws = [corpus.frame_bytes(i) for i in range(64)] + [corpus.frame_bytes(100 + i)[: 997 * (i + 1)] for i in range(48)]
    for kw, flags in (({}, reflib.DEFAULT_FLAGS), ({"write_checksum": True}, reflib.DEFAULT_FLAGS | reflib.F_CHECKSUM),
                      ({"write_content_size": False}, reflib.F_DICTID)):
        res = zstd.ZstdCompressor(level=3, **kw).multi_compress_to_buffer(raws)
        assert len(res) == len(raws)
        for i, r in enumerate(raws):
            assert res[i].tobytes() == chk.compress(r, level=3, flags=flags), (kw, i)


def test_buffer_with_segments_input_and_roundtrip(zstd, corpus):
    raws = [corpus.frame_bytes(200 + i)[: 5000 + 313 * i] for i in range(20)]
    blob = b"".join(raws)
    segs = b"".join(struct.pack("=QQ", sum(map(len, raws[:i])), len(raws[i])) for i in range(len(raws)))
    bws = zstd.BufferWithSegments(blob, segs)
    frames = zstd.ZstdCompressor().multi_compress_to_buffer(bws)
    back = zstd.ZstdDecompressor().multi_decompress_to_buffer(frames)
    assert [back[i].tobytes() for i in range(len(raws))] == raws
    coll = zstd.BufferWithSegmentsCollection(bws, bws)
    frames2 = zstd.ZstdCompressor().multi_compress_to_buffer(coll)
    assert len(frames2) == 2 * len(raws) and frames2[len(raws)].tobytes() == frames[0].tobytes()


def test_errors(zstd):
    c = zstd.ZstdCompressor()
    with pytest.raises(TypeError):
        c.multi_compress_to_buffer(True)
    with pytest.raises(ValueError, match="no source elements found"):
        c.multi_compress_to_buffer([])
    with pytest.raises(ValueError, match="source elements are empty"):
        c.multi_compress_to_buffer([b"", b"", b""])
    with pytest.raises(TypeError, match="item 0 not a bytes like object"):
        c.multi_compress_to_buffer([None])
    with pytest.raises(zstd.ZstdError):                      # loud: strategies above double-fast are not implemented
        zstd.ZstdCompressor(level=5).compress(b"x" * 2000)
    with pytest.raises(zstd.ZstdError):                      # level 4 is the greedy strategy for inputs up to 16 KiB
        zstd.ZstdCompressor(level=4).multi_compress_to_buffer([b"y" * 5000, b"z" * 300])


def test_dictionary_compression_bit_exact(zstd, corpus):
    """ZstdCompressor(dict_data=...) -- c-ext/compressor.c:150-171, 252-280: dictionary digested on the device, frames identical to
    libzstd's (attached-dictionary mode up to 16 KiB, table-copy mode above); golden vectors first, then a wider live comparison."""
    import hashlib
    from tests import reflib
    from tests.test_oracle_vs_golden import GOLD, _dict_vectors
    dicts, srcs = _dict_vectors()
    for key, kw in (("trained/default", {}), ("raw/default", {}),
                    ("trained/checksum_nodictid", {"write_checksum": True, "write_dict_id": False}),
                    ("raw/checksum_nodictid", {"write_checksum": True, "write_dict_id": False})):
        name = key.split("/")[0]
        c = zstd.ZstdCompressor(level=3, dict_data=zstd.ZstdCompressionDict(dicts[name]), **kw)
        res = c.multi_compress_to_buffer(srcs[1:])
        for i, rec in enumerate(GOLD["dictionary_compress"]["frames"][key][1:]):
            fr = res[i].tobytes()
            assert len(fr) == rec["size"] and hashlib.sha256(fr).hexdigest() == rec["sha256"], (key, i)
        rec0 = GOLD["dictionary_compress"]["frames"][key][0]
        assert hashlib.sha256(c.compress(srcs[0])).hexdigest() == rec0["sha256"]
    # wider: 600 ragged sources against the checker, round trip through the HIP decoder with the same dictionary
    chk = _checker()
    d = dicts["trained"]
    rng = np.random.default_rng(5)
    raws = [f[: int(rng.integers(1, 16385))] for f in corpus.frame_list(900, 600)]
    zd = zstd.ZstdCompressionDict(d)
    res = zstd.ZstdCompressor(level=3, dict_data=zd).multi_compress_to_buffer(raws)
    for i, r in enumerate(raws):
        assert res[i].tobytes() == chk.compress(r, level=3, flags=reflib.DEFAULT_FLAGS, dict_data=d), i
    back = zstd.ZstdDecompressor(dict_data=zd).multi_decompress_to_buffer(res)
    assert [back[i].tobytes() for i in range(len(raws))] == raws
    # above 16 KiB: libzstd's table-copy mode (tests/test_gpu_boundary.py covers it); a source beyond its window stays a loud failure
    if reflib.have_ref():                                                         # the C restatement stops at the attach cutoff; libzstd itself does not
        assert zstd.ZstdCompressor(level=3, dict_data=zd).compress(b"a" * 20000) == reflib.RefZstd().compress(b"a" * 20000, level=3, dict_data=d)
    with pytest.raises(zstd.ZstdError):                                           # level 3 windows stop at 2 MiB; beyond, libzstd drops the dictionary part-way
        zstd.ZstdCompressor(level=3, dict_data=zd).compress(b"a" * ((1 << 21) + 1))


def test_fast_strategy_levels_bit_exact(zstd):
    """levels 1, 2 and negative levels (ZSTD_fast, zstd.c:31906) against the golden vectors of all 46 inputs, then live on ragged sizes"""
    import hashlib
    from tests import reflib
    from tests.test_oracle_vs_golden import GOLD, _inputs
    inputs = _inputs()
    names = list(GOLD["levels"]["frames"])
    raws = [inputs[n] for n in names]
    nonempty = [i for i, r in enumerate(raws) if len(r)]
    for lvl in GOLD["levels"]["levels"]:
        res = zstd.ZstdCompressor(level=lvl).multi_compress_to_buffer([raws[i] for i in nonempty])
        for k, i in enumerate(nonempty):
            rec = GOLD["levels"]["frames"][names[i]][str(lvl)]
            fr = res[k].tobytes()
            assert len(fr) == rec["size"] and hashlib.sha256(fr).hexdigest() == rec["sha256"], (names[i], lvl)
    chk = _checker()
    from tests.corpus import Corpus
    c = Corpus()
    rng = np.random.default_rng(8)
    more = [f[: int(rng.integers(1, 131073))] for f in c.frame_list(700, 200)]
    for lvl in (1, 2, -3):
        res = zstd.ZstdCompressor(level=lvl, write_checksum=True).multi_compress_to_buffer(more)
        for i, r in enumerate(more):
            assert res[i].tobytes() == chk.compress(r, level=lvl, flags=reflib.DEFAULT_FLAGS | reflib.F_CHECKSUM), (lvl, i)
    back = zstd.ZstdDecompressor().multi_decompress_to_buffer(res)
    assert [back[i].tobytes() for i in range(len(more))] == more


def test_multiblock_frames_bit_exact(zstd):
    """inputs above 128 KiB (SURVEY config 1 and friends): golden vectors, one-shot and batch, round trip through the HIP decoder"""
    import hashlib
    from tests.test_oracle_vs_golden import GOLD, _multiblock_inputs
    data = _multiblock_inputs()
    one = zstd.ZstdCompressor(level=3).compress(data["random1M"])
    assert len(one) == 1048609 and hashlib.sha256(one).hexdigest() == GOLD["multiblock_compress"]["frames"]["random1M"]["3/default"]["sha256"]
    assert zstd.ZstdDecompressor().decompress(one) == data["random1M"]
    names = list(data)
    for lvl in GOLD["multiblock_compress"]["levels"]:
        for tag, kw in (("default", {}), ("checksum", {"write_checksum": True})):
            res = zstd.ZstdCompressor(level=lvl, **kw).multi_compress_to_buffer([data[n] for n in names] + [b"small neighbour"])
            for i, n in enumerate(names):
                want = GOLD["multiblock_compress"]["frames"][n]["%d/%s" % (lvl, tag)]
                fr = res[i].tobytes()
                assert len(fr) == want["size"] and hashlib.sha256(fr).hexdigest() == want["sha256"], (n, lvl, tag)
    back = zstd.ZstdDecompressor().multi_decompress_to_buffer(res)
    assert [back[i].tobytes() for i in range(len(names))] == [data[n] for n in names]


def test_sources_of_several_blocks_in_the_flat_search(zstd, corpus):
    """Batches of thousands of sources above 128 KiB take the flat match kernel for those too (ZeMbBlock, zhip_format.hpp: block layout by the
    split kernel, one lane per source over all its blocks, entropy coding and the check of the search's assumption in the generic kernel).
    ZHIP_MBC_MIN=0 turns it on for a small batch -- read when a thread's context is created, so the calls run in a fresh thread. Every frame
    against libzstd (ZSTD_compress_frameChunk, zstd/zstd.c:27545): compressible sources, incompressible stretches (raw blocks: the redo path),
    a block that repeats the one before, runs of one byte, tails of a few bytes, a small neighbour."""
    import os
    import threading
    from tests import reflib
    from tests.stress_emu_encode_blocks import make
    if not reflib.have_ref():
        pytest.fail("no libzstd 1.5.7 to check against: " + "needs reference libzstd")
    ref = reflib.RefZstd()
    rng = np.random.default_rng(123)
    raws = [make(rng, corpus) for _ in range(40)] + [corpus.frame_bytes(3)[:70000], b"tiny"]
    box = {}

    def run():
        try:
            for flags, kw in ((5, {}), (7, {"write_checksum": True})):
                res = zstd.ZstdCompressor(level=3, **kw).multi_compress_to_buffer(raws)
                box[flags] = [res[i].tobytes() for i in range(len(raws))]
            box["back"] = zstd.ZstdDecompressor().multi_decompress_to_buffer(box[7])
            box["back"] = [box["back"][i].tobytes() for i in range(len(raws))]
        except Exception as e:              # noqa: BLE001 -- reported by the assertion below
            box["error"] = e

    os.environ["ZHIP_MBC_MIN"] = "0"
    try:
        t = threading.Thread(target=run); t.start(); t.join()
    finally:
        del os.environ["ZHIP_MBC_MIN"]
    assert "error" not in box, box.get("error")
    for flags in (5, 7):
        for i, r in enumerate(raws):
            assert box[flags][i] == ref.compress(r, level=3, flags=flags), (flags, i, len(r))
    assert box["back"] == raws


def test_mixed_small_batch_through_the_large_batch_search(zstd, corpus):
    """A small batch forced onto the large-batch path (ZHIP_E1LDS_MAX=0 keeps the LDS-source kernel out of the way; read when a thread's context is
    created: fresh thread): sources of 63 ... 131 072 bytes side by side in the flat match kernel, the ones below 64 bytes in the lane-serial
    kernel with its 512-byte literal area (the slim arena slot of round 5). Frames must be libzstd's, byte for byte."""
    import os
    import threading
    from tests import reflib
    ref = reflib.checker()
    rng = np.random.default_rng(5)
    raws = []
    for i in range(300):
        n = int(rng.choice([63, 64, 100, 4096, 30000, 131071, 131072], p=[0.02, 0.02, 0.06, 0.2, 0.2, 0.1, 0.4]))
        kind = i % 6
        r = (corpus.frame_bytes(i)[:n] if kind < 3 else rng.bytes(n) if kind == 3 else bytes(rng.integers(0, 3, n, dtype=np.uint8)) if kind == 4
             else (rng.bytes(int(rng.integers(1, 900))) * (n + 1))[:n])
        raws.append(r)
    box = {}

    def run():
        try:
            res = zstd.ZstdCompressor(level=3).multi_compress_to_buffer(raws)
            box["out"] = [res[i].tobytes() for i in range(len(raws))]
        except Exception as e:              # noqa: BLE001 -- reported by the assertion below
            box["error"] = e

    os.environ["ZHIP_E1LDS_MAX"] = "0"
    try:
        t = threading.Thread(target=run); t.start(); t.join()
    finally:
        del os.environ["ZHIP_E1LDS_MAX"]
    assert "error" not in box, box.get("error")
    for i, r in enumerate(raws):
        assert box["out"][i] == ref.compress(r, level=3), (i, len(r))


def test_table_placement_pick_keeps_the_frames(zstd, corpus):
    """Round 5: the first launch of 49 152 sources or more (16 384 since round 6's last session) of a device context times the flat match kernel on up to three table allocations held side by
    side and keeps the fastest placement (zhip_compress_batch_device); round 6: up to six when the probes are cheap and the first three are
    alike, which is this batch's case on some boxes (kept = 5 seen in r06zzc / r06zzd); since the round's last session eight, always (the probes are short). The probes rewrite the chunk's sequences and lists before the real
    pass runs: every frame must still be libzstd's. 49 152 small sources (1-3 KiB: the launch is what counts, not the bytes), every one compared, both calls."""
    import importlib
    import torch
    from tests import reflib
    dev_mod = importlib.import_module("zstandard_amd.device")
    ref = reflib.checker()
    dev = torch.device("cuda", 0)
    F = 49152
    rng = np.random.default_rng(3)
    lens = rng.integers(1024, 3073, F).astype(np.int64)
    offs = np.zeros(F, dtype=np.int64); offs[1:] = np.cumsum(lens)[:-1]
    pool = np.frombuffer(b"".join(corpus.frame_bytes(i) for i in range(64)), dtype=np.uint8)
    starts = rng.integers(0, len(pool) - 4096, F)
    src_np = np.concatenate([pool[s:s + n] for s, n in zip(starts, lens)])
    bound = 4096
    def segs(o, n):
        a = np.zeros((F, 2), dtype=np.int64); a[:, 0] = o; a[:, 1] = n
        return torch.from_numpy(a).to(dev)
    src = torch.from_numpy(src_np).to(dev)
    dst = torch.zeros(F * bound, dtype=torch.uint8, device=dev)
    out_sizes = torch.zeros(F, dtype=torch.int64, device=dev); status = torch.zeros(F, dtype=torch.int32, device=dev)
    ctx = dev_mod.DeviceBatchContext()
    try:
        for _ in range(2):                                         # the second call runs without probes on the tables the first one kept
            ctx.compress(src, segs(offs, lens), dst, segs(np.arange(F, dtype=np.int64) * bound, np.full(F, bound, dtype=np.int64)), out_sizes, status)
            torch.cuda.synchronize()
            assert int(status.abs().max().item()) == 0
            ms, kept = ctx.table_pick()
            assert ms[0] > 0 and ms[1] > 0 and 0 <= kept <= 7, (ms, kept)
            got = dst.view(F, bound).cpu().numpy(); sz = out_sizes.cpu().numpy()
            for i in range(F):                                      # ALL of them (the probes rewrite every list up to three times; it costs seconds)
                assert got[i, : sz[i]].tobytes() == ref.compress(src_np[offs[i]: offs[i] + lens[i]].tobytes(), level=3), i
    finally:
        ctx.close()


def test_launch_numbers_in_the_tables_across_calls(zstd, corpus):
    """Round 6: the flat searches' tables are not zeroed per launch -- a cell carries its launch's number and the context zeroes the allocation when it must (new allocation, numbers used
    up, a batch that reaches slots never zeroed, tables last used WITHOUT numbers: the several-block search). One thread's context through a sequence that meets each of those, every frame
    of every call against libzstd: a batch, a slightly larger one (inside the allocation's headroom), the same sources shuffled (other sources' cells in every slot), sources of several
    blocks through the flat search (ZHIP_MBC_MIN=0; un-numbered cells), one-block sources again, another level's strategy in between, a dictionary batch twice (its own numbering), and
    plain sources once more."""
    import os
    import threading
    from tests import reflib
    from tests.stress_emu_encode_blocks import make
    ref = reflib.checker()
    rng = np.random.default_rng(77)
    small = [corpus.frame_bytes(500 + i)[: int(rng.integers(64, 131073))] for i in range(420)]
    blocks = [make(rng, corpus) for _ in range(24)]
    docs = [corpus.frame_bytes(900 + i)[i * 37: i * 37 + 4096] for i in range(300)]
    dd = ref.train_dictionary(16384, [corpus.frame_bytes(950 + i)[:4096] for i in range(200)]) if hasattr(ref, "train_dictionary") else corpus.frame_bytes(960)[:16384]
    steps = [("a", small[:380], 3, None), ("b", small, 3, None), ("c", [small[i] for i in rng.permutation(len(small))], 3, None), ("d", blocks + small[:40], 3, None),
             ("e", small[:400], 3, None), ("f", small[:100], 1, None), ("g", [small[i] for i in rng.permutation(400)], 3, None),
             ("h", docs, 3, dd), ("i", [docs[i] for i in rng.permutation(len(docs))], 3, dd), ("j", small[:410], 3, None)]
    box = {}

    def run():
        try:
            for name, raws, level, dict_bytes in steps:
                kw = {"dict_data": zstd.ZstdCompressionDict(dict_bytes)} if dict_bytes else {}
                res = zstd.ZstdCompressor(level=level, **kw).multi_compress_to_buffer(raws)
                box[name] = [res[i].tobytes() for i in range(len(raws))]
        except Exception as e:              # noqa: BLE001 -- reported by the assertion below
            box["error"] = e

    os.environ["ZHIP_MBC_MIN"] = "0"; os.environ["ZHIP_E1LDS_MAX"] = "0"
    try:
        t = threading.Thread(target=run); t.start(); t.join()
    finally:
        del os.environ["ZHIP_MBC_MIN"]; del os.environ["ZHIP_E1LDS_MAX"]
    assert "error" not in box, box.get("error")
    for name, raws, level, dict_bytes in steps:
        for i, r in enumerate(raws):
            want = ref.compress(r, level=level, dict_data=dict_bytes) if dict_bytes else ref.compress(r, level=level)
            assert box[name][i] == want, (name, i, len(r))


def test_fast_strategy_batches_above_32768_sources(zstd, corpus):
    """Round 6: fast-strategy batches (levels 1, 2, negative) above 32 768 sources run 65 536 per chunk at sixteen sources per wave of the lane-serial match kernel -- every source in
    flight at once -- instead of chunks of 32 768 at eight. 34 000 small sources (64 bytes ... 6 KiB, a few of a whole block) at levels 1 and -3: every frame libzstd's, all of them compared."""
    from tests import reflib
    ref = reflib.checker()
    rng = np.random.default_rng(83)
    pool = [corpus.frame_bytes(1200 + i) for i in range(40)]
    raws = []
    for i in range(34000):
        b = pool[i % 40]; o = int(rng.integers(0, 120000)); n = int(rng.integers(64, 6145)) if i % 500 else 131072
        raws.append(b[o:o + n] if n < 131072 else b)
    for level in (1, -3):
        res = zstd.ZstdCompressor(level=level).multi_compress_to_buffer(raws)
        assert len(res) == len(raws)
        for i in range(len(raws)):                                   # every frame (it was every 7th)
            assert res[i].tobytes() == ref.compress(raws[i], level=level), (level, i, len(raws[i]))
        del res
