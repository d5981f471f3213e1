"""The plan of the host-buffer batch calls (python-zstandard_amd/csrc/zhip_host_calls.hpp) on the CPU: everything zhip_compress_batch / zhip_decompress_batch decide between
their HIP calls -- frame inspection, the two segment layouts and their refusals, chunk cuts, upload steps, packing runs, the meta layouts, the verdicts over what comes back,
and the fan-out's device list, slot count and merge.

Four kinds of check. (1) Equality with tests/golden/host_calls.json, recorded from the commit BEFORE the header existed (that commit's lines of zhip_lib.hip pasted verbatim
behind the entries of tests/emu/emu_host_calls.cpp, the packing threads behind a note of their run), never from the header: ZHIP_PLAN_SO names such a library,
python -m tests.test_emu_host_calls --record writes the fixture from it. (2) Properties that hold whatever the fixture says: layouts without overlap inside their reservation,
cuts / steps / runs that cover [0, n) in order, once. (3) Every refusal and every verdict case, stated directly. (4) Frame inspection against libzstd itself.
A stand-alone AddressSanitizer + UBSan program (tests/emu/host_calls_main.cpp) runs the chain layout -> cuts -> steps -> packing -> verdicts in exactly sized allocations.

And the resources behind those calls, with stubs in place of HIP (tests/emu/host_pool_stubs.hpp): which device buffers a context gives back after a call (host_trim_order), and
zhip_host_pool.hpp's payload pool, device slots and fan-out -- each against a few lines of Python that restate its rule, the pool and the fan-out again in the program above and,
from several threads at once, in a ThreadSanitizer program (tests/emu/host_pool_tsan_main.cpp)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import craft, emulib

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "host_calls.json")
U64 = C.POINTER(C.c_uint64)

ERR_ZSTD, ERR_NO_MEMORY, ERR_SIZE_MISMATCH, ERR_UNKNOWN_SIZE, ERR_HIP, ERR_UNSUPPORTED = 1, 2, 3, 4, 5, 6          # include/zstd_hip.h
ZE_PREFIX_UNKNOWN, ZE_FRAMEPARAM_UNSUPPORTED, ZE_CORRUPTION, ZE_SRC_SIZE_WRONG = 10, 14, 20, 72                        # zhip_format.hpp == ZSTD_ErrorCode
CONTENTSIZE_UNKNOWN, CONTENTSIZE_ERROR = 2 ** 64 - 1, 2 ** 64 - 2
WALK_LAST, WALK_TRUNCATED, WALK_RESERVED = 0, 1, 2
CAP = 1 << 46
STAGE = 512 << 20
TEXT_2GIB = "inputs of 2 GiB and more are not implemented in the HIP backend"


def arr(v):
    return np.ascontiguousarray(v, dtype=np.uint64)


def ptr(a):
    return a.ctypes.data_as(U64)


class HcLib:
    def __init__(self, path=None):
        path = path or os.environ.get("ZHIP_PLAN_SO") or emulib.EMU_SO
        if not os.path.exists(path):
            emulib.build()
        self.lib = L = C.CDLL(path)
        for name in ("emu_hc_chunks", "emu_hc_upload_steps", "emu_hc_pack_split", "emu_hc_slots_for", "emu_hc_partition", "emu_hc_content_size", "emu_hc_compress_bound"):
            if hasattr(L, name):
                getattr(L, name).restype = C.c_uint64
        L.emu_hc_frame_size.restype = C.c_int64
        L.emu_hc_count_blocks.restype = C.c_uint32

    def chunks(self, in_len, out_len, max_bytes, max_items, first=0):
        a, b = arr(in_len), arr(out_len)
        out = np.zeros(len(a) + 2, dtype=np.uint64)
        k = self.lib.emu_hc_chunks(ptr(a), ptr(b), C.c_uint64(len(a)), C.c_uint64(max_bytes), C.c_uint64(max_items), C.c_uint64(first), ptr(out), C.c_uint64(len(out)))
        return out[:k].tolist()

    def steps(self, lens, lo, hi, stage):
        a = arr(lens)
        out = np.zeros(3 * (len(a) + 1), dtype=np.uint64)
        k = self.lib.emu_hc_upload_steps(ptr(a), C.c_uint64(len(a)), C.c_uint64(lo), C.c_uint64(hi), C.c_uint64(stage), ptr(out), C.c_uint64(len(a) + 1))
        return [tuple(out[3 * i:3 * i + 3].tolist()) for i in range(k)]

    def split(self, lens, lo, hi, threshold, threads):
        a = arr(lens)
        out = np.zeros(2 * (len(a) + 1), dtype=np.uint64)
        k = self.lib.emu_hc_pack_split(ptr(a), C.c_uint64(len(a)), C.c_uint64(lo), C.c_uint64(hi), C.c_uint64(threshold), C.c_uint32(threads), ptr(out), C.c_uint64(len(a) + 1))
        return [tuple(out[2 * i:2 * i + 2].tolist()) for i in range(k)]

    def layout_bytes(self, direction, n, n_chunks):
        out = (C.c_uint64 * 2)()
        self.lib.emu_hc_layout_bytes(C.c_int(direction), C.c_uint64(n), C.c_uint64(n_chunks), out)
        return list(out)

    def layout(self, direction, n, n_chunks):
        out = (C.c_uint64 * 9)()
        k = self.lib.emu_hc_layout(C.c_int(direction), C.c_uint64(n), C.c_uint64(n_chunks), out)
        names = ["dSizes", "dOffs", "dTotals", "dStatus", "dBytes", "hSizes", "hTotals", "hStatus", "hBytes"] if direction else ["dSizes", "dStatus", "dBytes", "hSizes", "hStatus", "hBytes"]
        assert k == len(names)
        return dict(zip(names, list(out)[:k]))

    def slots_for(self, slots, explicit, min_bytes, n, nbytes):
        return int(self.lib.emu_hc_slots_for(C.c_uint64(slots), C.c_int(explicit), C.c_uint64(min_bytes), C.c_uint64(n), C.c_uint64(nbytes)))

    def parse_devices(self, text, count):
        out = (C.c_int * 64)()
        k = self.lib.emu_hc_parse_devices(text.encode(), C.c_int(count), out, C.c_int(64))
        return list(out)[:k]

    def merge(self, rc, lo, err_index):
        out = (C.c_uint64 * 3)()
        self.lib.emu_hc_merge((C.c_int * len(rc))(*rc), ptr(arr(lo)), ptr(arr(err_index)), C.c_uint64(len(rc)), out)
        return list(out)

    def partition(self, sizes, workers):
        a = arr(sizes)
        out = np.zeros(2 * max(1, workers), dtype=np.uint64)
        used = self.lib.emu_hc_partition(ptr(a), C.c_uint64(len(a)), C.c_uint64(workers), ptr(out))
        return [tuple(out[2 * w:2 * w + 2].tolist()) for w in range(used)]

    # frame inspection
    def content_size(self, frame, fmt=0):
        return int(self.lib.emu_hc_content_size(bytes(frame), C.c_uint64(len(frame)), C.c_int(fmt)))

    def frame_size(self, frame, fmt=0):
        return int(self.lib.emu_hc_frame_size(bytes(frame), C.c_uint64(len(frame)), C.c_int(fmt)))

    def count_blocks(self, frame, fmt=0):
        return int(self.lib.emu_hc_count_blocks(bytes(frame), C.c_uint64(len(frame)), C.c_int(fmt)))

    def walk(self, data, pos):
        out = (C.c_uint64 * 3)()
        self.lib.emu_hc_walk(bytes(data), C.c_uint64(len(data)), C.c_uint64(pos), out)
        return tuple(out)

    # pass 1
    def decompress_segments(self, items, fmt=0):
        """items: (source bytes, dstSize). Returns (kind, index, srcTotal, dstTotal, segs, nBlocks)"""
        n = len(items)
        blob = b"".join(f for f, _ in items) + b"\0"
        src = [len(f) for f, _ in items]
        off = arr([sum(src[:i]) for i in range(n + 1)])
        segs = np.zeros(4 * n + 2, dtype=np.uint64); nb = np.zeros(n + 1, dtype=np.uint32); out = (C.c_uint64 * 4)()
        self.lib.emu_hc_decompress_segments(blob, ptr(off), ptr(arr(src)), ptr(arr([d for _, d in items])), C.c_uint64(n), C.c_int(fmt), ptr(segs),
                                            nb.ctypes.data_as(C.c_void_p), out)
        return out[0], out[1], out[2], out[3], segs[:4 * n].reshape(2 * n, 2).tolist(), nb[:n].tolist()

    def compress_segments(self, sizes):
        n = len(sizes)
        segs = np.zeros(4 * n + 2, dtype=np.uint64); out = (C.c_uint64 * 4)(); text = C.create_string_buffer(256)
        self.lib.emu_hc_compress_segments(ptr(arr(sizes)), C.c_uint64(n), ptr(segs), out, text, C.c_uint64(256))
        return out[0], out[1], out[2], out[3], segs[:4 * n].reshape(2 * n, 2).tolist(), text.value.decode()

    def compress_bound(self, n):
        return int(self.lib.emu_hc_compress_bound(C.c_uint64(n)))

    # verdicts
    def decompress_verdict(self, dst_len, sizes, status, lo, hi, allow_short):
        n = len(dst_len)
        segs = np.zeros(2 * (hi - lo) + 2, dtype=np.uint64); out = (C.c_uint64 * 5)()
        st = np.ascontiguousarray(status, dtype=np.int32)
        self.lib.emu_hc_decompress_verdict(ptr(arr(dst_len)), ptr(arr(sizes)), st.ctypes.data_as(C.c_void_p), C.c_uint64(n), C.c_uint64(lo), C.c_uint64(hi), C.c_int(allow_short), ptr(segs), out)
        return tuple(out), segs[:2 * (hi - lo)].reshape(hi - lo, 2).tolist()

    def compress_verdict(self, sizes, status, lo, hi):
        segs = np.zeros(2 * (hi - lo) + 2, dtype=np.uint64); out = (C.c_uint64 * 6)()
        st = np.ascontiguousarray(status, dtype=np.int32)
        self.lib.emu_hc_compress_verdict(ptr(arr(sizes)), st.ctypes.data_as(C.c_void_p), C.c_uint64(lo), C.c_uint64(hi), ptr(segs), out)
        return tuple(out), segs[:2 * (hi - lo)].reshape(hi - lo, 2).tolist()


    # what a context gives back, the payload pool, the device slots, the fan-out (zhip_host_pool.hpp over the stubs of tests/emu/host_pool_stubs.hpp)
    def trim_order(self, caps, trimmable, keep):
        out = np.zeros(len(caps) + 1, dtype=np.uint64)
        self.lib.emu_hc_trim_order.restype = C.c_uint64
        k = self.lib.emu_hc_trim_order(ptr(arr(caps)), bytes(bytearray(int(t) for t in trimmable)), C.c_uint64(len(caps)), C.c_uint64(keep), ptr(out))
        return out[:k].tolist()

    def pool_script(self, keep, ops):
        """ops: ("take", bytes) | ("give", the op number that took it) | ("foreign", bytes) | ("refuse", 0 or 1). Returns (per op [pointer id, allocated now, capacity asked, idle after],
        dict(allocs, unpins, unknown, live), the capacities unpinned in order)"""
        kinds = dict(take=0, give=1, foreign=2, refuse=3)
        flat = arr([v for kind, a in ops for v in (kinds[kind], a)] + [0])
        res = np.zeros(4 * len(ops) + 1, dtype=np.uint64); tail = (C.c_uint64 * 4)(); freed = np.zeros(len(ops) + 1, dtype=np.uint64)
        self.lib.emu_hc_pool_script(C.c_uint64(keep), ptr(flat), C.c_uint64(len(ops)), ptr(res), tail, ptr(freed), C.c_uint64(len(ops)))
        return res[:4 * len(ops)].reshape(len(ops), 4).tolist(), dict(zip(("allocs", "unpins", "unknown", "live"), tail)), freed[:tail[1]].tolist()

    def pool_parse(self, count, devices, min_bytes):
        out = (C.c_uint64 * 66)()
        k = self.lib.emu_hc_pool_parse(C.c_int(count), None if devices is None else devices.encode(), None if min_bytes is None else min_bytes.encode(), out, C.c_int(64))
        return bool(out[0]), int(out[1]), list(out)[2:2 + k]

    def fan_out(self, sizes, modes, d):
        n = len(sizes)
        out = (C.c_uint64 * 12)(); order = np.zeros(n + 1, dtype=np.uint64); text = C.create_string_buffer(256)
        self.lib.emu_hc_fan_out(ptr(arr(list(sizes) + [0])), bytes(bytearray(modes)) + b"\0", C.c_uint64(n), C.c_uint64(d), out, ptr(order), text, C.c_uint64(256))
        names = ("rc", "kind", "index", "zerr", "outputs", "runs", "empty_runs", "afters", "freed", "live", "bound", "bound_own_device")
        r = dict(zip(names, (int(v) for v in out)))
        r["order"] = order[:r["outputs"]].tolist(); r["text"] = text.value.decode()
        return r


@pytest.fixture(scope="module")
def lib():
    return HcLib()


# ------------------------------------------------------------------------------------------ the cases pinned to the parent commit
COUNTS = [0, 1, 2, 2047, 2048, 2049, 8192, 8193, 32768, 32769, 65537]


def mixed(n, seed, modulus):
    """n lengths in [0, modulus): a fixed sequence, zeros included"""
    i = np.arange(n, dtype=np.uint64)
    return ((i * np.uint64(2654435761) + np.uint64(seed) * np.uint64(40503)) >> np.uint64(7)) % np.uint64(modulus)


def chunk_cases():
    """(name, input lengths, output lengths, maxBytes, maxItems, firstItems)"""
    out = []
    for n in COUNTS:
        for first in (0, 1, 2048):
            out.append(("uniform decompress n=%d first=%d" % (n, first), np.full(n, 40000, np.uint64), np.full(n, 131072, np.uint64), 1 << 30, 32768, first))
            out.append(("uniform compress n=%d first=%d" % (n, first), np.full(n, 131072, np.uint64), np.full(n, 131600, np.uint64), 4 << 30, 32768, first))
            out.append(("mixed n=%d first=%d" % (n, first), mixed(n, 1, 3 << 20), mixed(n, 2, 9 << 20), 1 << 30, 32768, first))
        out.append(("mixed, small chunks n=%d" % n, mixed(n, 3, 700), mixed(n, 4, 5000), 1 << 20, 1000, 0))
        out.append(("empty items n=%d" % n, np.zeros(n, np.uint64), np.zeros(n, np.uint64), 1 << 30, 32768, 0))
    small = [("a single item above maxBytes", [10, 5000, 10, 10], [1, 1, 1, 1], 1000), ("an item above maxBytes by output", [1, 1, 1, 1], [10, 10, 5000, 10], 1000),
             ("an exact hit of maxBytes by input bytes", [400, 600, 400, 599, 1, 1], [1] * 6, 1000), ("one below the hit by input bytes", [400, 599, 400, 599, 1, 1], [1] * 6, 1000),
             ("an exact hit of maxBytes by output bytes", [1] * 6, [400, 600, 400, 599, 1, 1], 1000), ("one below the hit by output bytes", [1] * 6, [400, 599, 400, 599, 1, 1], 1000),
             ("hits on both sides at different items", [500, 500, 1, 1, 1], [1, 1, 999, 1, 1], 1000)]
    for name, a, b, mb in small:
        for first in (0, 1, 2048):
            for items in (32768, 2):
                out.append(("%s, first=%d items=%d" % (name, first, items), arr(a), arr(b), mb, items, first))
    return out


TABLES = [[5], [0], [100, 100], [0, 0, 0, 0], [100] * 16, [1, 99, 100, 101, 0, 250, 3, 3, 3, 90, 10], [1000, 1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1, 1000],
          [30, 0, 30, 0, 30, 0, 30, 0, 30, 0, 30, 0, 30, 0, 30, 0], [7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67]]


def step_cases():
    return [(t, lo, hi, stage) for t in TABLES for stage in (1, 100, 101, 250, 10 ** 9) for lo, hi in ((0, len(t)), (1, len(t)), (0, len(t) - 1), (len(t) // 2, len(t)))if lo < hi]


def split_cases():
    return [(t, lo, hi, thr, nt) for t in TABLES for thr in (0, 1, 100, 400, 10 ** 9) for nt in (1, 2, 3, 8) for lo, hi in ((0, len(t)), (1, len(t)), (2, len(t) - 1)) if lo < hi]


LAYOUT_NS, LAYOUT_CHUNKS = [0, 1, 2, 3, 63, 64, 65, 32769], [0, 1, 2, 3]
SLOT_CASES = [(slots, ex, mb, n, b) for slots in (0, 1, 2, 3, 8) for ex in (0, 1) for mb in (0, 1, 256 << 20) for n in (0, 1, 2, 5, 100)
              for b in (0, 1, (256 << 20) - 1, 256 << 20, (512 << 20) - 1, 512 << 20, 3 << 30, 1 << 40)]
DEVICE_LISTS = [("0,0", 1), ("0,0,0", 1), ("7", 1), ("", 1), ("0,x", 1), ("0,1,2", 8), ("2,1,0", 8), ("0,1,2", 2), ("0,,1", 8), ("-1,0", 8), (" 1, 2", 8), ("1;2", 8), ("x", 8), ("0,1,", 8),
                ("0", 0), ("3,3,9,3", 4), ("1x,2", 8)]
MERGE_CASES = [([0, 0, 0], [0, 10, 20], [0, 0, 0]), ([0, 3, 0], [0, 10, 20], [0, 4, 0]), ([0, 3, 1], [0, 10, 20], [0, 4, 7]), ([1, 3, 1], [0, 10, 20], [2, 4, 7]), ([0, 0, 5], [0, 10, 20], [0, 0, 0]),
               ([2], [0], [9]), ([0], [0], [0]), ([0, 1, 4, 0], [0, 1, 2, 3], [0, 0, 0, 0])]


def inspection_frames():
    """(name, frame): every frame of tests/golden/edge_frames.json, re-made by tests/craft.py under its pinned names (the fixture leaves one above 128 KiB out of its hex), the frames
    of tests/golden/frames.bin in the order they lie there (it holds 33; the first 64 are all of them), the short frames golden.json spells out in hex, and skippable frames"""
    made = {name: frame for gen in (craft.edge_frames, craft.skippable_frames, craft.encoding_variants) for name, frame, _, _ in gen()}
    pins = json.load(open(os.path.join(HERE, "golden", "edge_frames.json")))["frames"]
    out = []
    for r in pins:
        assert r["name"] in made and hashlib.sha256(made[r["name"]]).hexdigest() == r["frame_sha256"], r["name"]
        out.append(("edge: " + r["name"], bytes(made[r["name"]])))
    gold = json.load(open(os.path.join(HERE, "golden", "golden.json")))
    blob = open(os.path.join(HERE, "golden", "frames.bin"), "rb").read()
    recs, hexes = [], []

    def walk(o):
        if isinstance(o, dict):
            if "blob_offset" in o:
                recs.append((o["blob_offset"], o.get("frame_size", o.get("size"))))
            if isinstance(o.get("hex"), str) and len(o["hex"]) <= 128:
                hexes.append(bytes.fromhex(o["hex"]))
            for v in o.values():
                walk(v)
        elif isinstance(o, list):
            for v in o:
                walk(v)
    walk(gold)
    recs.sort()
    assert len(recs) >= 33
    out += [("frames.bin @%d" % o, blob[o:o + s]) for o, s in recs[:64]]
    out += [("golden.json hex %d" % i, f) for i, f in enumerate(hexes)]
    for magic in (0x184D2A50, 0x184D2A5F):
        for payload in (b"", b"x"):
            out.append(("skippable %x, %d bytes" % (magic, len(payload)), magic.to_bytes(4, "little") + len(payload).to_bytes(4, "little") + payload))
    return out


def inspection_views(frames):
    """(name, bytes, format): each frame whole, every proper prefix of the frames of at most 64 bytes, and each frame without its magic under the magicless format"""
    for name, f in frames:
        yield name, f, 0
        if len(f) <= 64:
            for k in range(len(f)):
                yield "%s [:%d]" % (name, k), f[:k], 0
        yield name + " magicless", f[4:], 1
        if len(f) <= 64:
            for k in range(max(len(f) - 4, 0)):
                yield "%s magicless [:%d]" % (name, k), f[4:4 + k], 1


def inspection_digest(lib):
    """content size, compressed size and block count of every view. One thing is NOT the parent's and is left out: the error CODE of the compressed size of inputs below
    5 bytes with a magic. The parent said srcSize_wrong for all of them; libzstd says prefix_unknown where the bytes already begin neither magic, and so does the header
    (test_inspection_is_libzstds holds it to that). That the answer is an error is pinned here too."""
    h = hashlib.sha256()
    for name, data, fmt in inspection_views(inspection_frames()):
        size = lib.frame_size(data, fmt)
        h.update(("%s|%d|%d|%d|%d\n" % (name, fmt, lib.content_size(data, fmt), -1 if fmt == 0 and len(data) < 5 and size < 0 else size, lib.count_blocks(data, fmt))).encode())
    return h.hexdigest()


def cut_row(cuts):
    return cuts if len(cuts) <= 40 else {"count": len(cuts), "sha256": hashlib.sha256(",".join(map(str, cuts)).encode()).hexdigest(), "head": cuts[:6], "tail": cuts[-3:]}


def pinned_rows(lib):
    return {
        "chunks": [cut_row(lib.chunks(a, b, mb, items, first)) for _, a, b, mb, items, first in chunk_cases()],
        "steps": [[list(s) for s in lib.steps(*c)] for c in step_cases()],
        "splits": [[list(s) for s in lib.split(*c)] for c in split_cases()],
        "layout_bytes": [lib.layout_bytes(d, n, k) for d in (0, 1) for n in LAYOUT_NS for k in LAYOUT_CHUNKS],
        "slots_for": [lib.slots_for(*c) for c in SLOT_CASES],
        "device_lists": [lib.parse_devices(*c) for c in DEVICE_LISTS],
        "merge": [lib.merge(*c) for c in MERGE_CASES],
        "inspection_sha256": inspection_digest(lib),
    }


def test_decisions_are_the_parent_commits(lib):
    fx = json.load(open(FIXTURE))
    got = pinned_rows(lib)
    assert len(got["chunks"]) > 150 and len(got["steps"]) > 100 and len(got["splits"]) > 400 and len(got["slots_for"]) == len(SLOT_CASES) > 1000
    names = dict(chunks=[c[0] for c in chunk_cases()], steps=step_cases(), splits=split_cases(), slots_for=SLOT_CASES, device_lists=DEVICE_LISTS, merge=MERGE_CASES)
    for key in ("chunks", "steps", "splits", "slots_for", "device_lists", "merge"):
        assert len(got[key]) == len(fx[key]), key
        bad = [(names[key][i], w, g) for i, (w, g) in enumerate(zip(fx[key], got[key])) if w != g]
        assert not bad, "%s: %d of %d cases differ from the recorded decisions (case, recorded, header); the first: %r" % (key, len(bad), len(got[key]), bad[:3])
    assert got["inspection_sha256"] == fx["inspection_sha256"], "content size, compressed size or block count of some frame, prefix or magicless view differs from the parent's"
    # the device area is the parent's to the byte; the pinned one may only have lost the n dead words the parent's compress carving left between the sizes and the totals
    cases = [(d, n, k) for d in (0, 1) for n in LAYOUT_NS for k in LAYOUT_CHUNKS]
    for (d, n, k), want, have in zip(cases, fx["layout_bytes"], got["layout_bytes"]):
        assert have[0] == want[0] and have[1] <= want[1], (d, n, k, want, have)
        assert have[1] == (want[1] if d == 0 else want[1] - 8 * n), (d, n, k, want, have)


# ------------------------------------------------------------------------------------------ properties
def arrays_of(direction, n, n_chunks):
    """(offset name, bytes per element, elements, the area's reservation name)"""
    if direction:
        return [("dSizes", 8, n, "dBytes"), ("dOffs", 8, n, "dBytes"), ("dTotals", 8, n_chunks + 1, "dBytes"), ("dStatus", 4, n, "dBytes"),
                ("hSizes", 8, n, "hBytes"), ("hTotals", 8, n_chunks + 1, "hBytes"), ("hStatus", 4, n, "hBytes")]
    return [("dSizes", 8, n, "dBytes"), ("dStatus", 4, n, "dBytes"), ("hSizes", 8, n, "hBytes"), ("hStatus", 4, n, "hBytes")]


def test_layouts_do_not_overlap_and_lie_inside_their_reservation(lib):
    fx = json.load(open(FIXTURE))["layout_bytes"]
    parents = dict(zip([(d, n, k) for d in (0, 1) for n in LAYOUT_NS for k in LAYOUT_CHUNKS], fx))
    for d in (0, 1):
        for n in LAYOUT_NS + [7, 1000, 65537]:
            for k in LAYOUT_CHUNKS + [9]:
                l = lib.layout(d, n, k)
                assert [l["dBytes"], l["hBytes"]] == lib.layout_bytes(d, n, k)
                if (d, n, k) in parents:
                    assert l["dBytes"] <= parents[(d, n, k)][0] and l["hBytes"] <= parents[(d, n, k)][1]
                for area in ("dBytes", "hBytes"):
                    spans = sorted((l[name], l[name] + size * cnt, size, name) for name, size, cnt, a in arrays_of(d, n, k) if a == area)
                    for lo, hi, size, name in spans:
                        assert lo % size == 0 and hi <= l[area], (d, n, k, name, l)
                    for (_, hi, _, a), (lo, _, _, b) in zip(spans, spans[1:]):
                        assert hi <= lo, (d, n, k, a, b, l)


def covers(runs, lo, hi):
    """runs [(a, b)] cover [lo, hi) in order, once, none empty"""
    assert all(a < b for a, b in runs), runs
    assert [a for a, _ in runs] == ([lo] + [b for _, b in runs[:-1]] if runs else []) and (runs[-1][1] if runs else lo) == hi, (runs, lo, hi)


def test_cuts_cover_the_batch_in_order(lib):
    for name, a, b, mb, items, first in chunk_cases():
        cuts = lib.chunks(a, b, mb, items, first)
        n = len(a)
        assert cuts[0] == 0 and cuts[-1] == n and (n == 0) == (len(cuts) == 1), name
        covers(list(zip(cuts, cuts[1:])), 0, n)
        ca, cb = [np.concatenate([np.zeros(1, np.uint64), np.cumsum(arr(v), dtype=np.uint64)]) for v in (a, b)]
        for k, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            lim = first if k == 0 and first else items
            assert hi - lo <= lim, (name, k)
            # a chunk closes AT the item that reaches a limit, never later: without its last item it is below every limit
            assert int(ca[hi - 1] - ca[lo]) < mb and int(cb[hi - 1] - cb[lo]) < mb, (name, k)
            if hi < n:
                assert hi - lo == lim or int(ca[hi] - ca[lo]) >= mb or int(cb[hi] - cb[lo]) >= mb, (name, k)


def test_a_chunk_closes_at_the_item_that_reaches_maxbytes(lib):
    """>= , not > : 400 + 600 bytes close a chunk of 1 000, 400 + 599 do not"""
    assert lib.chunks([400, 600, 400, 599, 1, 1], [1] * 6, 1000, 32768) == [0, 2, 5, 6]
    assert lib.chunks([1] * 6, [400, 600, 400, 599, 1, 1], 1000, 32768) == [0, 2, 5, 6]
    assert lib.chunks([400, 599, 400, 599, 1, 1], [1] * 6, 1000, 32768) == [0, 3, 6]
    assert lib.chunks([10, 5000, 10, 10], [1] * 4, 1000, 32768) == [0, 2, 4]
    assert lib.chunks([1] * 5, [1] * 5, 1000, 2) == [0, 2, 4, 5] and lib.chunks([1] * 5, [1] * 5, 1000, 2, 1) == [0, 1, 3, 5]
    assert lib.chunks(np.ones(8193), np.ones(8193), 1 << 30, 32768, 2048) == [0, 2048, 8193]


def test_upload_steps_cover_their_chunk_and_hold_512_mib_unless_one_item(lib):
    big = [600 << 20, 1, 511 << 20, 1 << 20, 1, 0, 0, 512 << 20, 0, 513 << 20, 100 << 20, 200 << 20, 212 << 20, 1]
    assert lib.steps(big, 0, len(big), STAGE) == [(0, 1, 600 << 20), (1, 3, (511 << 20) + 1), (3, 7, (1 << 20) + 1), (7, 9, 512 << 20), (9, 10, 513 << 20), (10, 13, 512 << 20), (13, 14, 1)]
    tables = [(big, STAGE), (mixed(5000, 5, 3 << 20), STAGE), (mixed(300, 6, 700 << 20), STAGE), (np.zeros(100, np.uint64), STAGE)] + [(t, s) for t, _, _, s in step_cases()]
    for lens, stage in tables:
        for lo, hi in ((0, len(lens)), (len(lens) // 3, len(lens) - 1)):
            if lo >= hi:
                continue
            steps = lib.steps(lens, lo, hi, stage)
            covers([(a, b) for a, b, _ in steps], lo, hi)
            for k, (a, b, nbytes) in enumerate(steps):
                assert nbytes == int(np.sum(arr(lens)[a:b], dtype=np.uint64)) and (nbytes <= stage or b - a == 1), (a, b, nbytes)
                if b < hi:
                    assert nbytes + int(lens[b]) > stage, "a step takes every item that still fits"


def test_packing_runs_cover_their_step(lib):
    for t, lo, hi, thr, nt in split_cases() + [(mixed(4000, 7, 1 << 16), 0, 4000, 32 << 20, 8), (mixed(4000, 7, 1 << 16), 5, 3999, 32 << 20, 3), (mixed(10, 8, 1 << 26), 0, 10, 32 << 20, 8)]:
        runs = lib.split(t, lo, hi, thr, nt)
        covers(runs, lo, hi)
        total = int(np.sum(arr(t)[lo:hi], dtype=np.uint64))
        if nt == 1 or total < thr or hi - lo < 2 * nt:
            assert runs == [(lo, hi)], (t, lo, hi, thr, nt)
        else:
            assert len(runs) <= nt
    assert lib.split([100] * 16, 0, 16, 400, 3) == [(0, 5), (5, 10), (10, 16)]          # (by bytes: a run closes before the item that passes its share)
    assert lib.split([1000, 1, 1, 1, 1, 1, 1, 1], 0, 8, 1, 3) == [(0, 1), (1, 2), (2, 8)]      # (an item above a share is a run of its own; the last thread takes the rest)
    assert lib.split([100] * 16, 0, 16, 1601, 3) == [(0, 16)] and lib.split([100] * 5, 0, 5, 1, 3) == [(0, 5)]
    assert lib.split([5], 0, 0, 0, 3) == []


def test_partition_covers_and_is_the_recorded_rule(lib):
    assert lib.partition([10] * 10, 3) == [(0, 4), (4, 8), (8, 10)] and lib.partition([100, 1, 1, 1], 2) == [(0, 1), (1, 4)] and lib.partition([5], 4) == [(0, 1)] and lib.partition([], 4) == []
    for sizes, w in ((list(range(1, 100)), 8), ([131072] * 4096, 8), ([0] * 9, 4), ([7] * 3, 0)):
        covers(lib.partition(sizes, w), 0, len(sizes))


# ------------------------------------------------------------------------------------------ the fan-out's decisions, stated directly
def test_device_list_and_slots(lib):
    assert lib.parse_devices("0,0", 1) == [0, 0] and lib.parse_devices("0,0,0", 1) == [0, 0, 0]          # (a device listed twice: two contexts on one GPU)
    assert lib.parse_devices("7", 1) == [] and lib.parse_devices("", 1) == [] and lib.parse_devices("0,x", 1) == [0]
    assert lib.parse_devices("3,3,9,3", 4) == [3, 3, 3] and lib.parse_devices("-1,0", 8) == [0] and lib.parse_devices("0", 0) == []
    # an explicit list: every slot, but never more than items -- and never "inline"; else never more slots than minBytes of input each, and one slot is inline
    assert lib.slots_for(2, 1, 256 << 20, 100, 0) == 2 and lib.slots_for(3, 1, 256 << 20, 2, 0) == 2 and lib.slots_for(1, 1, 256 << 20, 5, 0) == 1 and lib.slots_for(0, 1, 0, 5, 1 << 40) == 0
    assert lib.slots_for(8, 0, 256 << 20, 100, (512 << 20) - 1) == 0 and lib.slots_for(8, 0, 256 << 20, 100, 512 << 20) == 2 and lib.slots_for(8, 0, 256 << 20, 100, 1 << 40) == 8
    assert lib.slots_for(1, 0, 256 << 20, 100, 1 << 40) == 0 and lib.slots_for(8, 0, 256 << 20, 3, 1 << 40) == 3
    assert lib.slots_for(8, 0, 0, 100, 0) == 8 and lib.slots_for(8, 0, 0, 5, 0) == 5          # (minBytes 0: no floor)


def test_merge_reports_the_lowest_failing_run(lib):
    assert lib.merge([0, 0, 0], [0, 10, 20], [0, 0, 0]) == [3, 0, 0]
    assert lib.merge([0, 3, 1], [0, 10, 20], [0, 4, 7]) == [1, 3, 14]          # (the index counted from the call's first item)
    assert lib.merge([1, 3, 1], [0, 10, 20], [2, 4, 7]) == [0, 1, 2] and lib.merge([0, 0, 5], [0, 10, 20], [0, 0, 0]) == [2, 5, 20]


# ------------------------------------------------------------------------------------------ pass 1: layouts and refusals
NO_SIZE = bytes.fromhex("28b52ffd0000010000")          # an empty frame without a content size
SIZED = bytes.fromhex("28b52ffd2000010000")            # .. with one: 0 bytes
FOO = bytes.fromhex("28b52ffd2003190000666f6f")        # b"foo", content size 3, a raw block
Z = bytes(10)                                          # ten bytes that are no frame: a given size is what counts


def huge(fcs):
    """a frame header that claims fcs bytes in the 8-byte form, and one empty raw block"""
    return craft.frame_header(fcs=fcs, single_segment=True, fcs_bytes=8) + craft.block(0, b"", True)


def test_decompress_segments_and_refusals(lib):
    kind, index, st, dt, segs, nb = lib.decompress_segments([(FOO, 0), (SIZED, 0), (FOO, 7), (NO_SIZE, 5), (b"", 2)])
    assert (kind, st, dt) == (0, 2 * len(FOO) + 18, 3 + 0 + 7 + 5 + 2)
    assert segs == [[0, 12], [12, 9], [21, 12], [33, 9], [42, 0], [0, 3], [3, 0], [3, 7], [10, 5], [15, 2]] and nb == [1, 1, 1, 1, 0]
    assert lib.decompress_segments([])[:4] == (0, 0, 0, 0)
    # unknown size: no content size in the header and none given; a header that cannot be read -- at the first and at the last item
    for bad in (NO_SIZE, b"", b"\x28\xb5\x2f", b"nonsense!", FOO[:5]):
        for items, index in (([(bad, 0), (FOO, 0), (FOO, 0)], 0), ([(FOO, 0), (FOO, 0), (bad, 0)], 2), ([(FOO, 0), (bad, 0), (bad, 0)], 1)):
            assert lib.decompress_segments(items)[:2] == (ERR_UNKNOWN_SIZE, index), (bad, index)
    assert lib.decompress_segments([(FOO[4:], 0), (NO_SIZE[4:], 0)], fmt=1)[:2] == (ERR_UNKNOWN_SIZE, 1) and lib.decompress_segments([(FOO, 0)], fmt=1)[:2] == (ERR_UNKNOWN_SIZE, 0)
    # the 2^46 cap: a single size, given or claimed by a header, and the running total -- the item that crosses it
    assert lib.decompress_segments([(Z, CAP)])[:4] == (0, 0, 10, CAP)
    assert lib.decompress_segments([(Z, CAP + 1), (Z, 1)])[:2] == (ERR_NO_MEMORY, 0) and lib.decompress_segments([(Z, 1), (Z, 1), (Z, CAP + 1)])[:2] == (ERR_NO_MEMORY, 2)
    assert lib.decompress_segments([(Z, 1 << 45), (Z, 1 << 45)])[:4] == (0, 0, 20, CAP)
    assert lib.decompress_segments([(Z, 1 << 45), (Z, 1 << 45), (Z, 1), (Z, 1)])[:2] == (ERR_NO_MEMORY, 2)
    assert lib.decompress_segments([(Z, 1 << 45), (Z, (1 << 45) + 1)])[:2] == (ERR_NO_MEMORY, 1) and lib.decompress_segments([(Z, 2 ** 64 - 1)])[:2] == (ERR_NO_MEMORY, 0)
    assert lib.decompress_segments([(FOO, 0), (huge(CAP + 1), 0)])[:2] == (ERR_NO_MEMORY, 1) and lib.decompress_segments([(huge(CAP), 0)])[:4] == (0, 0, len(huge(CAP)), CAP)
    assert lib.decompress_segments([(huge(CAP + 1), 100)])[:2] == (0, 0)          # (a given size is what counts)
    assert lib.decompress_segments([(NO_SIZE, 0), (Z, CAP + 1)])[:2] == (ERR_UNKNOWN_SIZE, 0)          # (the first item that is refused)


def test_compress_segments_and_refusals(lib):
    sizes = [0, 1, 15, 16, 131071, 131072, 131073, 1 << 20, (1 << 31) - 1]
    kind, index, st, dt, segs, text = lib.compress_segments(sizes)
    assert (kind, text, st) == (0, "", sum(sizes))
    bounds = [s + (s >> 8) + (((128 << 10) - s) >> 11 if s < (128 << 10) else 0) for s in sizes]
    assert [lib.compress_bound(s) for s in sizes] == bounds
    slots = [(b + 15) & ~15 for b in bounds]
    assert [s[1] for s in segs[len(sizes):]] == slots and [s[0] for s in segs[len(sizes):]] == [sum(slots[:i]) for i in range(len(sizes))] and dt == sum(slots)
    assert [s[1] for s in segs[:len(sizes)]] == sizes and [s[0] for s in segs[:len(sizes)]] == [sum(sizes[:i]) for i in range(len(sizes))]
    for items, index in (([1 << 31, 5, 5], 0), ([5, 5, 1 << 31], 2), ([5, (1 << 31) + 1, 1 << 40], 1), ([2 ** 64 - 1], 0)):
        kind, at, _, _, _, text = lib.compress_segments(items)
        assert (kind, at, text) == (ERR_UNSUPPORTED, index, TEXT_2GIB)


# ------------------------------------------------------------------------------------------ verdicts
def test_decompress_verdict(lib):
    dst = [10, 20, 30, 40, 50]
    ok, segs = lib.decompress_verdict(dst, dst, [0] * 5, 0, 5, 0)
    assert ok == (0, 0, 0, 0, 0) and segs == [[0, 10], [10, 20], [30, 30], [60, 40], [100, 50]]
    assert lib.decompress_verdict(dst, dst, [0] * 5, 2, 5, 0) == ((0, 0, 0, 0, 0), [[0, 30], [30, 40], [70, 50]])          # (offsets count from the chunk's first item)
    # the first failing item; its status before its size; the detail words: produced, expected
    assert lib.decompress_verdict(dst, [10, 20, 31, 40, 50], [0, 0, 0, 0, 20], 0, 5, 0)[0] == (ERR_SIZE_MISMATCH, 2, 0, 31, 30)
    assert lib.decompress_verdict(dst, [10, 20, 31, 40, 50], [0, 20, 0, 0, 0], 0, 5, 0)[0] == (ERR_ZSTD, 1, 20, 0, 0)          # (a status at a lower index beats the mismatch)
    assert lib.decompress_verdict(dst, [10, 20, 31, 40, 50], [0, 0, 72, 0, 0], 0, 5, 0)[0] == (ERR_ZSTD, 2, 72, 0, 0)          # (and at the same item)
    assert lib.decompress_verdict(dst, [10, 20, 31, 40, 50], [0, 20, 0, 0, 0], 3, 5, 0)[0] == (0, 0, 0, 0, 0)                  # (other chunks' items are not this chunk's)
    assert lib.decompress_verdict(dst, [10, 20, 30, 40, 49], [0] * 5, 0, 5, 0)[0] == (ERR_SIZE_MISMATCH, 4, 0, 49, 50)
    # allowShort: the expected size is a capacity
    v, segs = lib.decompress_verdict(dst, [10, 0, 29, 40, 50], [0] * 5, 0, 5, 1)
    assert v == (0, 0, 0, 0, 0) and segs == [[0, 10], [10, 0], [30, 29], [60, 40], [100, 50]]          # (every item stays where its capacity put it)
    assert lib.decompress_verdict(dst, [10, 21, 29, 40, 50], [0] * 5, 0, 5, 1)[0] == (ERR_SIZE_MISMATCH, 1, 0, 21, 20)
    assert lib.decompress_verdict(dst, [10, 20, 29, 40, 50], [0] * 5, 0, 5, 0)[0] == (ERR_SIZE_MISMATCH, 2, 0, 29, 30)
    assert lib.decompress_verdict(dst, [10, 21, 29, 40, 50], [0, 0, 0, 0, 107], 4, 5, 1)[0] == (ERR_ZSTD, 4, 107, 0, 0)
    assert lib.decompress_verdict([], [], [], 0, 0, 0) == ((0, 0, 0, 0, 0), [])


def test_compress_verdict(lib):
    sizes = [9, 0, 30, 12]
    assert lib.compress_verdict(sizes, [0] * 4, 0, 4) == ((0, 0, 0, 0, 0, 51), [[0, 9], [9, 0], [9, 30], [39, 12]])
    assert lib.compress_verdict(sizes, [0] * 4, 2, 4) == ((0, 0, 0, 0, 0, 42), [[0, 30], [30, 12]])
    assert lib.compress_verdict(sizes, [0, 70, 0, 40], 0, 4)[0] == (ERR_ZSTD, 1, 70, 0, 0, 0)
    assert lib.compress_verdict(sizes, [0, 70, 0, 40], 2, 4)[0] == (ERR_ZSTD, 3, 40, 0, 0, 0) and lib.compress_verdict(sizes, [0, 70, 0, 40], 2, 3)[0][:2] == (0, 0)


# ------------------------------------------------------------------------------------------ frame inspection against libzstd
def ref_frame_size(ref, data):
    """ZSTD_findFrameCompressedSize as the header's entry reports it: the size, or minus the error code"""
    r = ref.find_frame_compressed_size(data)
    return r if r < 2 ** 63 else -(2 ** 64 - r)


def test_inspection_is_libzstds(lib, ref):
    """content size and compressed size of every frame, and of every proper prefix of the short ones, as ZSTD_getFrameContentSize and ZSTD_findFrameCompressedSize give them -- the
    error CODE, not only the fact. libzstd's two functions take no format, so the magicless views are held to the same frame WITH its magic: the same content size, the same
    error, a size 4 bytes less"""
    frames = inspection_frames()
    assert len(frames) > 100
    checked = errors = 0
    for name, data, fmt in inspection_views(frames):
        if fmt == 0:
            want_cs, want_fs = ref.frame_content_size(data), ref_frame_size(ref, data)
        else:
            full = b"\x28\xb5\x2f\xfd" + data
            want_cs, want_fs = ref.frame_content_size(full), ref_frame_size(ref, full)
            want_fs -= 4 if want_fs > 0 else 0
        assert lib.content_size(data, fmt) == want_cs, (name, data[:80].hex())
        assert lib.frame_size(data, fmt) == want_fs, (name, data[:80].hex())
        checked += 1; errors += want_fs < 0
    assert checked > 3000 and errors > 2000
    seen = {lib.frame_size(d, f) for _, d, f in inspection_views(frames)}
    assert {-ZE_SRC_SIZE_WRONG, -ZE_PREFIX_UNKNOWN} <= seen          # (corruption -- a reserved-type block -- is test_block_counts')
    # skippable frames: the size the header claims, checked against the input
    for magic in (0x184D2A50, 0x184D2A5F):
        for size in (0, 1):
            f = magic.to_bytes(4, "little") + size.to_bytes(4, "little") + b"x" * size
            assert lib.frame_size(f) == ref_frame_size(ref, f) == 8 + size and lib.content_size(f) == ref.frame_content_size(f) == 0 and lib.count_blocks(f) == 0
            assert lib.frame_size(f + b"tail") == 8 + size and lib.frame_size(f[:-1]) == ref_frame_size(ref, f[:-1]) == -ZE_SRC_SIZE_WRONG
    assert lib.frame_size(bytes.fromhex("28b52ffd2800")) == ref_frame_size(ref, bytes.fromhex("28b52ffd2800")) == -ZE_FRAMEPARAM_UNSUPPORTED          # (the reserved bit, in a whole header)


def test_block_counts(lib, ref):
    """host_count_blocks against frames written from explicit block lists: raw, RLE and compressed blocks, 1, 2, 3 and 4 096 of them; a reserved-type block; counts around 65 536"""
    hdr = craft.frame_header(fcs=None)
    makers = {"raw": lambda i: ("raw", bytes([i & 255]) * (i % 5)), "rle": lambda i: ("rle", i & 255, 1 + i % 7), "seq": lambda i: ("seq", b"abcd", [(4, 4, 7)])}
    for count in (1, 2, 3, 4096):
        for kind in ("raw", "rle", "seq", "all"):
            blocks = [makers[("raw", "rle", "seq")[i % 3] if kind == "all" else kind](i) for i in range(count)]
            f = craft.write_frame(blocks, fcs=None)
            assert lib.count_blocks(f) == count and lib.count_blocks(f[4:], 1) == count, (kind, count)
            assert lib.frame_size(f) == ref_frame_size(ref, f) == len(f) and lib.walk(f, len(hdr)) == (count, len(f), WALK_LAST)
            assert lib.count_blocks(f[:-1]) == 0 and lib.walk(f[:-1], len(hdr))[2] == WALK_TRUNCATED and lib.frame_size(f[:-1]) == ref_frame_size(ref, f[:-1]) == -ZE_SRC_SIZE_WRONG
            g = craft.write_frame(blocks, fcs=None, checksum=0x12345678)
            assert lib.count_blocks(g) == count and lib.frame_size(g) == ref_frame_size(ref, g) == len(g) == len(f) + 4 and lib.frame_size(g[:-1]) == -ZE_SRC_SIZE_WRONG
    # a block of the reserved type: no count, and the compressed size is "corruption", wherever it stands
    for lead in (0, 1, 2):
        f = hdr + b"".join(craft.block(0, b"ab", False) for _ in range(lead)) + craft.block(3, b"zz", True) + craft.block(0, b"", True)
        assert lib.count_blocks(f) == 0 and lib.frame_size(f) == ref_frame_size(ref, f) == -ZE_CORRUPTION
        assert lib.walk(f, len(hdr)) == (lead, len(hdr) + 5 * lead, WALK_RESERVED)
    # 65 536 blocks are counted; a frame whose first 65 536 blocks are not its last is not followed further -- its size still is
    for count, want in ((65535, 65535), (65536, 65536), (65537, 0), (70000, 0)):
        f = hdr + b"\x00\x00\x00" * (count - 1) + b"\x01\x00\x00"
        assert lib.count_blocks(f) == want and lib.frame_size(f) == ref_frame_size(ref, f) == len(f), count
    assert lib.count_blocks(hdr + b"\x00\x00\x00" * 65536) == 0 and lib.frame_size(hdr + b"\x00\x00\x00" * 65536) == -ZE_SRC_SIZE_WRONG
    assert lib.count_blocks(b"") == 0 and lib.count_blocks(b"nonsense!") == 0


# ------------------------------------------------------------------------------------------ what a context gives back after a call
MIB = 1 << 20
TRIM_FLOOR = 64 * MIB


def trim_rule(caps, trimmable, keep):
    """the rule, restated: while the buffers total more than keep, the largest trimmable one above 64 MiB goes (of equals the earlier one)"""
    caps, order = list(caps), []
    while sum(caps) > keep and any(t and c > TRIM_FLOOR for c, t in zip(caps, trimmable)):
        order.append(max((i for i, t in enumerate(trimmable) if t and caps[i] > TRIM_FLOOR), key=lambda i: (caps[i], -i)))
        caps[order[-1]] = 0
    return order


def test_trim_order_of_a_baseline_shaped_context(lib):
    """the 14 trimmable buffers of a thread's context after multi_compress_to_buffer and multi_decompress_to_buffer of 65 536 x 128 KiB at level 3 on 256 CUs (golden: each capacity
    is reserve()'s n + n/8 + 4096 over the parent's plans -- compress chunks of 32 768 sources, decompress chunks of 2 048 and 8 192 frames, the staging arenas of the whole batch),
    under the default 64 GiB, under limits that cut into them, and with untrimmable buffers beside them"""
    fx = json.load(open(FIXTURE))["trim_caps_baseline"]
    names, caps = fx["names"], fx["caps"]
    assert len(names) == len(caps) == 14 and 50 << 30 < sum(caps) < 64 << 30
    assert lib.trim_order(caps, [1] * 14, 64 << 30) == []
    assert [names[i] for i in lib.trim_order(caps, [1] * 14, 48 << 30)] == ["encFlatTables"]
    assert [names[i] for i in lib.trim_order(caps, [1] * 14, 16 << 30)] == ["encFlatTables", "encArena", "hDst", "hDense"]          # (hDst and hDense are equals: the earlier first)
    for keep in (0, 1 << 30, 2 << 30, 16 << 30, 32 << 30, 48 << 30, sum(caps) - 1, sum(caps), 64 << 30):
        assert lib.trim_order(caps, [1] * 14, keep) == trim_rule(caps, [1] * 14, keep), keep
        # .. with 30 small buffers that never go, and one large one that may not
        more, flags = caps + [4096] * 30 + [20 << 30], [1] * 14 + [0] * 31
        got = lib.trim_order(more, flags, keep)
        assert got == trim_rule(more, flags, keep) and all(i < 14 for i in got), keep
    assert len(lib.trim_order(caps, [1] * 14, 0)) == sum(c > TRIM_FLOOR for c in caps) == 10          # keep nothing: everything above the floor, nothing at or below it


def test_trim_order_synthetic(lib):
    f = TRIM_FLOOR
    cases = [([f + 1, f + 1, f + 1], [1, 1, 1], 0), ([f + 1, f + 2, f + 1, f + 2], [1, 1, 1, 1], f),                     # ties
             ([f, f, f - 1, 1, 0], [1] * 5, 0), ([f] * 20, [1] * 20, f),                                                # all at or below the floor: nothing goes, whatever the total
             ([f + 1, f, 5 * f], [1, 1, 1], 0), ([f + 1, f, 5 * f], [0, 1, 0], 0), ([f + 1, f, 5 * f], [1, 0, 0], 0),       # keep 0; flags
             ([3 * f, 2 * f], [1, 1], 5 * f), ([3 * f, 2 * f], [1, 1], 5 * f - 1), ([3 * f, 2 * f, f], [1, 1, 1], 3 * f),      # already under keep; just above it
             ([], [], 0), ([0], [1], 0)]
    for caps, flags, keep in cases:
        assert lib.trim_order(caps, flags, keep) == trim_rule(caps, flags, keep), (caps, flags, keep)
    assert lib.trim_order([f + 1, f + 1, f + 1], [1, 1, 1], 0) == [0, 1, 2]
    assert lib.trim_order([f, f + 1], [1, 1], 0) == [1]                        # the floor itself stays: strictly above 64 MiB
    assert lib.trim_order([3 * f, 2 * f], [1, 1], 5 * f) == [] and lib.trim_order([3 * f, 2 * f], [1, 1], 5 * f - 1) == [0]


# ------------------------------------------------------------------------------------------ the payload pool
PIN_MIN = 1 << 20


def pool_cap(n):
    return (n + 2 * MIB - 1) & ~(2 * MIB - 1)


def pool_model(keep, ops):
    """the pool's policy restated over capacities: per op (allocated now, capacity asked, idle bytes after), and the capacities unpinned in order"""
    idle, busy, rows, freed, refuse = [], {}, [], [], False
    for k, (kind, a) in enumerate(ops):
        row = (0, 0)
        if kind == "take" and a >= PIN_MIN:
            fit = [c for c in idle if c >= a]
            if fit and min(fit) <= a + a // 2 + 64 * MIB:
                idle.remove(min(fit)); busy[k] = min(fit)
            elif not refuse:
                busy[k] = pool_cap(a); row = (1, pool_cap(a))
        elif kind == "give" and a in busy:
            idle.append(busy.pop(a))
            while sum(idle) > keep:
                freed.append(max(idle)); idle.remove(max(idle))
        elif kind == "refuse":
            refuse = bool(a)
        rows.append(row + (sum(idle),))
    return rows, freed


def test_pool_small_requests_never_reach_the_allocator(lib):
    ops = [("take", 0), ("take", 1), ("take", PIN_MIN - 1), ("give", 0), ("give", 1), ("give", 2)]
    rows, tail, freed = lib.pool_script(24 << 30, ops)
    assert tail == dict(allocs=0, unpins=0, unknown=0, live=0) and freed == [] and all(r[1] == 0 and r[3] == 0 for r in rows)
    rows, tail, _ = lib.pool_script(24 << 30, [("take", PIN_MIN)])
    assert rows[0][1:3] == [1, 2 * MIB] and tail["allocs"] == 1          # 1 MiB itself is pinned, in a block of 2 MiB


def test_pool_reuses_inside_the_window_only(lib):
    # a 70 MiB block is the largest a 4 MiB request still takes (4 + 4/2 + 64); a 72 MiB one stays idle and a new block is pinned
    rows, tail, _ = lib.pool_script(24 << 30, [("take", 70 * MIB), ("give", 0), ("take", 4 * MIB), ("give", 2), ("take", 70 * MIB)])
    assert rows[2][:2] == [0, 0] and rows[4][:2] == [0, 0] and tail["allocs"] == 1          # both served by the block op 0 pinned
    rows, tail, _ = lib.pool_script(24 << 30, [("take", 72 * MIB), ("give", 0), ("take", 4 * MIB), ("take", 71 * MIB)])
    assert rows[2][1:3] == [1, 4 * MIB] and rows[2][0] == 2 and rows[2][3] == 72 * MIB          # the idle one is outside the window: a new 4 MiB block
    assert rows[3][:2] == [0, 0] and rows[3][3] == 0 and tail["allocs"] == 2                        # .. and serves the request it fits
    # best fit: the smallest idle block that holds the request
    rows, _, _ = lib.pool_script(24 << 30, [("take", 40 * MIB), ("take", 20 * MIB), ("take", 30 * MIB), ("give", 0), ("give", 1), ("give", 2), ("take", 25 * MIB), ("take", 25 * MIB), ("take", 25 * MIB)])
    assert [r[0] for r in rows[6:]] == [2, 0, 8] and [r[1] for r in rows[6:]] == [0, 0, 1]          # the 30, then the 40, then a new one (the 20 is too small)


def test_pool_keeps_at_most_keep_idle_bytes_largest_dropped_first(lib):
    rng = np.random.default_rng(7)
    for keep in (0, 10 * MIB, 64 * MIB, 200 * MIB, 24 << 30):
        ops, held = [], []
        for k in range(300):
            if held and rng.random() < 0.5:
                ops.append(("give", held.pop(int(rng.integers(len(held))))))
            else:
                ops.append(("take", int(rng.choice([PIN_MIN, 3 * MIB, 5 * MIB + 1, 17 * MIB, 64 * MIB, 100 * MIB, 130 * MIB])))); held.append(k)
        ops += [("give", k) for k in held]
        rows, tail, freed = lib.pool_script(keep, ops)
        want_rows, want_freed = pool_model(keep, ops)
        assert [tuple(r[1:]) for r in rows] == want_rows and freed == want_freed, keep
        assert all(r[3] <= keep for r in rows) and tail["unknown"] == 0
        assert tail["allocs"] == tail["unpins"] + tail["live"] and (keep or tail["live"] == 0)          # keep 0, everything given back: every block unpinned exactly once
    # the largest idle block goes, not the one just given: under a limit of 25 MiB the 30 goes when it comes and the 20 when it comes; then the 20 although the 10 came first
    _, _, freed = lib.pool_script(25 * MIB, [("take", 10 * MIB), ("take", 30 * MIB), ("take", 20 * MIB), ("give", 0), ("give", 1), ("give", 2)])
    assert freed == [30 * MIB, 20 * MIB]
    _, _, freed = lib.pool_script(25 * MIB, [("take", 60 * MIB), ("give", 0), ("take", 10 * MIB), ("take", 30 * MIB), ("take", 20 * MIB), ("give", 2), ("give", 4), ("give", 3)])
    assert freed == [60 * MIB, 20 * MIB, 30 * MIB]


def test_pool_frees_what_it_does_not_know_and_falls_back_to_malloc(lib):
    ops = [("foreign", 100), ("take", 8 * MIB), ("foreign", 5 * MIB), ("give", 1), ("refuse", 1), ("take", 50 * MIB), ("give", 5), ("refuse", 0), ("take", 50 * MIB), ("give", 8)]
    rows, tail, freed = lib.pool_script(0, ops)
    assert tail == dict(allocs=2, unpins=2, unknown=0, live=0) and freed == [8 * MIB, 50 * MIB]          # the refused request was malloc()ed and free()d: it never counted as a block
    assert rows[5][1] == 0 and rows[6][3] == 0


# ------------------------------------------------------------------------------------------ device slots and the fan-out
def test_device_pool_reads_its_environment_as_arguments(lib):
    assert lib.pool_parse(4, None, None) == (False, 256 << 20, [0, 1, 2, 3])
    assert lib.pool_parse(0, None, None) == (False, 256 << 20, [])
    assert lib.pool_parse(4, "0,0", "1000") == (True, 1000, [0, 0])
    assert lib.pool_parse(2, "1,5,0", "0") == (True, 0, [1, 0])
    assert lib.pool_parse(2, "", None) == (True, 256 << 20, [])


FAN_SIZES = [[1], [0], [5, 5], [0, 0, 0], [1, 2, 3, 4, 5, 6, 7, 8], [0, 9, 0, 0, 9, 0, 0, 0, 9], [100] + [1] * 12, [1] * 12 + [100], [0] * 13]


def test_fan_out_returns_the_items_in_order(lib):
    for sizes in FAN_SIZES:
        for d in range(1, 9):
            runs = lib.partition(sizes, d)
            assert runs and all(lo < hi for lo, hi in runs) and len(runs) <= min(d, len(sizes))          # fewer items than slots, items of no bytes: never an empty run
            r = lib.fan_out(sizes, [0] * len(sizes), d)
            assert r["rc"] == 0 and r["order"] == list(range(len(sizes))) and r["text"] == "", (sizes, d, r)
            assert r["runs"] == r["afters"] == len(runs) and r["empty_runs"] == 0 and r["freed"] == 0 and r["live"] == 0, (sizes, d, r)
            assert r["bound_own_device"] == 1 and r["bound"] >= len(runs)


def test_fan_out_reports_the_lowest_failing_run_and_frees_the_others(lib):
    sizes = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13]
    for d in range(1, 9):
        runs = lib.partition(sizes, d)
        for bad in ([0], [12], [3, 9], [12, 0, 6], list(range(13))):
            for mode, rc, zerr, text in ((1, ERR_ZSTD, 70, "stub: run failed"), (2, ERR_NO_MEMORY, 0, "out of host memory"), (3, ERR_HIP, 0, "stub: boom")):
                modes = [mode if i in bad else 0 for i in range(13)]
                failing = [w for w, (lo, hi) in enumerate(runs) if any(lo <= i < hi for i in bad)]
                lo, hi = runs[failing[0]]
                first = min(i for i in bad if lo <= i < hi)
                r = lib.fan_out(sizes, modes, d)
                # a run that returns an error reports its item; one that throws reports its first (index 0 of the run)
                assert (r["rc"], r["kind"], r["zerr"], r["text"]) == (rc, rc, zerr, text) and r["index"] == (first if mode == 1 else lo), (d, bad, mode, r)
                assert r["outputs"] == 0 and r["live"] == 0 and r["freed"] == sum(h - l for w, (l, h) in enumerate(runs) if w not in failing), (d, bad, mode, r)
                assert r["runs"] == r["afters"] == len(runs)
    # two kinds of failure in one call: the lowest run wins whatever it is
    r = lib.fan_out(sizes, [0] * 5 + [3] + [0] * 6 + [1], 4)
    assert (r["rc"], r["text"]) == (ERR_HIP, "stub: boom")


# ------------------------------------------------------------------------------------------ the sanitizer program
def test_bounds_program_is_clean(tmp_path):
    """AddressSanitizer + UBSan over layout -> cuts -> steps -> pack_items (three threads) -> the "device" copy -> both meta layouts -> the verdicts, every buffer a heap block
    of exactly the planned bytes; then the payload pool over blocks of exactly their capacity, the trim order and the fan-out over 1 to 8 stub slots with clean, failing and throwing
    runs, LeakSanitizer counting what is left: a stand-alone program (tests/emu/host_calls_main.cpp), nothing sanitized is loaded into this process"""
    exe = str(tmp_path / "host_calls")
    subprocess.check_call(["sh", os.path.join(HERE, "emu", "build_host_calls.sh"), exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and r.stdout.startswith("ok: ") and int(r.stdout.split()[1]) >= 36 + 5 + 480, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])      # + the pool, the trim order, the fan-out
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr and r.stderr == "", r.stderr[-4000:]


def test_threads_program_is_clean(tmp_path):
    """ThreadSanitizer over what only ever ran on several threads inside the library: host_fan_out called back to back from 4 threads over 3 shared slots with runs that return at
    once (a worker is then still between its count-down and its notify when its caller returns), and PinPool::take / give from 8 threads. A stand-alone program
    (tests/emu/host_pool_tsan_main.cpp), nothing sanitized is loaded into this process"""
    exe = str(tmp_path / "host_pool_tsan")
    subprocess.check_call(["sh", os.path.join(HERE, "emu", "build_host_pool_tsan.sh"), exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok: 6000 fan-out calls"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]


def _record():
    """writes the fixture from ZHIP_PLAN_SO: a library with the same entries that holds the PARENT commit's lines, never the header's"""
    assert os.environ.get("ZHIP_PLAN_SO"), "the fixture is recorded from the parent commit's decisions: name that library in ZHIP_PLAN_SO"
    rows = pinned_rows(HcLib())
    rows["trim_caps_baseline"] = json.load(open(FIXTURE))["trim_caps_baseline"]          # (worked out from the plans' formulas, not recorded: kept as it is)
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(' "%s": [\n%s\n ]' % (k, ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in v)) if isinstance(v, list) else ' "%s": %s' % (k, json.dumps(v))
                                     for k, v in rows.items()) + "\n}\n")
    print({k: (len(v) if isinstance(v, list) else v) for k, v in rows.items()}, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        _record()
