"""ctypes binding of tests/emu/libzhip_emu.so (product kernels compiled for the host wave emulator)."""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EMU_SO = os.environ.get("ZHIP_EMU_SO") or os.path.join(_DIR, "libzhip_emu.so")      # ZHIP_EMU_SO: e.g. the ASan build (tests/emu/build_asan.sh)


def build():
    subprocess.check_call(["sh", os.path.join(_DIR, "build.sh")])


def build_variant(out_path, defines):
    """the same sources with extra -D flags (experimental kernel variants), e.g. ["-DZP_K3_LONGONE"]"""
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + _DIR, "-Wno-unused-function", "-Wno-unused-variable"] + list(defines) +
                          ["-o", out_path, os.path.join(_DIR, "zhemu.cpp"), os.path.join(_DIR, "emu_kernels.cpp")])
    return out_path


class Emu:
    def __init__(self, so_path=None):
        path = so_path or EMU_SO
        if not os.path.exists(path):
            build()
        self.lib = C.CDLL(path)
        if os.environ.get("ZHIP_EMU_PROBES"):                    # stress campaigns: the flat search at four probes per trip (the product's form for chunks up to 32 768 sources)
            self.lib.emu_set_probes(C.c_uint32(int(os.environ["ZHIP_EMU_PROBES"])))

    def set_cparams(self, window_log=0, chain_log=0, hash_log=0, search_log=0, min_match=0, target_length=0, strategy=0, magicless=False):
        """explicit compression parameters / frame format of the following emulated launches (all zero / False = defaults)"""
        self.lib.emu_set_cparams(C.c_uint32(window_log), C.c_uint32(chain_log), C.c_uint32(hash_log), C.c_uint32(search_log),
                                 C.c_uint32(min_match), C.c_uint32(target_length), C.c_int32(strategy), C.c_uint32(1 if magicless else 0))

    def parse_dict(self, dict_bytes):
        """returns (entropy blob or None, content bytes, dictID) using the device dictionary parser under emulation"""
        import struct
        size = self.lib.emu_dict_entropy_size()
        blob = C.create_string_buffer(size)
        d = np.frombuffer(dict_bytes, dtype=np.uint8).copy()
        st = self.lib.emu_parse_dict(d.ctypes.data_as(C.c_void_p), C.c_uint32(len(d)), blob)
        if st:
            raise RuntimeError("dict parse error %d" % st)
        content_off, dict_id, status = struct.unpack_from("<IIi", blob.raw, size - 12)
        huf_count = struct.unpack_from("<I", blob.raw, 256)[0]
        return (blob if huf_count else None), dict_bytes[content_off:], dict_id

    def decompress_batch(self, frames, sizes, n_blocks=2, dict_content=None, dict_id=0, dict_entropy=None, pads=None):
        n = len(frames)
        if pads is None:
            src = np.frombuffer(b"".join(frames) + b"\0" * 0, dtype=np.uint8).copy()
            src_segs = np.zeros((n, 2), dtype=np.uint64)
            o = 0
            for i, f in enumerate(frames):
                src_segs[i] = (o, len(f)); o += len(f)
        else: src, src_segs = _padded_arena(frames, pads)
        dst_segs = np.zeros((n, 2), dtype=np.uint64)
        o = 0
        for i, s in enumerate(sizes):
            dst_segs[i] = (o, s); o += s
        dst = np.zeros(max(o, 1), dtype=np.uint8)
        out_sizes = np.zeros(n, dtype=np.uint64)
        status = np.full(n, -1, dtype=np.int32)
        dc = np.frombuffer(dict_content, dtype=np.uint8).copy() if dict_content else None
        self.lib.emu_decompress_batch(
            src.ctypes.data_as(C.c_void_p), src_segs.ctypes.data_as(C.c_void_p), C.c_uint32(n),
            dst.ctypes.data_as(C.c_void_p), dst_segs.ctypes.data_as(C.c_void_p),
            out_sizes.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p),
            dc.ctypes.data_as(C.c_void_p) if dc is not None else None, C.c_uint32(len(dc) if dc is not None else 0),
            C.c_uint32(dict_id), dict_entropy, C.c_uint32(n_blocks))
        outs = []
        for i in range(n):
            a = int(dst_segs[i][0])
            outs.append(dst[a:a + int(out_sizes[i])].tobytes())
        return outs, status.tolist()


def _emu_compress_batch(self, raws, level=3, flags=5, n_blocks=2, pipeline=False, chunk=0, dict_data=None):
    n = len(raws)
    if dict_data:
        d = np.frombuffer(dict_data, dtype=np.uint8).copy()
        st = self.lib.emu_set_cdict(d.ctypes.data_as(C.c_void_p), C.c_uint32(len(d)), C.c_int(level))
        if st:
            raise RuntimeError("cdict error %d" % st)
    else:
        self.lib.emu_set_cdict(None, C.c_uint32(0), C.c_int(level))
    src = np.frombuffer(b"".join(raws) + b"\0" * 16, dtype=np.uint8).copy()
    src_segs = np.zeros((n, 2), dtype=np.uint64)
    dst_segs = np.zeros((n, 2), dtype=np.uint64)
    o = d = 0
    for i, r in enumerate(raws):
        src_segs[i] = (o, len(r)); o += len(r)
        b = len(r) + (len(r) >> 8) + (((128 << 10) - len(r)) >> 11 if len(r) < (128 << 10) else 0)
        dst_segs[i] = (d, b); d += b
    dst = np.zeros(max(d, 1) + 16, dtype=np.uint8)
    out_sizes = np.zeros(n, dtype=np.uint64)
    status = np.full(n, -1, dtype=np.int32)
    args = [src.ctypes.data_as(C.c_void_p), src_segs.ctypes.data_as(C.c_void_p), C.c_uint32(n),
            dst.ctypes.data_as(C.c_void_p), dst_segs.ctypes.data_as(C.c_void_p),
            out_sizes.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p),
            C.c_int(level), C.c_uint32(flags), C.c_uint32(n_blocks)]
    if pipeline:
        self.lib.emu_compress_pipeline(*args, C.c_uint32(chunk))
    else:
        self.lib.emu_compress_batch(*args)
    outs = [dst[int(dst_segs[i][0]):int(dst_segs[i][0]) + int(out_sizes[i])].tobytes() for i in range(n)]
    return outs, status.tolist()


Emu.compress_batch = _emu_compress_batch


def _padded_arena(frames, pads):
    """frames with pads[i] filler bytes in front of frame i, in an arena whose first byte lies at a multiple of 64: (arena, segments). The offsets are
    then absolute alignments, so a test can place a bit stream at a chosen offset mod 16."""
    total = sum(pads) + sum(len(f) for f in frames)
    raw = np.full(total + 16 + 64, 0x3C, dtype=np.uint8)
    src = raw[(-raw.ctypes.data) % 64:][:total + 16]
    assert src.ctypes.data % 64 == 0
    segs = np.zeros((len(frames), 2), dtype=np.uint64)
    o = 0
    for i, f in enumerate(frames):
        o += pads[i]
        src[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
        segs[i] = (o, len(f)); o += len(f)
    return src, segs


def _emu_decompress_pipeline(self, frames, sizes, n_blocks=2, chunk=0, pads=None):
    n = len(frames)
    if pads is None:
        src = np.frombuffer(b"".join(frames) + b"\0" * 16, dtype=np.uint8).copy()
        src_segs = np.zeros((n, 2), dtype=np.uint64)
        o = 0
        for i, f in enumerate(frames):
            src_segs[i] = (o, len(f)); o += len(f)
    else: src, src_segs = _padded_arena(frames, pads)
    dst_segs = np.zeros((n, 2), dtype=np.uint64)
    o = 0
    for i, s in enumerate(sizes):
        dst_segs[i] = (o, s); o += s
    dst = np.zeros(max(o, 1) + 16, dtype=np.uint8)
    out_sizes = np.zeros(n, dtype=np.uint64)
    status = np.full(n, -1, dtype=np.int32)
    nfb = self.lib.emu_decompress_pipeline(src.ctypes.data_as(C.c_void_p), src_segs.ctypes.data_as(C.c_void_p), C.c_uint32(n),
                                           dst.ctypes.data_as(C.c_void_p), dst_segs.ctypes.data_as(C.c_void_p),
                                           out_sizes.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p),
                                           C.c_uint32(n_blocks), C.c_uint32(chunk))
    outs = [dst[int(dst_segs[i][0]):int(dst_segs[i][0]) + int(out_sizes[i])].tobytes() for i in range(n)]
    return outs, status.tolist(), nfb


Emu.decompress_pipeline = _emu_decompress_pipeline


def _emu_set_ddict(self, dict_data, raw_content=False):
    """decompression dictionary of the pipeline harness (None: no dictionary); returns the zstd error code of its digestion, 0 = fine"""
    if not dict_data:
        return self.lib.emu_set_ddict(None, C.c_uint32(0), C.c_int(0))
    d = np.frombuffer(dict_data, dtype=np.uint8).copy()
    return self.lib.emu_set_ddict(d.ctypes.data_as(C.c_void_p), C.c_uint32(len(d)), C.c_int(1 if raw_content else 0))


Emu.set_ddict = _emu_set_ddict


def _emu_set_blocks(self, per_frame):
    """several-block mode of the decode pipeline harness: item slots per frame (0 = off: frames of several blocks go to the generic kernel)"""
    self.lib.emu_set_blocks(C.c_uint32(per_frame))


Emu.set_blocks = _emu_set_blocks


def _emu_set_mb_compress(self, v):
    """sources of several blocks in the flat match kernel of the compress pipeline harness: 0 off (the generic kernel searches them), 1 on,
    > 1 on with that many block slots per frame"""
    self.lib.emu_set_mb_compress(C.c_uint32(v))


def _emu_set_mb_hint(self, v):
    """size the several-block compress arenas from this hint instead of the batch's largest source (0 = the largest source): what a device-API
    caller's stale zhip_ctx_set_size_hint does"""
    self.lib.emu_set_mb_hint(C.c_uint64(v))


def _emu_set_dict_slot_max(self, v):
    """dictionary batches: the match kernels take sources up to v bytes (their slots' size under a caller's size hint), larger ones go to the generic kernel; 0 = the attach cutoff"""
    self.lib.emu_set_dict_slot_max(C.c_uint32(v))


def _emu_stat(self, i):
    self.lib.emu_stat.restype = C.c_long
    return int(self.lib.emu_stat(C.c_int(i)))


Emu.set_mb_compress = _emu_set_mb_compress
Emu.set_mb_hint = _emu_set_mb_hint
Emu.set_dict_slot_max = _emu_set_dict_slot_max
Emu.stat = _emu_stat


def _emu_set_k0(self, v):
    """1 (default, as the product): K0 -- a lane per frame walks K1's serial descriptions -- runs before K1; 0: K1 parses everything itself"""
    self.lib.emu_set_k0(C.c_uint32(v))


Emu.set_k0 = _emu_set_k0


def _emu_set_dict_epochs(self, v):
    """1: the flat dictionary search's tables persist between calls and carry launch numbers in their cells (the product's way); 0 (default): the kernel's waves zero them"""
    self.lib.emu_set_dict_epochs(C.c_uint32(v))


Emu.set_dict_epochs = _emu_set_dict_epochs


def _emu_set_check_later(self, v):
    """1 (default, as the product): content checksums are verified by KX after K3, a lane per frame; 0: by K1 / K3 on one lane at the frame's end"""
    self.lib.emu_set_check_later(C.c_uint32(v))


Emu.set_check_later = _emu_set_check_later


# ---- the entropy kernel driven by explicit sequences (tests/emu/emu_entropy_sequences.cpp: a library of its own beside libzhip_emu.so, built by the same build.sh)
SEQ_SO = os.path.join(_DIR, "libzhip_emu_entropy_sequences.so")
_PARAM_ORDER = ("window_log", "chain_log", "hash_log", "search_log", "min_match", "target_length", "strategy")


def _seq_lib(self):
    lib = getattr(self, "_seqlib", None)
    if lib is None:
        if not os.path.exists(SEQ_SO):
            build()
        lib = self._seqlib = C.CDLL(SEQ_SO)
        lib.emu_seq_set_cdict.restype = C.c_int
        lib.emu_seq_set_cdict.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_int]
        lib.emu_seq_dict_rep.restype = C.c_uint32; lib.emu_seq_dict_rep.argtypes = [C.c_int]
        lib.emu_seq_capacity.restype = C.c_uint32
        lib.emu_entropy_sequences.restype = C.c_int
        lib.emu_entropy_sequences.argtypes = [C.c_void_p] * 9 + [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    return lib


def _emu_seq_set_dict(self, dict_data, level=3, params=None, raw_dict=False):
    """digests the compression dictionary of the following entropy_sequences calls (None: no dictionary) with the product's kernels under emulation; returns
    the repeat offsets frames then start from (1, 4, 8 without a dictionary or with a raw-content one)"""
    lib = _seq_lib(self)
    ov = np.array([(params or {}).get(k, 0) for k in _PARAM_ORDER], dtype=np.int32)
    if dict_data:
        d = np.frombuffer(dict_data, dtype=np.uint8).copy()
        st = lib.emu_seq_set_cdict(d.ctypes.data, len(d), level, ov.ctypes.data, 1 if raw_dict else 0)
        if st:
            raise RuntimeError("cdict error %d" % st)
    else:
        lib.emu_seq_set_cdict(None, 0, level, ov.ctypes.data, 0)
    return tuple(int(lib.emu_seq_dict_rep(i)) for i in range(3))


def _emu_entropy_sequences(self, sources, packed, level=3, flags=5, load_flags=0, params=None, dict_data=None, raw_dict=False, magicless=False, n_blocks=3, chunk=0):
    """the loader, the entropy kernel and the trailer kernel under emulation, as zhip_compress_sequences_device launches them. sources: bytes per item; packed:
    a uint64 array of packed sequences per item; flags: 1 content size, 2 checksum, 4 dictionary ID; load_flags bit 0: the loader copies the literals.
    Returns (frames, statuses). Destination slots are zhip_compress_bound-sized, back to back."""
    lib = _seq_lib(self)
    ov = np.array([(params or {}).get(k, 0) for k in _PARAM_ORDER], dtype=np.int32)
    _emu_seq_set_dict(self, dict_data, level, params, raw_dict)
    n = len(sources)
    lens = np.array([len(r) for r in sources], dtype=np.uint64)
    caps = lens + (lens >> np.uint64(8)) + np.where(lens < (128 << 10), (np.uint64(128 << 10) - np.minimum(lens, np.uint64(128 << 10))) >> np.uint64(11), 0).astype(np.uint64)
    ssegs = np.zeros((n, 2), dtype=np.uint64); ssegs[:, 1] = lens; ssegs[1:, 0] = np.cumsum(lens)[:-1]
    dsegs = np.zeros((n, 2), dtype=np.uint64); dsegs[:, 1] = caps; dsegs[1:, 0] = np.cumsum(caps)[:-1]
    counts = np.array([len(q) for q in packed], dtype=np.uint64)
    qsegs = np.zeros((n, 2), dtype=np.uint64); qsegs[:, 1] = counts; qsegs[1:, 0] = np.cumsum(counts)[:-1]
    src = np.frombuffer(b"".join(sources), dtype=np.uint8).copy() if lens.sum() else np.zeros(1, dtype=np.uint8)
    seqs = np.concatenate([np.asarray(q, dtype=np.uint64) for q in packed] + [np.zeros(1, dtype=np.uint64)])
    dst = np.zeros(int(caps.sum()) + 1, dtype=np.uint8)
    sizes = np.zeros(n, dtype=np.uint64); st = np.full(n, -1, dtype=np.int32)
    lib.emu_entropy_sequences(src.ctypes.data, ssegs.ctypes.data, n, seqs.ctypes.data, qsegs.ctypes.data, dst.ctypes.data, dsegs.ctypes.data, sizes.ctypes.data, st.ctypes.data,
                              level, ov.ctypes.data, flags | (8 if magicless else 0), load_flags, n_blocks, chunk)
    return [dst[int(dsegs[i, 0]): int(dsegs[i, 0] + sizes[i])].tobytes() for i in range(n)], st.tolist()


def _emu_seq_capacity(self):
    return int(_seq_lib(self).emu_seq_capacity())


Emu.entropy_sequences = _emu_entropy_sequences
Emu.seq_set_dict = _emu_seq_set_dict
Emu.seq_capacity = _emu_seq_capacity
