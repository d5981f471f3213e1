"""Device-resident batch API: frames already in HBM in, frames in HBM out (torch tensors only carry the memory).

This is the same hot path as ``multi_*_to_buffer`` without the PCIe hops, and it is what shards across GPUs:
each rank owns a contiguous range of frames (the reference's partition rule, c-ext/compressor.c:1127-1216) and
results stay resident per GPU.
"""
import ctypes as C

import torch

from . import _lib
from .backend_hip import ZstdError


def _filter_code(filter):
    """the filter of a typed seekable stream, None or "delta" -> ZHIP_FILTER_NONE / ZHIP_FILTER_DELTA"""
    if filter is None:
        return 0
    if filter == "delta":
        return 1
    raise ZstdError("filter must be None or \"delta\"")


def _base_filter(filter, base):
    """filter and base of a typed call -> True where the call is the xor-with-base one: ``base=`` alone selects it, "xor_base" is its name"""
    if base is None:
        if filter == "xor_base":
            raise ZstdError("filter \"xor_base\" needs base=, the tensor to XOR with")
        return False
    if filter not in (None, "xor_base"):
        raise ZstdError("a base goes with filter \"xor_base\" (or no filter argument), not with %r" % (filter,))
    return True


def _base_bytes(base, like, nbytes, what):
    """base as the uint8 view the calls take: a contiguous CUDA tensor on like's device, nbytes long"""
    if not (isinstance(base, torch.Tensor) and base.is_cuda and base.is_contiguous() and base.device == like.device):
        raise ZstdError("%s: base must be a contiguous CUDA tensor on the source's device" % what)
    raw = base.view(torch.uint8).reshape(-1)
    if raw.numel() != nbytes:
        raise ZstdError("%s: the base has %d bytes, the tensor %d" % (what, raw.numel(), nbytes))
    return raw


class DeviceBatchContext:
    """Owns the native context (scratch, dictionary tables, kernel timers) for one GPU / one stream."""

    def __init__(self, dict_data=None, level=3, write_checksum=False, write_content_size=True, write_dict_id=True, dict_type=0,
                 format=0, max_window_size=0, match_finder="libzstd", **cparams):
        """dict_data: a ZstdCompressionDict (or bytes) used by both directions; level / write_* / cparams (window_log, hash_log,
        chain_log, min_match, target_length, strategy): what ZstdCompressor takes; format / max_window_size: what ZstdDecompressor takes.
        match_finder: "libzstd" (the default: frames byte for byte libzstd's), "wave", "none" (no search: literals-only frames, for numeric tensors) or "auto" ("none" or "libzstd",
        chosen per source) -- see set_match_finder."""
        self.ctx = None
        if match_finder not in self.MATCH_FINDERS:                      # (before anything native exists)
            raise ZstdError("match_finder must be one of %s" % ", ".join(repr(k) for k in self.MATCH_FINDERS))
        self.L = _lib.lib()
        self.ctx = self.L.zhip_ctx_create()
        if not self.ctx:
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())
        self.set_match_finder(match_finder)
        raw = None if dict_data is None else (dict_data.as_bytes() if hasattr(dict_data, "as_bytes") else bytes(dict_data))
        self._dict_buf = C.create_string_buffer(raw, len(raw)) if raw else None          # kept alive: the library fingerprints it per call
        rc = self.L.zhip_ctx_set_dformat(self.ctx, format, max_window_size)
        if rc:
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())
        if raw:
            rc = self.L.zhip_ctx_set_ddict(self.ctx, C.cast(self._dict_buf, C.c_void_p), len(raw), dict_type)
            if rc:
                raise ZstdError("could not load dictionary: %s" % (_lib.error_name(-rc) if rc < 0 else _lib.last_error()))
        p = _lib.CParams()
        p.level, p.contentSizeFlag, p.checksumFlag, p.dictIDFlag = level, int(write_content_size), int(write_checksum), int(write_dict_id)
        p.dictType, p.format = dict_type, format
        names = {"window_log": "windowLog", "chain_log": "chainLog", "hash_log": "hashLog", "search_log": "searchLog",
                 "min_match": "minMatch", "target_length": "targetLength", "strategy": "strategy"}
        for k, v in cparams.items():
            setattr(p.cp, names[k], v)
        if raw:
            p.dict, p.dictSize = C.cast(self._dict_buf, C.c_void_p), len(raw)
        # the compression side is set up by the first compress() call: digesting the dictionary for compression (tagged tables, entropy
        # encoding tables) is work a decode-only context never needs, and a dictionary the compressor refuses must not stop a decoder
        self._cparams, self._cparams_set = p, False

    def _ensure_cparams(self):
        if not self._cparams_set:
            rc = self.L.zhip_ctx_set_cparams(self.ctx, C.byref(self._cparams))
            if rc:
                raise ZstdError("could not set compression parameters: %s" % (_lib.error_name(-rc) if rc < 0 else _lib.last_error()))
            self._cparams_set = True

    def set_size_hint(self, max_item_bytes):
        """largest uncompressed item of the coming calls (0 = unknown): with items above 128 KiB (frames of several blocks) decompression
        runs the phase-split kernels in their several-block mode and compression of large batches gives those sources to the flat match
        kernel; untold, such items are served one wave each by a token grid of the generic kernels (correct, slow)"""
        self.L.zhip_ctx_set_size_hint(self.ctx, int(max_item_bytes))

    MATCH_FINDERS = {"libzstd": 0, "wave": 1, "none": 2, "auto": 4}

    def set_match_finder(self, match_finder):
        """the match finder of the coming compress / seekable_compress / seekable_compress_records calls (compress_sequences has none). "libzstd": the searches
        that keep libzstd's table contents, frames byte for byte libzstd's. "wave": one wave per source with its hash table in LDS -- valid zstd frames that every
        decoder reads, deterministic, NOT libzstd's bytes; sources of one block, no dictionary, levels whose one-block row is fast or double-fast (<= 4, negative),
        anything else raises ZstdError from the compress call or gets status 40 at its own index.
        "none": no match search at all, for NUMERIC TENSORS -- float weights and activations, above all the byte planes of a typed stream
        (seekable_compress(..., element_size=k)). One kernel per chunk reads each source as its block's literals: every frame is byte for byte what libzstd's
        ZSTD_compressSequences writes for an empty sequence list (and what compress_sequences writes for count 0) -- a Huffman, raw or RLE literals section and
        "0 sequences", or a raw block -- at the context's level, parameters and flags. On float tensors such frames are the size of level 3's or up to 13 % smaller
        (the search finds only short, worthless matches there) and no search is paid for. The caveat: "On data with real repetition they lose badly: the int64 sums
        here [1.9 x level 3's size], and any text" -- nothing picks the finder for you. Scope and refusals as for "wave": sources of one block, no dictionary, levels
        whose one-block row is fast or double-fast; a dictionary or level 5 raises ZstdError naming "none" from the compress call, a source of several blocks gets
        status 40 at its own index.
        "auto": "none" or "libzstd", chosen PER SOURCE by a classify kernel from a bounded sample of the source (``classify`` shows its decisions): the planes of one
        typed stream want different finders, and so do the records of a mixed stream. Every frame is byte for byte what "none" or "libzstd" writes for that source,
        with status and size at the source's own index; the choice depends on the source's bytes alone. A source above one block or below 64 bytes goes to the
        search. Unlike the other finders the compress call waits once on its stream (for the two parts' sizes). A dictionary or level 5 raises ZstdError naming
        "auto" from the compress call. Host state only."""
        if match_finder not in self.MATCH_FINDERS:
            raise ZstdError("match_finder must be one of %s" % ", ".join(repr(k) for k in self.MATCH_FINDERS))
        if self.L.zhip_ctx_set_match_finder(self.ctx, self.MATCH_FINDERS[match_finder]):
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())
        self.match_finder = match_finder

    def close(self):
        if getattr(self, "ctx", None):
            self.L.zhip_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _check(t, dtype):
        assert t.is_cuda and t.is_contiguous() and t.dtype == dtype, "expected a contiguous CUDA tensor of %s" % dtype

    def decompress(self, src, src_segs, dst, dst_segs, out_sizes, status, stream=None):
        """Asynchronous. src/dst: uint8 arenas; *_segs: int64 [n,2] (offset,length|capacity); out_sizes int64[n]; status int32[n]."""
        self._check(src, torch.uint8); self._check(dst, torch.uint8)
        self._check(src_segs, torch.int64); self._check(dst_segs, torch.int64)
        self._check(out_sizes, torch.int64); self._check(status, torch.int32)
        n = src_segs.shape[0]
        s = stream if stream is not None else torch.cuda.current_stream()
        rc = self.L.zhip_decompress_batch_device(self.ctx, src.data_ptr(), src_segs.data_ptr(), n, dst.data_ptr(),
                                                 dst_segs.data_ptr(), out_sizes.data_ptr(), status.data_ptr(),
                                                 s.cuda_stream)
        if rc:
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())

    def compress(self, src, src_segs, dst, dst_segs, out_sizes, status, stream=None):
        self._ensure_cparams()
        self._check(src, torch.uint8); self._check(dst, torch.uint8)
        n = src_segs.shape[0]
        s = stream if stream is not None else torch.cuda.current_stream()
        rc = self.L.zhip_compress_batch_device(self.ctx, src.data_ptr(), src_segs.data_ptr(), n, dst.data_ptr(),
                                               dst_segs.data_ptr(), out_sizes.data_ptr(), status.data_ptr(),
                                               s.cuda_stream)
        if rc:
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())

    def classify(self, src, src_segs, stats=False, stream=None):
        """match_finder="auto"'s decision for every source of a batch, without compressing anything: a uint8 CUDA tensor [n], 0 = the search ("libzstd"),
        1 = literals only ("none"); with stats=True also an int32 tensor [n, 4] of the integers it was made from -- sampled window bytes, their order-0 cost and
        the matches' credit in 1/256 bit, sampled positions with a candidate of 4 bytes or more (zeros for a source that was not sampled: above one block, below
        64 bytes). Asynchronous; reads the context's level, finder and dictionary not at all."""
        self._check(src, torch.uint8); self._check(src_segs, torch.int64)
        n = src_segs.shape[0]
        choice = torch.zeros(n, dtype=torch.uint8, device=src.device)
        st = torch.zeros((n, 4), dtype=torch.int32, device=src.device) if stats else None
        s = stream if stream is not None else torch.cuda.current_stream()
        rc = self.L.zhip_classify_batch_device(self.ctx, src.data_ptr(), src_segs.data_ptr(), n, choice.data_ptr(), st.data_ptr() if stats else None, s.cuda_stream)
        if rc:
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())
        return (choice, st) if stats else choice

    def compress_sequences(self, src, src_segs, seqs, seq_segs, dst, dst_segs, out_sizes, status, copy_literals=False, stream=None):
        """compress() from the caller's sequences instead of a match search (an external match finder; tests of the entropy stage). seqs: int64 CUDA tensor of
        packed sequences -- offBase | litLength << 28 | matchLength << 46 --, seq_segs: int64 [n,2] (first, count) per source. Sources of one block. A list the
        loader refuses gets status 107. copy_literals: the loader copies the literals out (the lane-serial match kernel's hand-over) instead of leaving
        the gather to the entropy kernel; the frames are the same."""
        self._ensure_cparams()
        self._check(src, torch.uint8); self._check(dst, torch.uint8); self._check(seqs, torch.int64); self._check(seq_segs, torch.int64)
        n = src_segs.shape[0]
        assert seq_segs.shape[0] == n
        s = stream if stream is not None else torch.cuda.current_stream()
        rc = self.L.zhip_compress_sequences_device(self.ctx, src.data_ptr(), src_segs.data_ptr(), n, seqs.data_ptr(), seq_segs.data_ptr(), dst.data_ptr(),
                                                   dst_segs.data_ptr(), out_sizes.data_ptr(), status.data_ptr(), s.cuda_stream, 1 if copy_literals else 0)
        if rc:
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())

    def entropy_grid(self):
        """waves of the entropy kernel resident on this device"""
        return int(self.L.zhip_ctx_entropy_grid(self.ctx))

    def seekable_compress(self, src, frame_size=131072, checksum=False, stream=None, element_size=1, filter=None, base=None):
        """src (a uint8 CUDA tensor) as ONE zstd seekable stream: frames of frame_size bytes of it, compressed as a batch with this context's
        parameters, back to back, then the seek table (checksum: with the low 32 bits of XXH64 of every frame's content). Returns a uint8 CUDA
        tensor of exactly the stream's size -- a view of a zhip_seekable_bound-sized allocation. Waits for the size. Any zstd decoder decompresses
        the stream whole; SeekableStream reads ranges of it.
        element_size 2, 4 or 8: a TYPED stream -- src holds elements of that many bytes (a tensor's bytes: t.view(torch.uint8)), frame_size counts the ELEMENTS
        of one group, and every group becomes element_size frames, one per byte position of the elements ("byte planes": each gets entropy tables of its own,
        8-20 % smaller streams for bf16 / fp16 / fp32 weights and integer ids). A marker frame behind the last plane makes the stream describe itself:
        SeekableStream reads elements back; other zstd decoders see the planar bytes (zstandard_amd.seekable.planes_to_elements). Takes src.numel() more
        bytes of context memory, kept between calls.
        filter "delta" (typed streams only): for INTEGER tensors whose neighbours are close -- offsets, sorted ids, timestamps, counters, running sums. Per group
        the planes are those of d[0] = x[0], d[i] = x[i] - x[i - 1] mod 2^(8 * element_size), the subtraction fused into the split kernel; 13-34 % smaller
        streams on such data, nothing gained on floats. The marker names the filter: SeekableStream reads the elements back (``SeekableStream.filter``),
        other decoders see the filtered planar bytes (planes_to_elements(..., filter="delta")).
        base (typed streams only; ``base=`` alone selects the filter, whose name is "xor_base"): for VERSIONS of one tensor -- the next checkpoint, a fine-tune
        beside its base model, an optimizer state some steps later. base is a contiguous CUDA tensor of src's size, the earlier version, already in HBM; the
        planes are those of src XOR base, bytewise, fused into the split kernel. Versions differ in the low mantissa bits and almost nowhere else, so the high
        planes become runs of zeros: bf16 streams 2-12 x smaller than the unfiltered typed stream, fp32 1.3-1.8 x (README). THE STREAM DOES NOT NAME ITS BASE:
        SeekableStream(..., base=) reads the elements back, and with another base of the right size it returns wrong elements and no error. Other decoders see
        the filtered planar bytes (planes_to_elements(..., base=)). A base with filter="delta", or "xor_base" without a base, raises ZstdError."""
        self._ensure_cparams()
        self._check(src, torch.uint8)
        s = stream if stream is not None else torch.cuda.current_stream()
        flags = _lib.SEEKABLE_CHECKSUM if checksum else 0
        with_base = _base_filter(filter, base)
        code = 0 if with_base else _filter_code(filter)
        if (code or with_base) and element_size == 1:
            raise ZstdError("seekable compress: a filter needs an element_size of 2, 4 or 8")
        if element_size != 1:
            return self._seekable_compress_typed(src, frame_size, element_size, flags, s, code, base if with_base else None)
        bound = self.L.zhip_seekable_bound(src.numel(), frame_size, flags)
        if not bound:
            raise ZstdError("seekable compress: frame_size must be 1 ... 2^30 and give at most 2^27 frames")
        with torch.cuda.stream(s):
            dst = torch.empty(bound, dtype=torch.uint8, device=src.device)
            size = torch.zeros(1, dtype=torch.int64, device=src.device)
            status = torch.zeros(2, dtype=torch.int32, device=src.device)
        rc = self.L.zhip_seekable_compress_device(self.ctx, src.data_ptr(), src.numel(), frame_size, flags, dst.data_ptr(), bound, size.data_ptr(),
                                                  status.data_ptr(), s.cuda_stream)
        if rc:
            raise ZstdError("seekable compress failed: %s" % _lib.last_error())
        err = _lib.Error()
        rc = self.L.zhip_ctx_sync(self.ctx, s.cuda_stream, status.data_ptr(), 1, C.byref(err))
        if rc == _lib.ERR_ZSTD:
            raise ZstdError("seekable compress: frame %d: %s" % (int(status[1]), _lib.error_name(err.zstdErr)))
        if rc:
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())
        return dst[:int(size[0])]

    def _seekable_compress_typed(self, src, frame_size, element_size, flags, s, filter_code=0, base=None):
        if element_size not in (2, 4, 8):
            raise ZstdError("seekable compress: element_size must be 1, 2, 4 or 8")
        if src.numel() % element_size:
            raise ZstdError("seekable compress: %d bytes are no whole elements of %d" % (src.numel(), element_size))
        bound = self.L.zhip_seekable_typed_bound(src.numel(), frame_size, element_size, flags) if 0 < frame_size <= 1 << 30 else 0
        if not bound:
            raise ZstdError("seekable compress: frame_size must be 1 ... 2^30 elements and give at most 2^27 - 1 plane frames")
        if base is not None:
            base = _base_bytes(base, src, src.numel(), "seekable compress")
        with torch.cuda.stream(s):
            dst = torch.empty(bound, dtype=torch.uint8, device=src.device)
            size = torch.zeros(1, dtype=torch.int64, device=src.device)
            status = torch.zeros(2, dtype=torch.int32, device=src.device)
        if base is not None:
            rc = self.L.zhip_seekable_compress_typed_base_device(self.ctx, src.data_ptr() if src.numel() else None, src.numel(), frame_size, element_size, base.data_ptr(), flags,
                                                                 dst.data_ptr(), bound, size.data_ptr(), status.data_ptr(), s.cuda_stream)
        else:
            rc = self.L.zhip_seekable_compress_typed_filter_device(self.ctx, src.data_ptr() if src.numel() else None, src.numel(), frame_size, element_size, filter_code, flags,
                                                                   dst.data_ptr(), bound, size.data_ptr(), status.data_ptr(), s.cuda_stream)
        if rc:
            raise ZstdError("seekable compress failed: %s" % _lib.last_error())
        err = _lib.Error()
        rc = self.L.zhip_ctx_sync(self.ctx, s.cuda_stream, status.data_ptr(), 1, C.byref(err))
        if rc == _lib.ERR_ZSTD:
            raise ZstdError("seekable compress: plane frame %d: %s" % (int(status[1]), _lib.error_name(err.zstdErr)))
        if rc:
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())
        return dst[:int(size[0])]

    def _planes(self, call, src, frame_size, element_size, out, stream, filter=None, base=None):
        assert src.is_cuda and src.is_contiguous(), "expected a contiguous CUDA tensor"
        raw = src.view(torch.uint8).reshape(-1)
        with_base = _base_filter(filter, base)
        if with_base:
            base = _base_bytes(base, src, raw.numel(), "planes")
        s = stream if stream is not None else torch.cuda.current_stream()
        if out is None:
            with torch.cuda.stream(s):
                out = torch.empty(raw.numel(), dtype=torch.uint8, device=src.device)
        self._check(out, torch.uint8)
        assert out.numel() >= raw.numel(), "out is shorter than the source"
        if with_base:
            call = self.L.zhip_planes_split_base_device if call is self.L.zhip_planes_split_filter_device else self.L.zhip_planes_join_base_device
            rc = call(self.ctx, raw.data_ptr() if raw.numel() else None, raw.numel(), element_size, frame_size, base.data_ptr(), out.data_ptr() if raw.numel() else None, s.cuda_stream)
        else:
            rc = call(self.ctx, raw.data_ptr() if raw.numel() else None, raw.numel(), element_size, frame_size, _filter_code(filter), out.data_ptr() if raw.numel() else None, s.cuda_stream)
        if rc:
            raise ZstdError("planes: %s" % _lib.last_error())
        return out[:raw.numel()]

    def planes_split(self, src, frame_size, element_size=None, out=None, stream=None, filter=None, base=None):
        """the bytes of src (any contiguous CUDA tensor; element_size None: its dtype's) in the PLANAR order of a typed seekable stream, as a uint8 tensor: groups
        of frame_size elements, group g's plane p -- byte p of every element -- at g * element_size * frame_size + p * (the group's elements). filter "delta": the planes of the
        group's differences (seekable_compress), subtracted in the same kernel. base (a contiguous CUDA tensor of src's size; selects filter "xor_base"): the
        planes of src XOR base, in one kernel; base and out must not overlap. Asynchronous."""
        return self._planes(self.L.zhip_planes_split_filter_device, src, frame_size, src.element_size() if element_size is None else element_size, out, stream, filter, base)

    def planes_join(self, planar, frame_size, element_size, out=None, stream=None, filter=None, base=None):
        """planes_split's inverse under the same filter: planar bytes -> the elements' bytes, as a uint8 tensor (view it as the dtype). Under "delta" the
        prefix sum of every group, three launches and 8 bytes of context memory per 1 024 elements. With base (the tensor the split was given -- another one
        gives wrong elements, no error): the joined bytes XOR base, in one kernel. Asynchronous."""
        return self._planes(self.L.zhip_planes_join_filter_device, planar, frame_size, element_size, out, stream, filter, base)

    def planes_join_chain(self, planars, frame_size, element_size, out=None, stream=None, base=None):
        """1 ... 16 planar buffers of ONE layout (planes_split's, the same size, frame_size and element_size) -> the elements' bytes of their bytewise XOR,
        XORed with base where one is given, as a uint8 tensor: what a chain of versions stored against their predecessors reads back as (SeekableChain), in
        one kernel -- the planar words are XORed and transposed once. base and out must not overlap. Asynchronous."""
        planars = list(planars)
        if not 1 <= len(planars) <= 16:
            raise ZstdError("planes join chain: a chain has 1 ... 16 links, not %d" % len(planars))
        raws = []
        for i, p in enumerate(planars):
            if not (isinstance(p, torch.Tensor) and p.is_cuda and p.is_contiguous() and p.device == planars[0].device):
                raise ZstdError("planes join chain: link %d is no contiguous CUDA tensor on link 0's device" % i)
            raws.append(p.view(torch.uint8).reshape(-1))
            if raws[i].numel() != raws[0].numel():
                raise ZstdError("planes join chain: link %d has %d bytes, link 0 %d" % (i, raws[i].numel(), raws[0].numel()))
        nbytes = raws[0].numel()
        if base is not None:
            base = _base_bytes(base, planars[0], nbytes, "planes join chain")
        s = stream if stream is not None else torch.cuda.current_stream()
        if out is None:
            with torch.cuda.stream(s):
                out = torch.empty(nbytes, dtype=torch.uint8, device=planars[0].device)
        self._check(out, torch.uint8)
        assert out.numel() >= nbytes, "out is shorter than the planar buffers"
        ptrs = (C.c_void_p * len(raws))(*[r.data_ptr() if nbytes else None for r in raws])
        rc = self.L.zhip_planes_join_chain_device(self.ctx, ptrs, len(raws), nbytes, element_size, frame_size, base.data_ptr() if base is not None and nbytes else None,
                                                  out.data_ptr() if nbytes else None, s.cuda_stream)
        if rc:
            raise ZstdError("planes: %s" % _lib.last_error())
        return out[:nbytes]

    def _records_table(self, src, records, max_content_bytes, max_record_bytes, s, what="seekable compress"):
        """records as seekable_compress_records takes them -> (the (n, 2) int64 CUDA table, n, max_content_bytes, max_record_bytes)"""
        import numpy as np
        if isinstance(records, torch.Tensor) and records.is_cuda:
            if max_content_bytes is None or max_record_bytes is None:
                raise ZstdError("%s: a device-resident record table needs max_content_bytes and max_record_bytes" % what)
            self._check(records, torch.int64)
            if records.dim() != 2 or records.shape[1] != 2:
                raise ZstdError("%s: records must have the shape (n, 2)" % what)
            table = records
        else:
            try:
                r = np.asarray(records.cpu() if isinstance(records, torch.Tensor) else records if len(records) else np.zeros((0, 2), dtype=np.int64))
            except Exception:
                raise ZstdError("%s: records must be a sequence of (offset, length)" % what)
            if r.ndim != 2 or r.shape[1] != 2 or r.dtype.kind not in "iu":
                raise ZstdError("%s: records must be a sequence of (offset, length) or an integer array of shape (n, 2)" % what)
            if r.shape[0] and ((r.astype(object) < 0).any() or (r.astype(object) >= 1 << 63).any()):
                raise ZstdError("%s: records must not be negative" % what)
            r = np.ascontiguousarray(r.astype(np.int64))
            if max_content_bytes is None:
                max_content_bytes = int(r[:, 1].sum()) if r.shape[0] else 0
            if max_record_bytes is None:
                max_record_bytes = int(r[:, 1].max()) if r.shape[0] else 0
            with torch.cuda.stream(s):
                table = torch.from_numpy(r).to(src.device) if r.shape[0] else torch.zeros((0, 2), dtype=torch.int64, device=src.device)
        n = int(table.shape[0])
        max_content_bytes, max_record_bytes = int(max_content_bytes), int(max_record_bytes)
        if max_content_bytes < 0 or not 0 <= max_record_bytes <= 1 << 30 or n > 1 << 27:
            raise ZstdError("%s: at most 2^27 records of at most 2^30 bytes" % what)
        return table, n, max_content_bytes, max_record_bytes

    def seekable_compress_records(self, src, records, max_content_bytes=None, max_record_bytes=None, checksum=False, stream=None):
        """One frame per record: records[i] = (offset, length) of record i in src (a uint8 CUDA tensor), anywhere in it, in any order, with gaps or sharing
        bytes, length 0 allowed; the stream's content is the records concatenated in index order. records: an (n, 2) int64 CUDA tensor -- it may have been
        written by work queued on `stream`, nothing is waited for; max_content_bytes (an upper bound on the lengths' sum) and max_record_bytes (on every
        length, at most 2^30) are then required, and the device checks them -- or a host sequence / array of (offset, length), which is uploaded and gives both
        bounds itself. Returns a uint8 CUDA tensor of exactly the stream's size, as seekable_compress does. Waits for the size. A record outside src or above
        a bound raises ZstdError (srcSize_wrong) with its index. SeekableStream.read_records reads records back by index."""
        self._ensure_cparams()
        self._check(src, torch.uint8)
        s = stream if stream is not None else torch.cuda.current_stream()
        table, n, max_content_bytes, max_record_bytes = self._records_table(src, records, max_content_bytes, max_record_bytes, s)
        flags = _lib.SEEKABLE_CHECKSUM if checksum else 0
        bound = self.L.zhip_seekable_records_bound(min(max_content_bytes, n * max_record_bytes), n, flags)
        if not bound:
            raise ZstdError("seekable compress: at most 2^27 records of at most 2^30 bytes")
        with torch.cuda.stream(s):
            dst = torch.empty(bound, dtype=torch.uint8, device=src.device)
            size = torch.zeros(1, dtype=torch.int64, device=src.device)
            status = torch.zeros(2, dtype=torch.int32, device=src.device)
        rc = self.L.zhip_seekable_compress_records_device(self.ctx, src.data_ptr(), src.numel(), table.data_ptr() if n else None, n, max_content_bytes, max_record_bytes,
                                                          flags, dst.data_ptr(), bound, size.data_ptr(), status.data_ptr(), s.cuda_stream)
        if rc:
            raise ZstdError("seekable compress failed: %s" % _lib.last_error())
        err = _lib.Error()
        rc = self.L.zhip_ctx_sync(self.ctx, s.cuda_stream, status.data_ptr(), 1, C.byref(err))
        if rc == _lib.ERR_ZSTD:
            raise ZstdError("seekable compress: record %d: %s" % (int(status[1]), _lib.error_name(err.zstdErr)))
        if rc:
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())
        return dst[:int(size[0])]

    def _edit(self, old, picks, src, records, max_content_bytes, max_record_bytes, checksum, out, stream):
        """zhip_seekable_edit_device behind seekable_edit (old None) and SeekableStream.edit (old: the opened stream) -> out[:size], or a view of a new tensor
        sized by zhip_seekable_edit_bound"""
        import numpy as np
        try:
            p = np.asarray(picks if len(picks) else np.zeros((0, 2), dtype=np.int64))
        except Exception:
            raise ZstdError("seekable edit: picks must be a sequence of (0 | 1, index)")
        if p.ndim != 2 or p.shape[1] != 2 or p.dtype.kind not in "iu":
            raise ZstdError("seekable edit: picks must be a sequence of (0 | 1, index) or an integer array of shape (k, 2)")
        k = p.shape[0]
        if k > 1 << 27:
            raise ZstdError("seekable edit: at most 2^27 picks")
        s = stream if stream is not None else torch.cuda.current_stream()
        if records is None:
            table, n, max_content_bytes, max_record_bytes = None, 0, 0, 0
        else:
            if src is None:
                raise ZstdError("seekable edit: records need src")
            self._ensure_cparams()
            self._check(src, torch.uint8)
            table, n, max_content_bytes, max_record_bytes = self._records_table(src, records, max_content_bytes, max_record_bytes, s, "seekable edit")
        n_frames = old.n_frames if old is not None else 0
        if k:
            if (p < 0).any():
                raise ZstdError("seekable edit: position %d is negative" % int(np.nonzero((p < 0).any(axis=1))[0][0]))
            kind, index = p[:, 0].astype(np.uint64), p[:, 1].astype(np.uint64)
            wrong = np.nonzero((kind != _lib.PICK_FRAME) & (kind != _lib.PICK_RECORD))[0]
            if len(wrong):
                raise ZstdError("seekable edit: position %d is neither a frame (0) nor a record (1) pick" % int(wrong[0]))
            if old is None and (kind == _lib.PICK_FRAME).any():
                raise ZstdError("seekable edit: position %d picks a frame, and no stream is opened" % int(np.nonzero(kind == _lib.PICK_FRAME)[0][0]))
            wrong = np.nonzero(index >= np.where(kind == _lib.PICK_FRAME, np.uint64(n_frames), np.uint64(n)))[0]
            if len(wrong):
                w = int(wrong[0])
                raise ZstdError("seekable edit: position %d names %s %d, there are %d" % ((w, "frame", int(index[w]), n_frames) if kind[w] == _lib.PICK_FRAME
                                                                                          else (w, "record", int(index[w]), n)))
        pk = np.ascontiguousarray(p.astype(np.uint32)) if k else np.zeros((1, 2), dtype=np.uint32)
        device = old.tensor.device if old is not None else src.device if src is not None else torch.device("cuda", torch.cuda.current_device())
        flags = _lib.SEEKABLE_CHECKSUM if checksum else 0
        handle = old.handle if old is not None else None
        bound = self.L.zhip_seekable_edit_bound(handle, pk.ctypes.data, k, max_record_bytes, flags)
        if not bound:
            raise ZstdError("seekable edit: bad arguments")
        with torch.cuda.stream(s):
            if out is None:
                out = torch.empty(bound, dtype=torch.uint8, device=device)
            size = torch.zeros(1, dtype=torch.int64, device=device)
            status = torch.zeros(2, dtype=torch.int32, device=device)
        self._check(out, torch.uint8)
        rc = self.L.zhip_seekable_edit_device(self.ctx, handle, pk.ctypes.data, k, src.data_ptr() if n else None, src.numel() if n else 0, table.data_ptr() if n else None, n,
                                              max_content_bytes, max_record_bytes, flags, out.data_ptr(), out.numel(), size.data_ptr(), status.data_ptr(), s.cuda_stream)
        if rc:
            raise ZstdError("seekable edit failed: %s" % _lib.last_error())
        err = _lib.Error()
        rc = self.L.zhip_ctx_sync(self.ctx, s.cuda_stream, status.data_ptr(), 1, C.byref(err))
        if rc == _lib.ERR_ZSTD:
            code, index = (int(x) for x in status)
            raise ZstdError("seekable edit: %s %d: %s" % ("record" if code == 72 else "position", index, _lib.error_name(err.zstdErr)))
        if rc:
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())
        return out[:int(size[0])]

    def seekable_edit(self, picks, src=None, records=None, max_content_bytes=None, max_record_bytes=None, checksum=False, out=None, stream=None):
        """SeekableStream.edit without an opened stream: every pick is (1, record index). With picks (1, 0) .. (1, n - 1) the result is
        seekable_compress_records' byte for byte; a record may be picked any number of times or not at all."""
        return self._edit(None, picks, src, records, max_content_bytes, max_record_bytes, checksum, out, stream)

    def kernel_time(self, direction):
        """(average ms per launch, launches) of the dominant kernel since the last call, from HIP events on the launch stream."""
        ms, n = C.c_double(0), C.c_uint64(0)
        self.L.zhip_ctx_kernel_time(self.ctx, direction, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def decode_fallbacks(self):
        """frames of the last decompress() call that the phase-split kernels handed to the generic kernel (waits for the device)"""
        n = C.c_uint64(0)
        if self.L.zhip_ctx_decode_fallbacks(self.ctx, C.byref(n)):
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())
        return n.value

    def table_pick(self):
        """(candidate times in ms -- 0 = not tried --, index kept) of the compress direction's table placement pick; zeros while none has happened"""
        ms = (C.c_float * 3)()
        kept = self.L.zhip_ctx_table_pick(self.ctx, ms)
        return [float(x) for x in ms], int(kept)

    def kernel_name(self, direction):
        return self.L.zhip_kernel_name(direction).decode()


def planes_split(src, frame_size, element_size=None, ctx=None, out=None, stream=None, filter=None, base=None):
    """DeviceBatchContext.planes_split on `ctx`, or on a context of its own (then it waits)"""
    if ctx is not None:
        return ctx.planes_split(src, frame_size, element_size, out, stream, filter, base)
    with_ctx = DeviceBatchContext()
    try:
        return with_ctx.planes_split(src, frame_size, element_size, out, stream, filter, base)
    finally:
        with_ctx.close()


def planes_join(planar, frame_size, element_size, ctx=None, out=None, stream=None, filter=None, base=None):
    """DeviceBatchContext.planes_join on `ctx`, or on a context of its own (then it waits)"""
    if ctx is not None:
        return ctx.planes_join(planar, frame_size, element_size, out, stream, filter, base)
    with_ctx = DeviceBatchContext()
    try:
        return with_ctx.planes_join(planar, frame_size, element_size, out, stream, filter, base)
    finally:
        with_ctx.close()


def planes_join_chain(planars, frame_size, element_size, ctx=None, out=None, stream=None, base=None):
    """DeviceBatchContext.planes_join_chain on `ctx`, or on a context of its own (then it waits)"""
    if ctx is not None:
        return ctx.planes_join_chain(planars, frame_size, element_size, out, stream, base)
    with_ctx = DeviceBatchContext()
    try:
        return with_ctx.planes_join_chain(planars, frame_size, element_size, out, stream, base)
    finally:
        with_ctx.close()


def _ranges_table(ranges, out, out_offsets):
    """the (offset, length) ranges of a read_ranges call -> (the [R][3] table the library takes, R, the lengths, the bytes `out` needs)"""
    import numpy as np
    try:
        r = np.asarray(ranges if len(ranges) else np.zeros((0, 2), dtype=np.int64))
    except Exception:
        raise ZstdError("ranges must be a sequence of (offset, length)")
    if r.ndim != 2 or r.shape[1] != 2 or r.dtype.kind not in "iu":
        raise ZstdError("ranges must be a sequence of (offset, length) or an integer array of shape (R, 2)")
    n = r.shape[0]
    if n and (r.astype(object) < 0).any():
        raise ZstdError("ranges must not be negative")
    table = np.zeros((max(n, 1), 3), dtype=np.uint64)
    table[:n, :2] = r
    lengths = [int(x) for x in table[:n, 1]]
    if out_offsets is None:
        at = 0
        for k, ln in enumerate(lengths):
            table[k, 2] = at; at += ln
        need = at
    else:
        if out is None:
            raise ZstdError("out_offsets needs out")
        offs = [int(x) for x in out_offsets]
        if len(offs) != n or any(x < 0 for x in offs):
            raise ZstdError("out_offsets must hold one non-negative offset per range")
        table[:n, 2] = np.array(offs, dtype=np.uint64) if n else 0
        need = max([o + ln for o, ln in zip(offs, lengths)] + [0])
    return table, n, lengths, need


class SeekableStream:
    """Range reads of a zstd seekable stream resident in HBM (any writer's): ``read(offset, length)`` decodes only the frames that cover the range,
    ``read_ranges`` many ranges as one decode batch, ``read_records`` whole frames by index; ``frame_offsets`` is the table it opened.

    A TYPED stream (DeviceBatchContext.seekable_compress with element_size 2, 4 or 8) is recognised by its marker: ``element_size`` and ``group_elements``
    say so (1 and 0 for a plain stream), ``filter`` is None or "delta" (seekable_compress's), and ``read`` / ``read_ranges`` return ELEMENTS whatever the
    filter -- offsets and lengths count the tensor's bytes; under "delta" a group read in part is summed from its first element. ``read_records`` and
    ``frame_offsets`` stay raw: they name the plane frames. The edit family raises ValueError on a typed stream (moving plane frames breaks the groups).
    ``raw=True`` opens a typed stream as the plain stream it also is: every call then sees its planar content -- under a filter the filtered one --, the edit family included.
    A stream written with ``seekable_compress(..., base=)`` has ``filter == "xor_base"``: ``read`` / ``read_ranges`` return elements when ``base=`` -- the
    tensor it was compressed against, kept alive and unchanged while this object is open -- was given, and raise ZstdError when not (``raw=True`` needs none).
    THE STREAM DOES NOT NAME ITS BASE: with another tensor of the right size the reads return wrong elements and no error. Only the base's bytes at the
    offsets a read covers are read; the base must not overlap a read's `out`.

    ctx: the DeviceBatchContext that decodes (its dictionary, format and window limit apply); stream_tensor: the whole stream, a uint8 CUDA tensor,
    kept alive and unchanged while this object is open. Opening reads and checks the seek table (it waits); a damaged table raises ZstdError."""

    def __init__(self, ctx, stream_tensor, stream=None, scratch_limit=None, raw=False, base=None):
        """scratch_limit: see set_scratch_limit; raw, base: see the class"""
        DeviceBatchContext._check(stream_tensor, torch.uint8)
        self.ctx, self.tensor, self.handle = ctx, stream_tensor, None
        s = stream if stream is not None else torch.cuda.current_stream()
        h, info, err = C.c_void_p(), _lib.SeekableInfo(), _lib.Error()
        rc = ctx.L.zhip_seekable_open_device(ctx.ctx, stream_tensor.data_ptr(), stream_tensor.numel(), s.cuda_stream, C.byref(h), C.byref(info), C.byref(err))
        if rc == _lib.ERR_ZSTD:
            raise ZstdError("not a seekable stream: %s" % _lib.error_name(err.zstdErr))
        if rc:
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())
        self.handle = h
        self.content_size, self.n_frames, self.has_checksums = int(info.contentSize), int(info.nFrames), bool(info.checksumFlag)
        self.max_frame_content = int(info.maxFrameContent)
        typed = not raw and ctx.L.zhip_seekable_element_size(h) != 1
        self.element_size = int(ctx.L.zhip_seekable_element_size(h)) if typed else 1
        self.group_elements = int(ctx.L.zhip_seekable_group_elements(h)) if typed else 0
        self.filter = {1: "delta", 4: "xor_base"}.get(int(ctx.L.zhip_seekable_filter(h))) if typed else None
        self.base = None
        if base is not None and self.filter == "xor_base":
            try:
                self.base = _base_bytes(base, stream_tensor, self.content_size, "seekable stream")
            except ZstdError:
                self.close()
                raise
        elif base is not None and not raw:
            self.close()
            raise ZstdError("seekable stream: base= goes with a stream written against a base (filter \"xor_base\"), this one's filter is %r" % (self.filter,))
        self.last_gather_stats = None
        self._frame_offsets = None
        if scratch_limit is not None:
            self.set_scratch_limit(scratch_limit)

    def set_scratch_limit(self, nbytes):
        """most device memory read_ranges may hold frames in that do not decode straight into their place (0: the default, 1 GiB). A call that needs more
        runs in several passes; one frame larger than the limit is still held whole. On a typed stream it also bounds the planar buffer the elements are
        put together from: ranges are taken in passes and cut at group boundaries, one group above the limit is still held whole."""
        if self.handle is None:
            raise ZstdError("the seekable stream is closed")
        if nbytes < 0:
            raise ZstdError("scratch_limit must not be negative")
        self.ctx.L.zhip_seekable_set_scratch_limit(self.handle, int(nbytes))

    def read(self, offset=0, length=None, out=None, stream=None):
        """content bytes [offset, offset + length) (length None: to the end) as a uint8 CUDA tensor -- `out`, where given, else a new one. Waits for the
        result's status; a frame that fails (corrupt, wrong size, wrong checksum) raises ZstdError with its index in the table."""
        if self.handle is None:
            raise ZstdError("the seekable stream is closed")
        if length is None:
            length = self.content_size - offset
        if offset < 0 or length < 0 or offset + length > self.content_size:
            raise ZstdError("range %d + %d is outside the content (%d bytes)" % (offset, length, self.content_size))
        if self.element_size != 1:                                          # the one-range case of the typed call
            if out is not None:
                assert out.numel() >= length, "out is shorter than the range"
            return self.read_ranges([(offset, length)], out, None if out is None else [0], stream)[0]
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            if out is None:
                out = torch.empty(length, dtype=torch.uint8, device=self.tensor.device)
            status = torch.zeros(2, dtype=torch.int32, device=self.tensor.device)
        DeviceBatchContext._check(out, torch.uint8)
        assert out.numel() >= length, "out is shorter than the range"
        L = self.ctx.L
        rc = L.zhip_seekable_decompress_device(self.ctx.ctx, self.handle, offset, length, out.data_ptr(), status.data_ptr(), s.cuda_stream)
        if rc:
            raise ZstdError("seekable read failed: %s" % _lib.last_error())
        err = _lib.Error()
        rc = L.zhip_ctx_sync(self.ctx.ctx, s.cuda_stream, status.data_ptr(), 1, C.byref(err))
        if rc == _lib.ERR_ZSTD:
            raise ZstdError("seekable read: frame %d: %s" % (int(status[1]), _lib.error_name(err.zstdErr)))
        if rc:
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())
        return out[:length]

    def read_ranges(self, ranges, out=None, out_offsets=None, stream=None):
        """Many ranges as ONE decode batch: every frame a range touches is decoded once, whatever the ranges share. ranges: a sequence of (offset, length) or
        an integer array of shape (R, 2). Without `out` a new uint8 CUDA tensor holds the ranges back to back in call order; with `out`, range r goes to
        out[out_offsets[r]:] (out_offsets None: back to back) -- the destinations must not overlap. Returns a list of views, one per range. Waits for the
        status; a frame that fails raises ZstdError naming the lowest range that needs it, the frame and the error. last_gather_stats holds the call's
        counts (items, inPlace, scratchBytes, copyJobs, passes)."""
        if self.handle is None:
            raise ZstdError("the seekable stream is closed")
        table, n, lengths, need = _ranges_table(ranges, out, out_offsets)
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            if out is None:
                out = torch.empty(need, dtype=torch.uint8, device=self.tensor.device)
            status = torch.zeros(2 + 2 * n, dtype=torch.int32, device=self.tensor.device)
        DeviceBatchContext._check(out, torch.uint8)
        L = self.ctx.L
        stats = _lib.SeekableGatherStats()
        if self.filter == "xor_base":
            if self.base is None:
                raise ZstdError("seekable read: the stream was written against a base (filter \"xor_base\") -- open it with base= to read elements, or raw=True for its planar bytes")
            rc = L.zhip_seekable_decompress_typed_ranges_base_device(self.ctx.ctx, self.handle, self.base.data_ptr(), self.base.numel(), table.ctypes.data, n, out.data_ptr(), out.numel(),
                                                                     status.data_ptr(), C.byref(stats), s.cuda_stream)
        else:
            call = L.zhip_seekable_decompress_ranges_device if self.element_size == 1 else L.zhip_seekable_decompress_typed_ranges_device
            rc = call(self.ctx.ctx, self.handle, table.ctypes.data, n, out.data_ptr(), out.numel(), status.data_ptr(), C.byref(stats), s.cuda_stream)
        if rc:
            raise ZstdError("seekable read failed: %s" % _lib.last_error())
        self.last_gather_stats = {k: int(getattr(stats, k)) for k, _ in stats._fields_}
        err = _lib.Error()
        rc = L.zhip_ctx_sync(self.ctx.ctx, s.cuda_stream, status.data_ptr(), 1, C.byref(err))
        if rc == _lib.ERR_ZSTD:
            bad = int(status[1])
            raise ZstdError("seekable read: range %d: frame %d: %s" % (bad, int(status[3 + 2 * bad]), _lib.error_name(err.zstdErr)))
        if rc:
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())
        return [out[int(table[k, 2]):int(table[k, 2]) + lengths[k]] for k in range(n)]

    def frame_offsets(self):
        """the table this object opened: a numpy uint64 array of n_frames + 1 decompressed offsets -- frame (record) f is content bytes [a[f], a[f + 1])"""
        if self.handle is None:
            raise ZstdError("the seekable stream is closed")
        import numpy as np
        if self._frame_offsets is None:
            a = np.zeros(self.n_frames + 1, dtype=np.uint64)
            if self.ctx.L.zhip_seekable_frame_offsets(self.handle, 0, self.n_frames, a.ctypes.data):
                raise ZstdError("seekable read failed: %s" % _lib.last_error())
            self._frame_offsets = a
        return self._frame_offsets.copy()

    def read_records(self, indices, out=None, out_offsets=None, stream=None):
        """Whole frames by index -- the records of a stream written by seekable_compress_records -- as ONE decode batch: every distinct frame is decoded once,
        a frame named once straight into its place. indices: a sequence of frame indices, in any order, repeats allowed. Without `out` a new uint8 CUDA tensor
        holds the records back to back in call order; with `out`, record k goes to out[out_offsets[k]:] (out_offsets None: back to back) -- the destinations
        must not overlap. Returns a list of views, one per index. Waits for the status; a frame that fails raises ZstdError naming the lowest position that
        names it, the frame and the error. last_gather_stats holds the call's counts, as after read_ranges."""
        if self.handle is None:
            raise ZstdError("the seekable stream is closed")
        import numpy as np
        try:
            idx = np.asarray(indices if len(indices) else np.zeros(0, dtype=np.int64))
        except Exception:
            raise ZstdError("indices must be a sequence of frame indices")
        if idx.ndim != 1 or idx.dtype.kind not in "iu":
            raise ZstdError("indices must be a sequence of frame indices")
        n = idx.shape[0]
        wrong = np.nonzero((idx < 0) | (idx >= self.n_frames))[0]
        if len(wrong):
            raise ZstdError("seekable read: position %d names frame %d, the table has %d" % (int(wrong[0]), int(idx[wrong[0]]), self.n_frames))
        idx32 = np.ascontiguousarray(idx.astype(np.uint32)) if n else np.zeros(1, dtype=np.uint32)
        if self._frame_offsets is None:
            self.frame_offsets()
        d = self._frame_offsets
        lengths = (d[idx32[:n].astype(np.int64) + 1] - d[idx32[:n].astype(np.int64)]).tolist()
        if out_offsets is None:
            offs, at = [], 0
            for ln in lengths:
                offs.append(at); at += ln
            need = at
        else:
            if out is None:
                raise ZstdError("out_offsets needs out")
            offs = [int(x) for x in out_offsets]
            if len(offs) != n or any(x < 0 for x in offs):
                raise ZstdError("out_offsets must hold one non-negative offset per index")
            need = max([o + ln for o, ln in zip(offs, lengths)] + [0])
        offs64 = np.array(offs, dtype=np.uint64) if n else np.zeros(1, dtype=np.uint64)
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            if out is None:
                out = torch.empty(need, dtype=torch.uint8, device=self.tensor.device)
            status = torch.zeros(2 + 2 * n, dtype=torch.int32, device=self.tensor.device)
        DeviceBatchContext._check(out, torch.uint8)
        L = self.ctx.L
        stats = _lib.SeekableGatherStats()
        rc = L.zhip_seekable_decompress_frames_device(self.ctx.ctx, self.handle, idx32.ctypes.data, n, offs64.ctypes.data, out.data_ptr(), out.numel(), status.data_ptr(),
                                                      C.byref(stats), s.cuda_stream)
        if rc:
            raise ZstdError("seekable read failed: %s" % _lib.last_error())
        self.last_gather_stats = {k: int(getattr(stats, k)) for k, _ in stats._fields_}
        err = _lib.Error()
        rc = L.zhip_ctx_sync(self.ctx.ctx, s.cuda_stream, status.data_ptr(), 1, C.byref(err))
        if rc == _lib.ERR_ZSTD:
            bad = int(status[1])
            raise ZstdError("seekable read: position %d: frame %d: %s" % (bad, int(status[3 + 2 * bad]), _lib.error_name(err.zstdErr)))
        if rc:
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())
        return [out[offs[k]:offs[k] + lengths[k]] for k in range(n)]

    def edit(self, picks, src=None, records=None, max_content_bytes=None, max_record_bytes=None, out=None, stream=None):
        """A NEW stream out of this stream's frames and of new records, without recompressing what is kept: picks, an integer array of shape (k, 2), names the
        new stream's frames in order -- (0, i): frame i of this stream, its bytes and its table entry as they are; (1, j): record j of `records`, compressed by
        this call with the context's level, parameters, dictionary and match finder. A frame or a record may be picked any number of times; a record nobody
        picks is dropped. records / src / max_content_bytes / max_record_bytes: as in DeviceBatchContext.seekable_compress_records (an (n, 2) int64 CUDA tensor
        may have been written by work queued on `stream` and needs both bounds). The new table has checksums exactly when this stream's has. Returns a uint8
        CUDA tensor of exactly the new stream's size: out[:size] -- `out` must not overlap this stream's tensor --, or a view of a new tensor sized by the bound.
        Waits for the status only; ZstdError names the record (a record outside src or above a bound) or the position in picks (a record the level refuses, a
        frame that ends beyond `out`)."""
        if self.handle is None:
            raise ZstdError("the seekable stream is closed")
        self._plain_only("edit")
        return self.ctx._edit(self, picks, src, records, max_content_bytes, max_record_bytes, self.has_checksums, out, stream)

    def _plain_only(self, what):
        if self.element_size != 1:
            raise ValueError("seekable %s: a typed stream's frames are byte planes in groups of %d -- moving them breaks the groups (open it with raw=True to edit its "
                             "planar form)" % (what, self.element_size))

    @staticmethod
    def _count(records):
        return int(records.shape[0]) if hasattr(records, "shape") else len(records)

    def _picks(self, frames, n_records=0):
        import numpy as np
        p = np.zeros((len(frames) + n_records, 2), dtype=np.int64)
        p[:len(frames), 1] = frames
        p[len(frames):, 0] = _lib.PICK_RECORD
        p[len(frames):, 1] = np.arange(n_records)
        return p

    def append_records(self, src, records, buffer=None, max_content_bytes=None, max_record_bytes=None, stream=None):
        """this stream's frames, then one new frame per record: edit() with picks (0, 0) .. (0, n_frames - 1), (1, 0) .. (1, n - 1). With `buffer` -- a uint8 CUDA
        tensor that starts where this stream's tensor starts (the same data_ptr()) and has room for the bound -- the append is IN PLACE: the kept frames are
        neither read nor written, the new frames start where the old table started; this object is closed (it describes bytes that no longer exist) and
        buffer[:new size] is returned: open it again to read. A failed append in place leaves the old stream as it was, and this object open."""
        import numpy as np
        self._plain_only("append")
        picks = self._picks(np.arange(self.n_frames), self._count(records))
        if buffer is None:
            return self.edit(picks, src, records, max_content_bytes, max_record_bytes, None, stream)
        DeviceBatchContext._check(buffer, torch.uint8)
        if buffer.data_ptr() != self.tensor.data_ptr():
            raise ZstdError("seekable append: buffer must start where the stream's tensor starts")
        out = self.edit(picks, src, records, max_content_bytes, max_record_bytes, buffer, stream)
        self.close()
        return out

    def replace_records(self, indices, src, records, max_content_bytes=None, max_record_bytes=None, stream=None):
        """frame indices[j] gives way to record j of `records` (an index named twice keeps the later record); every other frame is kept"""
        import numpy as np
        self._plain_only("replace")
        idx = np.asarray(indices if len(indices) else np.zeros(0, dtype=np.int64))
        if idx.ndim != 1 or idx.dtype.kind not in "iu" or len(idx) != self._count(records):
            raise ZstdError("seekable replace: one frame index per record")
        wrong = np.nonzero((idx < 0) | (idx >= self.n_frames))[0]
        if len(wrong):
            raise ZstdError("seekable replace: position %d names frame %d, the table has %d" % (int(wrong[0]), int(idx[wrong[0]]), self.n_frames))
        picks = self._picks(np.arange(self.n_frames))
        picks[idx, 0] = _lib.PICK_RECORD
        picks[idx, 1] = np.arange(len(idx))
        return self.edit(picks, src, records, max_content_bytes, max_record_bytes, None, stream)

    def delete_records(self, indices, stream=None):
        """the stream without the frames named by `indices`"""
        import numpy as np
        self._plain_only("delete")
        idx = np.asarray(indices if len(indices) else np.zeros(0, dtype=np.int64))
        if idx.ndim != 1 or idx.dtype.kind not in "iu":
            raise ZstdError("seekable delete: indices must be a sequence of frame indices")
        wrong = np.nonzero((idx < 0) | (idx >= self.n_frames))[0]
        if len(wrong):
            raise ZstdError("seekable delete: position %d names frame %d, the table has %d" % (int(wrong[0]), int(idx[wrong[0]]), self.n_frames))
        keep = np.ones(self.n_frames, dtype=bool)
        keep[idx] = False
        return self.edit(self._picks(np.nonzero(keep)[0]), stream=stream)

    def reorder(self, order, stream=None):
        """the frames named by `order`, in that order -- a permutation lays an epoch's sample order out contiguously; `order` may repeat or omit frames"""
        import numpy as np
        self._plain_only("reorder")
        return self.edit(self._picks(np.asarray(order if len(order) else np.zeros(0, dtype=np.int64))), stream=stream)

    def close(self):
        if self.handle is not None:
            self.ctx.L.zhip_seekable_close(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SeekableChain:
    """Reads of version n of a tensor through a CHAIN of typed seekable streams, each version written against its PREDECESSOR
    (``seekable_compress(v[i], element_size=k, base=v[i - 1])``): ``links`` are ``[full, d1, ..., dn]`` -- v0 as an unfiltered typed stream, then the deltas,
    oldest first -- or ``[d1, ..., dn]`` with ``base=v0``, 1 ... 16 of them, stream tensors (opened here, closed by ``close``) or open SeekableStreams (the
    caller's; they stay usable on their own between the chain's calls). ``read`` / ``read_ranges`` have SeekableStream's semantics and return types and
    give the elements of the LAST version: per link only the frames the ranges touch are decoded, and ONE kernel XORs all links' planes, transposes once and
    XORs the base -- no version in between is materialised. A frame that fails raises ZstdError naming the range, the link and the frame in that link's
    table; where several links fail under a range, the earliest link. ``last_gather_stats`` sums over the links, ``passes`` counted once.

    NO LINK NAMES ITS BASE OR ITS PREDECESSOR: links in the wrong order behind a wrong start, a link of another tensor, or another base return wrong
    elements and no error. Device memory: every link holds at most the scratch limit (see set_scratch_limit) of planar bytes, the chain that many times
    its links. The base, the streams and the open links stay alive and unchanged while the chain is open; the base must not overlap a read's `out`."""

    def __init__(self, ctx, links, base=None, scratch_limit=None, stream=None):
        self.ctx, self.links, self._own, self.base = ctx, [], [], None
        try:
            for i, link in enumerate(links):
                if isinstance(link, SeekableStream):
                    if link.handle is None:
                        raise ZstdError("seekable chain: link %d is closed" % i)
                    if link.ctx is not ctx:
                        raise ZstdError("seekable chain: link %d was opened on another context" % i)
                else:
                    link = SeekableStream(ctx, link, stream=stream)
                    self._own.append(link)
                self.links.append(link)
            if not 1 <= len(self.links) <= 16:
                raise ZstdError("seekable chain: a chain has 1 ... 16 links, not %d" % len(self.links))
            L, first = ctx.L, self.links[0]
            self.element_size = int(L.zhip_seekable_element_size(first.handle))
            self.group_elements = int(L.zhip_seekable_group_elements(first.handle))
            self.content_size = first.content_size
            if base is not None:
                self.base = _base_bytes(base, first.tensor, self.content_size, "seekable chain")
            self.last_gather_stats, self._scratch_limit = None, scratch_limit
            if scratch_limit is not None:
                self.set_scratch_limit(scratch_limit)
            # the library's own verdict on the chain, now rather than at the first read: a call over no ranges decodes nothing
            self.read_ranges([], stream=stream)
        except Exception:
            self.close()
            raise

    def set_scratch_limit(self, nbytes):
        """SeekableStream.set_scratch_limit on EVERY link (the chain's plan is made with link 0's, and every link holds at most that much)"""
        for link in self.links:
            link.set_scratch_limit(nbytes)
        self._scratch_limit = nbytes

    def extended(self, stream_tensor_or_link):
        """a NEW chain with one more link behind this one's (the next version's delta); this chain stays open, and the links it opened stay its own"""
        return SeekableChain(self.ctx, self.links + [stream_tensor_or_link], base=self.base, scratch_limit=self._scratch_limit)

    def read(self, offset=0, length=None, out=None, stream=None):
        """the last version's bytes [offset, offset + length) (length None: to the end) as a uint8 CUDA tensor -- `out`, where given, else a new one"""
        if length is None:
            length = self.content_size - offset
        if offset < 0 or length < 0 or offset + length > self.content_size:
            raise ZstdError("range %d + %d is outside the content (%d bytes)" % (offset, length, self.content_size))
        if out is not None:
            assert out.numel() >= length, "out is shorter than the range"
        return self.read_ranges([(offset, length)], out, None if out is None else [0], stream)[0]

    def read_ranges(self, ranges, out=None, out_offsets=None, stream=None):
        """SeekableStream.read_ranges on the last version: a list of views, one per range. Waits for the status"""
        if any(link.handle is None for link in self.links) or not self.links:
            raise ZstdError("the seekable chain is closed")
        table, n, lengths, need = _ranges_table(ranges, out, out_offsets)
        device = self.links[0].tensor.device
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            if out is None:
                out = torch.empty(need, dtype=torch.uint8, device=device)
            status = torch.zeros(2 + 2 * n, dtype=torch.int32, device=device)
            which = torch.zeros(1 + n, dtype=torch.int32, device=device)
        DeviceBatchContext._check(out, torch.uint8)
        L = self.ctx.L
        stats = _lib.SeekableGatherStats()
        handles = (C.c_void_p * len(self.links))(*[link.handle.value for link in self.links])
        rc = L.zhip_seekable_decompress_typed_ranges_chain_device(self.ctx.ctx, handles, len(self.links), None if self.base is None else self.base.data_ptr(),
                                                                  0 if self.base is None else self.base.numel(), table.ctypes.data, n, out.data_ptr(), out.numel(),
                                                                  status.data_ptr(), which.data_ptr(), C.byref(stats), s.cuda_stream)
        if rc:
            raise ZstdError("seekable chain read failed: %s" % _lib.last_error())
        self.last_gather_stats = {k: int(getattr(stats, k)) for k, _ in stats._fields_}
        err = _lib.Error()
        rc = L.zhip_ctx_sync(self.ctx.ctx, s.cuda_stream, status.data_ptr(), 1, C.byref(err))
        if rc == _lib.ERR_ZSTD:
            bad = int(status[1])
            raise ZstdError("seekable chain read: range %d: link %d: frame %d: %s" % (bad, int(which[1 + bad]), int(status[3 + 2 * bad]), _lib.error_name(err.zstdErr)))
        if rc:
            raise ZstdError("HIP backend failure: %s" % _lib.last_error())
        return [out[int(table[k, 2]):int(table[k, 2]) + lengths[k]] for k in range(n)]

    def close(self):
        """closes the links this chain opened; the caller's SeekableStreams stay open"""
        for link in self._own:
            link.close()
        self._own, self.links = [], []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
