"""What the double-fast tests share (test_emu_dfast.py, test_emu_dfast_mutants.py, the runner in dfast_mutants.py, the seed chooser and the fixture writer of dfast_sources.py): libzstd
1.5.7's parse of a source (ZSTD_generateSequences, with or without a raw-content dictionary), the binding of emu/emu_dfast.cpp, and the comparison of the two. No test lives here
and nothing here imports a test module; dfast_sources.py imports this module only inside the two tools that need libzstd."""
import ctypes as C
import os
import subprocess

import numpy as np

BLOCK = 131072
STRATEGY_DFAST = 2
HERE = os.path.dirname(os.path.abspath(__file__))
FORMS = ("serial", "flat2", "flat3", "flat4", "blocks2", "blocks4", "g", "ext")          # ext: sources with a dictionary only, and they run nothing else


class _Seq(C.Structure):          # ZSTD_Sequence (zstd.h)
    _fields_ = [("offset", C.c_uint), ("litLength", C.c_uint), ("matchLength", C.c_uint), ("rep", C.c_uint)]


class _CPar(C.Structure):         # ZSTD_compressionParameters (zstd.h)
    _fields_ = [(k, C.c_uint) for k in ("window_log", "chain_log", "hash_log", "search_log", "min_match", "target_length", "strategy")]


class Lz:
    """libzstd 1.5.7: the sequences of a source, block by block, and the parameters it resolves for it"""

    def __init__(self):
        from tests import reflib
        self.ref = reflib.RefZstd()
        L = self.L = self.ref.lib
        L.ZSTD_createCCtx.restype = C.c_void_p
        L.ZSTD_sequenceBound.restype = C.c_size_t; L.ZSTD_sequenceBound.argtypes = [C.c_size_t]
        L.ZSTD_generateSequences.restype = C.c_size_t; L.ZSTD_generateSequences.argtypes = [C.c_void_p, C.POINTER(_Seq), C.c_size_t, C.c_char_p, C.c_size_t]
        L.ZSTD_getCParams.restype = _CPar; L.ZSTD_getCParams.argtypes = [C.c_int, C.c_ulonglong, C.c_size_t]
        L.ZSTD_adjustCParams.restype = _CPar; L.ZSTD_adjustCParams.argtypes = [_CPar, C.c_ulonglong, C.c_size_t]
        L.ZSTD_CCtx_loadDictionary_advanced.restype = C.c_size_t; L.ZSTD_CCtx_loadDictionary_advanced.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_int]
        self.cache = {}

    def cparams(self, n, level=3, **params):
        """what ZSTD_getCParamsFromCCtxParams makes of a level and explicit fields for a source of n bytes"""
        p = self.L.ZSTD_getCParams(level, n, 0)
        for k, v in params.items(): setattr(p, k, v)
        p = self.L.ZSTD_adjustCParams(p, n, 0)
        return {k: getattr(p, k) for k, _ in _CPar._fields_}

    def __call__(self, raw, level=3, dict_data=None, **params):
        """[(sequences [(position, matchLength, offset)], last literals, end)] per block; dict_data: a raw-content dictionary loaded into the context (offsets reach into it)"""
        key = (raw, level, dict_data, tuple(sorted(params.items())))
        if key in self.cache: return self.cache[key]
        L = self.L
        ctx = C.c_void_p(L.ZSTD_createCCtx())
        try:
            L.ZSTD_CCtx_setParameter(ctx, 100, level)
            for k, v in params.items():
                assert not L.ZSTD_isError(L.ZSTD_CCtx_setParameter(ctx, self.ref.PARAM_IDS[k], v))
            if dict_data is not None: assert not L.ZSTD_isError(L.ZSTD_CCtx_loadDictionary_advanced(ctx, dict_data, len(dict_data), 0, 1))          # by copy, raw content
            cap = L.ZSTD_sequenceBound(len(raw))
            buf = (_Seq * cap)()
            n = L.ZSTD_generateSequences(ctx, buf, cap, raw, len(raw))
            assert not L.ZSTD_isError(n), (len(raw), level, params)
            a = np.frombuffer(buf, dtype=np.uint32, count=4 * n).reshape(n, 4).tolist()
        finally:
            L.ZSTD_freeCCtx(ctx)
        blocks, cur, pos = [], [], 0
        for off, ll, ml, _ in a:
            if off == 0 and ml == 0: pos += ll; blocks.append((cur, ll, pos)); cur = []
            else: cur.append((pos + ll, ml, off)); pos += ll + ml
        assert pos == len(raw) and not cur
        if len(self.cache) < 4000: self.cache[key] = blocks
        return blocks


def build_emu(out_dir, header=None):
    """compiles emu_dfast.cpp (against another copy of the encoder header when one is given) and returns the library's path"""
    out = os.path.join(str(out_dir), "libzhip_emu_dfast.so")
    emu = os.path.join(HERE, "emu")
    cmd = ["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-I" + emu, "-w", "-o", out, os.path.join(emu, "zhemu.cpp"), os.path.join(emu, "emu_dfast.cpp")]
    if header: cmd[1:1] = ['-DZHIP_DFAST_HEADER="%s"' % header, "-I" + os.path.join(os.path.dirname(HERE), "python-zstandard_amd", "csrc")]     # (the copy includes its neighbours by name)
    subprocess.check_call(cmd)
    return out


class Emu:
    def __init__(self, path):
        lib = self.lib = C.CDLL(path)
        u8p, u32p, u64p, i = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_int
        lib.emu_dfast_serial.restype = C.c_uint32; lib.emu_dfast_serial.argtypes = [u8p, C.c_uint32, i, i, i, u64p]
        lib.emu_dfast_flat.restype = C.c_uint32; lib.emu_dfast_flat.argtypes = [u8p, C.c_uint32, i, i, i, i, C.c_uint32, u32p, u64p]
        lib.emu_dfast_blocks.restype = C.c_uint32; lib.emu_dfast_blocks.argtypes = [u8p, u32p, C.c_uint32, i, i, i, i, u64p, u32p, u32p]
        lib.emu_dfast_ext_dict.restype = C.c_int; lib.emu_dfast_ext_dict.argtypes = [u8p, C.c_uint32, i]
        lib.emu_dfast_ext.restype = C.c_int64; lib.emu_dfast_ext.argtypes = [u8p, C.c_uint32, u32p, C.c_uint32, u64p, u32p, u32p]
        self.dict_key = None
        lib.emu_dfast_g_blocks.restype = C.c_uint32; lib.emu_dfast_g_blocks.argtypes = [u8p, u32p, C.c_uint32, i, i, i, i, u64p, u32p, u32p]
        self.p = (u8p, u32p, u64p)

    @staticmethod
    def _resolve(q, start, reps):
        """packed sequences -> [(position, matchLength, offset)] with the repeat-offset codes resolved against `reps` (updated in place), from position `start`"""
        ofb = (q & np.uint64(0xFFFFFFF)).tolist(); ll = ((q >> np.uint64(28)) & np.uint64(0x3FFFF)).tolist(); ml = (q >> np.uint64(46)).tolist()
        out, pos = [], start
        for i in range(len(ofb)):
            if ofb[i] > 3: off = ofb[i] - 3; reps[:] = [off, reps[0], reps[1]]
            else:
                k = ofb[i] - 1 + (1 if ll[i] == 0 else 0)
                if k == 0: off = reps[0]
                elif k == 3: off = reps[0] - 1; reps[:] = [off, reps[0], reps[1]]
                else: off = reps[k]; reps[:] = [off] + reps[:k] + reps[k + 1:]
            out.append((pos + ll[i], ml[i], off)); pos += ll[i] + ml[i]
        return out, pos

    def _src(self, raw):
        return np.frombuffer(raw, dtype=np.uint8).copy() if len(raw) else np.zeros(1, dtype=np.uint8)         # exactly len(raw) bytes: a search may not read past them

    def serial(self, raw, cp):
        u8p, u32p, u64p = self.p
        src = self._src(raw); seqs = np.zeros(len(raw) // 4 + 8, dtype=np.uint64)
        n = self.lib.emu_dfast_serial(src.ctypes.data_as(u8p), len(raw), cp["hash_log"], cp["chain_log"], cp["min_match"], seqs.ctypes.data_as(u64p))
        s, pos = self._resolve(seqs[:n], 0, [1, 4, 8])
        return [(s, len(raw) - pos, len(raw))]

    def flat(self, raw, cp, probes, epoch=0, tables=None):
        u8p, u32p, u64p = self.p
        assert 16 <= len(raw) <= BLOCK
        src = self._src(raw); seqs = np.zeros(len(raw) // 4 + 8, dtype=np.uint64)
        if tables is None: tables = np.zeros((1 << cp["hash_log"]) + (1 << cp["chain_log"]), dtype=np.uint32)
        assert len(tables) >= (1 << cp["hash_log"]) + (1 << cp["chain_log"])
        n = self.lib.emu_dfast_flat(src.ctypes.data_as(u8p), len(raw), cp["hash_log"], cp["chain_log"], cp["min_match"], probes, epoch, tables.ctypes.data_as(u32p), seqs.ctypes.data_as(u64p))
        s, pos = self._resolve(seqs[:n], 0, [1, 4, 8])
        return [(s, len(raw) - pos, len(raw))]

    def _blocks(self, fn, raw, ends, args):
        u8p, u32p, u64p = self.p
        src = self._src(raw); seqs = np.zeros(len(raw) // 4 + 8 * len(ends), dtype=np.uint64)
        e = np.array(ends, dtype=np.uint32); counts = np.zeros(len(ends), dtype=np.uint32); reps_out = np.zeros(2 * len(ends), dtype=np.uint32)
        fn(src.ctypes.data_as(u8p), e.ctypes.data_as(u32p), len(ends), *args, seqs.ctypes.data_as(u64p), counts.ctypes.data_as(u32p), reps_out.ctypes.data_as(u32p))
        out, start, bs, reps = [], 0, 0, [1, 4, 8]
        for j, be in enumerate(ends):
            s, pos = self._resolve(seqs[start: start + int(counts[j])], bs, reps)
            # what the search hands on as repeat offsets is what its sequences imply (the entropy stage and the next block rely on it)
            assert [int(reps_out[2 * j]), int(reps_out[2 * j + 1])] == reps[:2], ("repeat offsets out of block", j, reps_out[2 * j: 2 * j + 2].tolist(), reps)
            out.append((s, be - pos, be)); start += int(counts[j]); bs = be
        return out

    def blocks(self, raw, ends, cp, probes):
        return self._blocks(self.lib.emu_dfast_blocks, raw, ends, (cp["hash_log"], cp["chain_log"], cp["min_match"], probes))

    def g_blocks(self, raw, ends, cp):
        return self._blocks(self.lib.emu_dfast_g_blocks, raw, ends, (cp["window_log"], cp["hash_log"], cp["chain_log"], cp["min_match"]))

    def ext(self, raw, ends, dict_data, level):
        """ze_dfast_ext over the blocks of a frame compressed against a raw-content dictionary in table-copy mode"""
        u8p = self.p[0]
        if self.dict_key != (dict_data, level):
            d = np.frombuffer(dict_data, dtype=np.uint8).copy()
            assert self.lib.emu_dfast_ext_dict(d.ctypes.data_as(u8p), len(d), level) == 0
            self.dict_key = (dict_data, level)
        return self._blocks(lambda src, e, nb, *rest: self._ext_status(self.lib.emu_dfast_ext(src, len(raw), e, nb, *rest)), raw, ends, ())

    @staticmethod
    def _ext_status(n):
        assert n >= 0, "ze_dfast_ext's parameters refused: status %d" % -n

    def run(self, form, raw, ends, cp):
        """the parse of one form, or None where the form does not take the source"""
        n = len(raw)
        one = len(ends) == 1
        if form == "serial": return self.serial(raw, cp) if one else None
        if form.startswith("flat"): return self.flat(raw, cp, int(form[4:])) if one and 16 <= n else None
        windowed = (1 << cp["window_log"]) < n
        if form.startswith("blocks"): return self.blocks(raw, ends, cp, int(form[6:])) if not windowed and n < (1 << 22) - 8 and (not one or n >= 16) else None
        return self.g_blocks(raw, ends, cp)


def property_failures(case, blocks):
    """what of the case's property libzstd's parse does not show"""
    seqs = {s for b in blocks for s in b[0]}
    starts = {s[0] for s in seqs}
    out = ["no sequence %r" % (e,) for e in case.expect if tuple(e) not in seqs]
    out += ["a sequence at %d" % a for a in case.absent if a in starts]
    if case.last is not None and blocks[-1][1] != case.last: out.append("last literals %d, not %d" % (blocks[-1][1], case.last))
    return out


def param_sets(case, lz):
    """the parameter sets a case runs under, with what libzstd resolves them to: those whose resolved strategy is double-fast (level 4's row is greedy up to 16 KiB)"""
    out = []
    for p in case.params:
        cp = lz.cparams(len(case.raw), **p)
        if cp["strategy"] == STRATEGY_DFAST: out.append((p, cp))
    assert out
    return out


def differences(case, lz, emu, forms=FORMS):
    """[(form, parameters, first differing block, ours, libzstd's)] over the case's parameter sets; the case's property is asserted first"""
    out = []
    if case.dict_data is not None:                                 # table-copy mode against a dictionary: level 3 as it is, ze_dfast_ext alone
        if "ext" not in forms: return out
        want = lz(case.raw, dict_data=case.dict_data)
        bad = property_failures(case, want)
        assert not bad, "the SOURCE %r misses its aim with its dictionary (libzstd's parse does not show it): %s" % (case.name, "; ".join(bad))
        try:
            got = emu.ext(case.raw, [b[2] for b in want], case.dict_data, 3)
        except AssertionError as e:
            return [("ext", "level 3", 0, str(e), None, None, None)]
        if got != want:
            j = next(i for i in range(len(want)) if got[i] != want[i])
            k = next((i for i in range(min(len(got[j][0]), len(want[j][0]))) if got[j][0][i] != want[j][0][i]), min(len(got[j][0]), len(want[j][0])))
            out.append(("ext", "level 3", j, got[j][0][k: k + 2], got[j][1], want[j][0][k: k + 2], want[j][1]))
        return out
    for p, cp in param_sets(case, lz):
        want = lz(case.raw, **p)
        bad = property_failures(case, want)
        assert not bad, "the SOURCE %r misses its aim under %r (libzstd's parse does not show it): %s; libzstd near it: %s" % (
            case.name, p, "; ".join(bad), [s for b in want for s in b[0] if any(abs(s[0] - e[0]) < 40 for e in case.expect)][:8])
        ends = [b[2] for b in want]
        for form in forms:
            if form == "ext": continue
            try:
                got = emu.run(form, case.raw, ends, cp)
            except AssertionError as e:                          # (the repeat offsets a block form hands on)
                out.append((form, p, 0, str(e), None, None, None)); continue
            if got is None or got == want: continue
            j = next(i for i in range(len(want)) if got[i] != want[i])
            k = next((i for i in range(min(len(got[j][0]), len(want[j][0]))) if got[j][0][i] != want[j][0][i]), min(len(got[j][0]), len(want[j][0])))
            out.append((form, p, j, got[j][0][k: k + 2], got[j][1], want[j][0][k: k + 2], want[j][1]))
    return out


