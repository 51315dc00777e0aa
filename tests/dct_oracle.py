"""A DCT-capable CPU oracle, built at test time.  The stock oracle (oracle/mvo_analyse.c) refuses dct 1..4; this helper copies its text into a
temporary directory, removes those refusals, routes the luma cost of modes 1..4 into tests/dct_emu.cpp -- csrc/mvx_dct_block.h compiled for the
host -- compiles the result with the other oracle sources and the oracle Makefile's CFLAGS, and loads it through a second instance of the
oracle's binding module.  Nothing generated is committed; every anchor must match exactly as often as expected.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ORACLE = os.path.join(ROOT, "oracle")
CSRC = os.path.join(ROOT, "vapoursynth-mvtools_amd", "csrc")

# (anchor line, replacement, expected matches)
_ANCHORS = [
    ('    if (d->dctmode >= 1 && d->dctmode <= 4) FAIL("Analyse: dct 1..4 need FFTW3 (out of scope for the oracle).");\n', "", 1),
    ('    if (an->dctmode >= 1 && an->dctmode <= 4) FAIL("Recalculate: dct 1..4 need FFTW3 (out of scope for the oracle).");\n', "", 1),
    ("    if (m == 0) return blk_sad(p, 0, ref0);\n",
     "    if (m == 0) return blk_sad(p, 0, ref0);\n"
     "    if (m >= 1 && m <= 4)\n"
     "        return dct_emu_luma_cost(p->pSrc[0], p->nSrcPitch[0], ref0, p->nRefPitch[0], p->nBlkSizeX, p->nBlkSizeY, p->bits, m, p->srcLuma, p->dctweight16);\n", 1),
    ("static int64_t luma_sad(pob *p, const uint8_t *ref0) {\n",
     "long long dct_emu_luma_cost(const void *src, long spitch, const void *ref, long rpitch, int bw, int bh, int bits, int mode, int srcLuma, int weight16);\n"
     "static int64_t luma_sad(pob *p, const uint8_t *ref0) {\n", 1),
]


def patched_source():
    text = open(os.path.join(ORACLE, "mvo_analyse.c")).read()
    for anchor, new, count in _ANCHORS:
        assert text.count(anchor) == count, "oracle anchor matches %d times, expected %d: %r" % (text.count(anchor), count, anchor)
        text = text.replace(anchor, new)
    assert "need FFTW3" not in text
    return text


def _cflags():
    mk = open(os.path.join(ORACLE, "Makefile")).read()
    m = re.findall(r"^CFLAGS\s*=\s*(.*)$", mk, flags=re.M)
    assert len(m) == 1, "oracle/Makefile: CFLAGS"
    return m[0].split()


_tmp = None  # keeps the temporary directory alive for the session
_emu = None
_mod = {}


def _dir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.TemporaryDirectory(prefix="mvx_dct_oracle_")
    return _tmp.name


def build_emu():
    """tests/dct_emu.cpp as a shared library -> path"""
    so = os.path.join(_dir(), "libdct_emu.so")
    if not os.path.exists(so):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I" + CSRC, os.path.join(HERE, "dct_emu.cpp"), "-o", so])
    return so


def emu():
    """ctypes handle of the host build of the library's DCT arithmetic"""
    global _emu
    if _emu is None:
        L = C.CDLL(build_emu())
        L.dct_emu_coeffs.argtypes = [C.c_void_p, C.c_ssize_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.dct_emu_coeffs.restype = None
        L.dct_emu_block.argtypes = [C.c_void_p, C.c_ssize_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.dct_emu_block.restype = None
        L.dct_emu_quant.argtypes = [C.c_float, C.c_int, C.c_int, C.c_int]
        L.dct_emu_cost_formula.argtypes = [C.c_int, C.c_longlong, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int]
        L.dct_emu_cost_formula.restype = C.c_longlong
        L.dct_emu_luma_cost.argtypes = [C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t] + [C.c_int] * 6
        L.dct_emu_luma_cost.restype = C.c_longlong
        _emu = L
    return _emu


def emu_coeffs(block, bits):
    b = np.ascontiguousarray(block)
    out = np.zeros(b.shape, dtype=np.float32)
    emu().dct_emu_coeffs(b.ctypes.data, b.strides[0], b.shape[1], b.shape[0], bits, out.ctypes.data)
    return out


def emu_bytes(block, bits):
    b = np.ascontiguousarray(block)
    out = np.zeros(b.shape, dtype=b.dtype)
    emu().dct_emu_block(b.ctypes.data, b.strides[0], b.shape[1], b.shape[0], bits, out.ctypes.data)
    return out


def emu_luma_cost(src, ref, bits, mode, src_luma, weight16):
    s, r = np.ascontiguousarray(src), np.ascontiguousarray(ref)
    return int(emu().dct_emu_luma_cost(s.ctypes.data, s.strides[0], r.ctypes.data, r.strides[0], s.shape[1], s.shape[0], bits, mode, int(src_luma), int(weight16)))


def build_oracle(f64=False):
    """the patched oracle as one shared library (the oracle's C sources + the emu) -> path.  f64: the emu's float64 variant (tools/dct_precision.py)"""
    d = os.path.join(_dir(), "f64" if f64 else "f32")
    so = os.path.join(d, "libmvoracle_dct.so")
    if os.path.exists(so):
        return so
    os.makedirs(d)
    open(os.path.join(d, "mvo_analyse_dct.c"), "w").write(patched_source())
    objs = []
    for src in ("mvo_super.c", "mvo_degrain.c", "mvo_blockfps.c"):
        o = os.path.join(d, src[:-2] + ".o")
        subprocess.check_call(["gcc"] + _cflags() + ["-I" + ORACLE, "-c", os.path.join(ORACLE, src), "-o", o])
        objs.append(o)
    o = os.path.join(d, "mvo_analyse_dct.o")
    subprocess.check_call(["gcc"] + _cflags() + ["-I" + ORACLE, "-c", os.path.join(d, "mvo_analyse_dct.c"), "-o", o])
    objs.append(o)
    o = os.path.join(d, "dct_emu.o")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-I" + CSRC, "-c", os.path.join(HERE, "dct_emu.cpp"), "-o", o]
                          + (["-DDCT_EMU_F64"] if f64 else []))
    objs.append(o)
    subprocess.check_call(["g++", "-shared", "-o", so] + objs + ["-lm"])
    return so


def module(f64=False):
    """a second instance of the oracle's binding module (oracle/mvoracle.py) whose build() points at the patched library"""
    if f64 not in _mod:
        so = build_oracle(f64)
        spec = importlib.util.spec_from_file_location("mvoracle_dct" + ("_f64" if f64 else ""), os.path.join(ORACLE, "mvoracle.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build = lambda force=False: so
        mod.lib()
        _mod[f64] = mod
    return _mod[f64]


def flat_clip(frames, bits=8):
    """the same motion at a 32nd of the contrast around mid-grey: no block's luma sum is a 32nd away from any other's, so the luma switch of
    dct 3 / 4 never fires"""
    half = 1 << (bits - 1)
    return [[(half + (p.astype(np.int64) - half) // 32).astype(p.dtype) for p in f] for f in frames]


def luma_ramp(frames, bits, ramp=40, which=1):
    """a brightness change on one frame (8-bit scale), stronger to the right, as the parity suite's _lumaramp: dctweight16 becomes non-zero and
    the luma switch of dct 3 / 4 fires"""
    y = frames[which][0]
    v = y.astype(np.int64) + (np.linspace(0, ramp, y.shape[1])[None, :] * (1 << (bits - 8))).astype(np.int64)
    y[...] = np.clip(v, 0, (1 << bits) - 1).astype(y.dtype)
    return frames
