"""CPU tests of the flow restatement tests/flow_ref.py: its int16 vector resizer against the reference's AVX2 object code (oracle/_ref when
built, else the digests recorded from it in tests/golden/flow_ref_objects.json), and two properties of the interpolation."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

import flow_ref

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SO = os.path.join(HERE, "..", "oracle", "_ref", "libmvref.so")
RECORD = os.path.join(HERE, "golden", "flow_ref_objects.json")
SYMBOL = "_Z25simpleResize_int16_t_avx2PK12SimpleResizePsiPKsii"
# (src_w = nBlkXP, src_h = nBlkYP, dst_w, dst_h, limit_w, limit_h, pel, horizontal): pel 1 / 2 / 4, both directions, widths that are no
# multiple of 8; nBlkXP >= 8 (below 8 columns the AVX2 form reads before its buffers)
GEOMETRIES = [(8, 6, 36, 28, 34, 26, 1, 1), (8, 6, 36, 28, 34, 26, 1, 0), (31, 17, 128, 72, 126, 70, 2, 1), (31, 17, 128, 72, 126, 70, 2, 0),
              (25, 15, 203, 123, 200, 120, 4, 1), (25, 15, 203, 123, 200, 120, 4, 0), (60, 34, 484, 276, 480, 270, 2, 1), (12, 9, 50, 37, 49, 37, 4, 0)]


class SimpleResize(C.Structure):  # SimpleResize.h:51-73
    _fields_ = [("dst_width", C.c_int), ("dst_height", C.c_int), ("src_width", C.c_int), ("src_height", C.c_int), ("limit_width", C.c_int),
                ("limit_height", C.c_int), ("pel", C.c_int), ("vertical_offsets", C.c_void_p), ("vertical_weights", C.c_void_p),
                ("horizontal_offsets", C.c_void_p), ("horizontal_weights", C.c_void_p), ("f8", C.c_void_p), ("f16", C.c_void_p)]


def ref_lib():
    return C.CDLL(REF_SO) if os.path.exists(REF_SO) else None


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _field(sw, sh, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-300, 300, (sh, sw)).astype(np.int16)


def ref_resize_i16(lib, sw, sh, dw, dh, lw, lh, pel, horizontal):
    src = np.zeros((sh + 1, sw + 16), np.int16)
    src[:sh, :sw] = _field(sw, sh, sw * 100 + dw + horizontal)
    vo, vw = flow_ref.resize_tables(dh, sh)
    ho, hw = np.zeros(dw + 16, np.int32), np.zeros(dw + 16, np.int32)  # (+16: the AVX2 form reads the tables eight entries at a time)
    ho[:dw], hw[:dw] = flow_ref.resize_tables(dw, sw)
    hw[:dw] = (hw[:dw] << 16) | (16384 - hw[:dw])  # the AVX2 form's packed weights (simpleInit, SimpleResize.cpp:148-159)
    s = SimpleResize(dw, dh, sw, sh, lw, lh, pel, vo.ctypes.data, vw.ctypes.data, ho.ctypes.data, hw.ctypes.data, None, None)
    dst = np.zeros((dh, dw + 16), np.int16)
    f = getattr(lib, SYMBOL)
    f.argtypes = [C.POINTER(SimpleResize), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
    f(C.byref(s), dst.ctypes.data, dst.shape[1], src.ctypes.data, src.shape[1], horizontal)
    return dst[:, :dw]


def test_int16_resizer_against_reference_object():
    lib = ref_lib()
    with open(RECORD) as f:
        rec = json.load(f)["simpleResize_int16_t_avx2"]
    assert len(rec) == len(GEOMETRIES)
    for g, want in zip(GEOMETRIES, rec):
        sw, sh, dw, dh, lw, lh, pel, horizontal = g
        ours = flow_ref.upsize_i16(_field(sw, sh, sw * 100 + dw + horizontal), dw, dh, lw, lh, pel, horizontal)
        if lib is not None:
            assert np.array_equal(ours, ref_resize_i16(lib, *g)), g
        assert digest(ours) == want, g


def _planes(rng, h, w, bits):
    return rng.integers(0, 1 << bits, (h, w)).astype(np.uint8 if bits == 8 else np.uint16)


def test_zero_vectors_reproduce_the_frame_8bit():
    """identical frames and zero vectors (hence zero occlusion masks): every formula returns the frame itself in 8 bit"""
    rng = np.random.default_rng(1)
    h, w, pel = 24, 40, 2
    fin = np.repeat(np.repeat(_planes(rng, h, w, 8), pel, 0), pel, 1)
    z = (np.zeros((h, w), np.int16), np.zeros((h, w), np.int16))
    for kind in ("simple", "regular", "extra"):
        for t in (1, 77, 128, 200):
            m = np.zeros((h, w), np.uint8)
            out = flow_ref.flow_inter(kind, t, fin, fin, (0, 0), pel, z, z, m, m, w, h, np.uint8, z, z)
            assert np.array_equal(out, fin[::pel, ::pel]), (kind, t)


def test_simple_has_its_own_formula_at_half_time():
    """FlowInterSimple at time256 == 128 (MaskFun.cpp:512-531) is not its general formula evaluated at 128"""
    rng = np.random.default_rng(2)
    h, w = 16, 32
    a, b = _planes(rng, h, w, 8), _planes(rng, h, w, 8)
    m1, m2 = rng.integers(0, 256, (h, w)).astype(np.uint8), rng.integers(0, 256, (h, w)).astype(np.uint8)
    z = (np.zeros((h, w), np.int16), np.zeros((h, w), np.int16))
    special = flow_ref.flow_inter("simple", 128, a, b, (0, 0), 1, z, z, m1, m2, w, h, np.uint8)
    dF, dB, MF, MB = b.astype(np.int64), a.astype(np.int64), m2.astype(np.int64), m1.astype(np.int64)
    general = ((((dF * (255 - MF) + dB * MF + 255) >> 8) * 128 + ((dB * (255 - MB) + dF * MB + 255) >> 8) * 128) >> 8).astype(np.uint8)
    assert not np.array_equal(special, general)
