"""CPU tests of mv.Flow / mv.FlowBlur creation (mvx_flowcomp_create / mvx_flowblur_create touch no device): the reference's checks and
messages in its order (MVFlow.cpp:391-593, MVFlowBlur.c:346-552, MVAnalysisData.c:7-31,68-98), Flow's reference frame, the argument
rounding; and of the restatement tests/flowmc_ref.py: its shift winners against a literal transcription of flowShift, properties of the
three kernels, and the int16 resizer on FlowBlur's unpadded geometries against the reference's AVX2 object code."""
import json
import os

import numpy as np
import pytest

import flow_ref
import flowmc_ref
import test_flow_ref

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "golden", "flowblur_ref_objects.json")
# FlowBlur's upsizer (MVFlowBlur.c:525-536): src = nBlkX x nBlkY (no padding), dst = limit = the plane; grids that do not cover the frame
# (8/4 blocks at 206 x 118: 50 x 28 blocks cover 204 x 116), chroma of 4:2:0 / 4:2:2, pel 1 / 2 / 4, both directions
GEOMETRIES = [(50, 28, 206, 118, 206, 118, 2, 1), (50, 28, 206, 118, 206, 118, 2, 0), (50, 28, 103, 59, 103, 59, 2, 1), (50, 28, 103, 59, 103, 59, 2, 0),
              (24, 13, 200, 120, 200, 120, 4, 1), (24, 13, 200, 120, 200, 120, 4, 0), (31, 23, 128, 96, 128, 96, 1, 1), (31, 23, 64, 96, 64, 96, 1, 0),
              (239, 134, 1920, 1080, 1920, 1080, 2, 1), (239, 134, 960, 540, 960, 540, 2, 0)]


def _pair(mv, w=320, h=192, bits=8, sup_kw=None, **akw):
    sup = mv.Super(w, h, bits, **(sup_kw or {}))
    bw = mv.Analyse(sup, isb=1, **akw).ad
    fw = mv.Analyse(sup, isb=0, **akw).ad
    return sup, bw, fw


def _copy(mv, ad, **fields):
    a = mv.AnalysisData.from_buffer_copy(bytes(ad))
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def _err(call):
    import mvtools_amd
    with pytest.raises(mvtools_amd.MvtoolsError) as e:
        call()
    return str(e.value)


def _flow(mv, sup, ad, **kw):
    return mv.Flow(sup, ad, 10, [320, 160, 160], **kw)


def _blur(mv, sup, bw, fw, **kw):
    return mv.FlowBlur(sup, bw, fw, 10, [320, 160, 160], **kw)


def test_flow_argument_checks(mv):
    sup, bw, fw = _pair(mv)
    assert _err(lambda: _flow(mv, sup, bw, time=-0.5)) == "Flow: time must be between 0 and 100 % (inclusive)."
    assert _err(lambda: _flow(mv, sup, bw, time=100.5)) == "Flow: time must be between 0 and 100 % (inclusive)."
    assert _err(lambda: _flow(mv, sup, bw, mode=2)) == "Flow: mode must be 0 or 1."
    assert _err(lambda: _flow(mv, sup, bw, mode=-1)) == "Flow: mode must be 0 or 1."
    assert _err(lambda: _flow(mv, sup, bw, time=200.0, mode=5)).startswith("Flow: time")           # time is checked first
    assert _err(lambda: _flow(mv, sup, bw, thscd1=16321)) == "Flow: thscd1 can be at most 16320."
    assert _err(lambda: _flow(mv, sup, bw, mode=3, thscd1=16321)) == "Flow: mode must be 0 or 1."
    _flow(mv, sup, bw, thscd1=16320)
    assert _err(lambda: _flow(mv, mv.Super(336, 192, 8), bw)) == "Flow: wrong source or super clip frame size."
    assert _err(lambda: _flow(mv, mv.Super(320, 192, 8, pel=4), bw)) == "Flow: wrong source or super clip frame size."
    assert _err(lambda: _flow(mv, mv.Super(336, 192, 8), bw, thscd1=99999)) == "Flow: thscd1 can be at most 16320."
    # unlike FlowInter / FlowBlur, Flow takes vectors with absolute frame references and either direction
    _flow(mv, sup, _copy(mv, fw, nDeltaFrame=-3))
    _flow(mv, sup, fw, mode=1)
    # the deliberate divergence: a single block column
    tiny = mv.Super(8, 64, 8)
    assert _err(lambda: _flow(mv, tiny, mv.Analyse(tiny, isb=1, blksize=8, overlap=0).ad)) == \
        "Flow: the frame must be at least two blocks wide and two blocks high."


def test_flowblur_argument_checks(mv):
    sup, bw, fw = _pair(mv)
    assert _err(lambda: _blur(mv, sup, bw, fw, blur=-0.5)) == "FlowBlur: blur must be between 0 and 200 % (inclusive)."
    assert _err(lambda: _blur(mv, sup, bw, fw, blur=200.5)) == "FlowBlur: blur must be between 0 and 200 % (inclusive)."
    assert _err(lambda: _blur(mv, sup, bw, fw, prec=0)) == "FlowBlur: prec must be at least 1."
    assert _err(lambda: _blur(mv, sup, bw, fw, blur=300.0, prec=0)).startswith("FlowBlur: blur")   # blur is checked first
    assert _err(lambda: _blur(mv, sup, bw, fw, prec=0, thscd1=99999)) == "FlowBlur: prec must be at least 1."
    assert _err(lambda: _blur(mv, sup, bw, fw, thscd1=16321)) == "FlowBlur: thscd1 can be at most 16320."
    _blur(mv, sup, bw, fw, thscd1=16320, prec=64, blur=200.0)
    # the similarity check: the LAST mismatching field's message wins
    assert _err(lambda: _blur(mv, sup, bw, _copy(mv, fw, nWidth=336))) == "FlowBlur: mvbw and mvfw have different widths."
    assert _err(lambda: _blur(mv, sup, bw, _copy(mv, fw, nWidth=336, nPel=4))) == "FlowBlur: mvbw and mvfw have different pel precision."
    assert _err(lambda: _blur(mv, sup, bw, _copy(mv, fw, nBlkSizeX=16, nOverlapY=2))) == "FlowBlur: mvbw and mvfw have different overlap."
    assert _err(lambda: _blur(mv, sup, bw, _copy(mv, fw, nWidth=336), thscd1=99999)) == "FlowBlur: thscd1 can be at most 16320."
    assert _err(lambda: _blur(mv, sup, _copy(mv, bw, nDeltaFrame=0), _copy(mv, fw, nDeltaFrame=0))) == \
        "FlowBlur: cannot use motion vectors with absolute frame references."
    assert _err(lambda: _blur(mv, sup, bw, _copy(mv, fw, nDeltaFrame=2))) == "FlowBlur: mvbw and mvfw must be generated with the same delta."
    assert _err(lambda: _blur(mv, sup, fw, fw)) == "FlowBlur: mvbw must be generated with isb=True."
    assert _err(lambda: _blur(mv, sup, bw, bw)) == "FlowBlur: mvfw must be generated with isb=False."
    assert _err(lambda: _blur(mv, mv.Super(336, 192, 8), bw, fw)) == "FlowBlur: wrong source or super clip frame size."
    assert _err(lambda: _blur(mv, mv.Super(320, 192, 8, pel=1), bw, fw)) == "FlowBlur: wrong source or super clip frame size."
    assert _err(lambda: _blur(mv, mv.Super(336, 192, 8), _copy(mv, bw, nDeltaFrame=0), _copy(mv, fw, nDeltaFrame=0))) == \
        "FlowBlur: cannot use motion vectors with absolute frame references."
    tiny = mv.Super(64, 8, 8)
    tb, tf = mv.Analyse(tiny, isb=1, blksize=8, overlap=0).ad, mv.Analyse(tiny, isb=0, blksize=8, overlap=0).ad
    assert _err(lambda: _blur(mv, tiny, tb, tf)) == "FlowBlur: the frame must be at least two blocks wide and two blocks high."


@pytest.mark.parametrize("isb,delta", [(1, 1), (0, 1), (1, 2), (0, 3), (0, -2), (1, 0)])
def test_flow_reference_frame(mv, isb, delta):
    """MVFlow.cpp:170-176: n + delta (isb), n - delta, or the absolute frame -delta"""
    sup = mv.Super(320, 192, 8)
    ad = mv.Analyse(sup, isb=isb, delta=delta if delta > 0 else 1).ad
    ad = _copy(mv, ad, nDeltaFrame=delta)
    g = _flow(mv, sup, ad)
    ref = flowmc_ref.Flow(ad, 10, 3, 16, 16, 8)
    for n in range(10):
        want = (n + delta if isb else n - delta) if delta > 0 else -delta
        assert g.ref(n) == ref.ref(n) == want, (n, isb, delta)


def test_time_and_blur_rounding():
    """Flow forms time256 in double (MVFlow.cpp:434), FlowBlur forms blur256 in float (MVFlowBlur.c:385): at these arguments the other
    precision gives the other value"""
    import mvoracle
    ad = mvoracle.AnalysisData(nBlkSizeX=8, nBlkSizeY=8, nOverlapX=4, nOverlapY=4, nBlkX=10, nBlkY=10, nWidth=44, nHeight=44, nPel=2,
                               nDeltaFrame=1, isBackward=1, xRatioUV=2, yRatioUV=2, bitsPerSample=8)
    assert flowmc_ref.Flow(ad, 10, 3, 16, 16, 8, time=0.39062499).time256 == 0
    assert int(np.float32(0.39062499) * np.float32(256.0) / np.float32(100.0)) == 1
    assert flowmc_ref.Flow(ad, 10, 3, 16, 16, 8, time=37.5).time256 == 96
    assert flowmc_ref.FlowBlur(ad, ad, 10, 3, 16, 16, 8, blur=0.78124999).blur256 == 1
    assert int(0.78124999 * 256.0 / 200.0) == 0
    assert flowmc_ref.FlowBlur(ad, ad, 10, 3, 16, 16, 8, blur=50.0).blur256 == 64


@pytest.mark.parametrize("pel,t,seed", [(1, 256, 1), (2, 256, 2), (4, 200, 3), (2, 97, 4), (1, 0, 5)])
def test_shift_winners_match_the_loop(pel, t, seed):
    """the scatter's winner rule (largest raster index) reproduces flowShift's last-writer-wins loop, holes keeping pixel_max"""
    rng = np.random.default_rng(seed)
    h, w = 13, 17
    src = rng.integers(0, 256, (h, w)).astype(np.uint8)
    vx = rng.integers(-6 * pel, 6 * pel, (h, w)).astype(np.int16)
    vy = rng.integers(-5 * pel, 5 * pel, (h, w)).astype(np.int16)
    fin = np.repeat(np.repeat(src, pel, 0), pel, 1)
    stats = {}
    got = flowmc_ref.shift(fin, (0, 0), (vx, vy), t, pel, w, h, 8, np.uint8, stats)
    assert np.array_equal(got, flowmc_ref.shift_loop(src, vx, vy, t, pel, 8))
    if t:
        assert stats["collide"] > 0 and stats["hole"] > 0


def test_zero_vectors_reproduce_the_frame():
    """zero vectors: fetch and shift return the integer-pel frame at every time, FlowBlur takes no taps"""
    rng = np.random.default_rng(6)
    h, w = 20, 36
    for pel in (1, 2, 4):
        src = rng.integers(0, 1 << 10, (h, w)).astype(np.uint16)
        fin = np.pad(np.repeat(np.repeat(src, pel, 0), pel, 1), 8)
        z = (np.zeros((h, w), np.int16), np.zeros((h, w), np.int16))
        for t in (0, 1, 128, 256):
            assert np.array_equal(flowmc_ref.fetch(fin, (8, 8), z, t, pel, w, h, np.uint16), src)
            assert np.array_equal(flowmc_ref.shift(fin, (8, 8), z, t, pel, w, h, 10, np.uint16), src)
        stats = {}
        assert np.array_equal(flowmc_ref.blur(fin, (8, 8), z, z, 256, 1, pel, w, h, np.uint16, stats), src)
        assert stats["taps"] == 0 and stats["notaps"] == h * w


def test_shift_by_a_uniform_vector_translates():
    """a uniform vector (-3, 2) at time 100 and pel 1 moves the frame by (3, -2); the uncovered border keeps pixel_max"""
    rng = np.random.default_rng(7)
    h, w = 16, 24
    src = rng.integers(0, 255, (h, w)).astype(np.uint8)
    v = (np.full((h, w), -3, np.int16), np.full((h, w), 2, np.int16))
    out = flowmc_ref.shift(src, (0, 0), v, 256, 1, w, h, 8, np.uint8)
    want = np.full((h, w), 255, np.uint8)
    want[:h - 2, 3:] = src[2:, :w - 3]
    assert np.array_equal(out, want)


def test_blur_at_zero_gives_the_frame():
    """blur=0: blur256 = 0, so no sample takes a tap whatever the vectors"""
    rng = np.random.default_rng(8)
    h, w, pel = 14, 22, 2
    src = rng.integers(0, 256, (h, w)).astype(np.uint8)
    fin = np.pad(np.repeat(np.repeat(src, pel, 0), pel, 1), 16)
    v = (rng.integers(-9, 9, (h, w)).astype(np.int16), rng.integers(-9, 9, (h, w)).astype(np.int16))
    assert np.array_equal(flowmc_ref.blur(fin, (16, 16), v, v, 0, 1, pel, w, h, np.uint8), src)


def test_blur_divisions_truncate():
    """a vector of -7 at blur256 = 100, prec 1: v0 = -700, m = 2, v0 / m = -350 (C truncation) where floor division also gives -350; at
    prec 3, m = 0 (no taps); at blur256 = 97: v0 = -679, m = 2, -679 / 2 = -339 in C (floor would give -340), taps at -339 >> 8 = -2 and
    -678 >> 8 = -3"""
    assert int(flowmc_ref.cdiv(np.int64(-679), np.int64(2))) == -339
    h, w = 1, 1
    fin = np.arange(25 * 25, dtype=np.int64).reshape(25, 25).astype(np.uint16)
    v = (np.full((1, 1), -7, np.int16), np.zeros((1, 1), np.int16))
    z = (np.zeros((1, 1), np.int16), np.zeros((1, 1), np.int16))
    stats = {}
    out = flowmc_ref.blur(fin, (12, 12), z, v, 97, 1, 1, w, h, np.uint16, stats)
    assert int(out[0, 0]) == (fin[12, 12] + fin[12, 10] + fin[12, 9]) // 3
    assert stats["trunc"] == 1 and stats["taps"] == 1
    assert int(flowmc_ref.blur(fin, (12, 12), z, v, 100, 3, 1, w, h, np.uint16)[0, 0]) == fin[12, 12]


def test_int16_resizer_on_flowblur_geometries():
    """FlowBlur's upsizer is flow_ref's int16 resizer on unpadded grids with the destination at the limit: pinned against the reference's
    AVX2 object code (oracle/_ref when built, else the digests recorded from it)"""
    lib = test_flow_ref.ref_lib()
    with open(RECORD) as f:
        rec = json.load(f)["simpleResize_int16_t_avx2"]
    assert len(rec) == len(GEOMETRIES)
    for g, want in zip(GEOMETRIES, rec):
        sw, sh, dw, dh, lw, lh, pel, horizontal = g
        ours = flow_ref.upsize_i16(test_flow_ref._field(sw, sh, sw * 100 + dw + horizontal), dw, dh, lw, lh, pel, horizontal)
        if lib is not None:
            assert np.array_equal(ours, test_flow_ref.ref_resize_i16(lib, *g)), g
        assert test_flow_ref.digest(ours) == want, g

