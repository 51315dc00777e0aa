"""CPU tests of mv.Mask: creation (mvx_mask_create touches no device) with the reference's checks and messages in its order
(MVMask.c:227-346, MVAnalysisData.c:7-31) and the library's own rejections; the struct layouts; the argument rounding; the restatement
tests/mask_ref.py on hand-computed fields for every kind; its upsizer on Mask's unpadded geometries against the reference's AVX2 object
code; and the condition that tests/mask_cases.py puts on the inputs of the GPU parity cases."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import flow_ref
import mask_cases as mc
import mask_ref
import mvoracle
import test_flow_ref

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "golden", "mask_ref_objects.json")
# Mask's upsizers (MVMask.c:331-332): src = nBlkX x nBlkY (no padding), dst = the block-covered rectangle of the plane.  8/4 blocks at
# 206 x 118 (50 x 28 blocks cover 204 x 116) with the chroma of 4:2:0 and 4:2:2, 16/8 blocks there, grids that cover 128 x 96 and 1920 x 1080,
# 32/0 blocks at 1080p (33 rows cover 1056)
GEOMETRIES = [(50, 28, 204, 116), (50, 28, 102, 58), (50, 28, 102, 116), (24, 13, 200, 112), (24, 13, 100, 56), (31, 23, 128, 96), (31, 23, 64, 48),
              (31, 23, 64, 96), (479, 269, 1920, 1080), (479, 269, 960, 540), (60, 33, 1920, 1056), (60, 33, 960, 528)]


def _ad(mv, w=320, h=192, bits=8, sup_kw=None, **akw):
    return mv.Analyse(mv.Super(w, h, bits, **(sup_kw or {})), **dict(dict(isb=1), **akw)).ad


def _err(call):
    import mvtools_amd
    with pytest.raises(mvtools_amd.MvtoolsError) as e:
        call()
    return str(e.value)


FORMAT = "Mask: input clip must be GRAY8, YUV420P8, YUV422P8, YUV440P8, or YUV444P8, with constant dimensions."
BLOCKS = "Mask: the frame must be at least two blocks wide and two blocks high."
GEOMETRY = "Mask: the clip's size and chroma subsampling must be those of the vector clip."


def test_argument_checks_in_the_reference_order(mv):
    ad = _ad(mv)
    m = lambda **kw: mv.Mask(ad, kw.pop("w", 320), kw.pop("h", 192), **kw)
    assert _err(lambda: m(gamma=-0.5)) == "Mask: gamma must not be negative."
    assert _err(lambda: m(kind=6)) == "Mask: kind must 0, 1, 2, 3, 4, or 5."
    assert _err(lambda: m(kind=-1)) == "Mask: kind must 0, 1, 2, 3, 4, or 5."
    assert _err(lambda: m(time=-0.5)) == "Mask: time must be between 0.0 and 100.0 (inclusive)."
    assert _err(lambda: m(time=100.5)) == "Mask: time must be between 0.0 and 100.0 (inclusive)."
    assert _err(lambda: m(ysc=256)) == "Mask: ysc must be between 0 and 255 (inclusive)."
    assert _err(lambda: m(ysc=-1)) == "Mask: ysc must be between 0 and 255 (inclusive)."
    assert _err(lambda: m(thscd1=16321)) == "Mask: thscd1 can be at most 16320."
    assert _err(lambda: m(bits=16)) == FORMAT
    assert _err(lambda: m(subsampling=(2, 1))) == FORMAT
    assert _err(lambda: m(subsampling=(1, 2))) == FORMAT
    # the order: gamma, kind, time, ysc, the vector clip and thscd1, the format, then the library's own checks
    assert _err(lambda: m(gamma=-1.0, kind=9, time=200.0, ysc=999, thscd1=99999, bits=16)).startswith("Mask: gamma")
    assert _err(lambda: m(kind=9, time=200.0, ysc=999, thscd1=99999, bits=16)).startswith("Mask: kind")
    assert _err(lambda: m(time=200.0, ysc=999, thscd1=99999, bits=16)).startswith("Mask: time")
    assert _err(lambda: m(ysc=999, thscd1=99999, bits=16)).startswith("Mask: ysc")
    assert _err(lambda: m(thscd1=99999, bits=16)).startswith("Mask: thscd1")
    assert _err(lambda: m(bits=16, w=336)) == FORMAT
    # the limits themselves are accepted; a negative zero gamma is not negative
    m(gamma=0.0, kind=5, time=0.0, ysc=255, thscd1=16320)
    m(gamma=-0.0, kind=0, time=100.0, ysc=0)
    # gamma is a float argument: a negative double that rounds to -0.0f passes, as in the reference
    m(gamma=-1e-60)


def test_deliberate_divergences_are_rejected(mv):
    ad = _ad(mv)
    assert _err(lambda: mv.Mask(ad, 336, 192)) == GEOMETRY
    assert _err(lambda: mv.Mask(ad, 320, 200)) == GEOMETRY
    assert _err(lambda: mv.Mask(ad, 320, 192, subsampling=(0, 0))) == GEOMETRY
    assert _err(lambda: mv.Mask(ad, 320, 192, subsampling=(1, 0))) == GEOMETRY
    assert _err(lambda: mv.Mask(ad, 320, 192, gray=True)) == GEOMETRY                 # Gray counts as 1 / 1, the vectors are 2 / 2
    gray = mv.Analyse(mv.Super(320, 192, 8, gray=True, subsampling=(0, 0)), isb=1).ad
    assert (gray.xRatioUV, gray.yRatioUV) == (1, 1)
    info = mv.Mask(gray, 320, 192, gray=True).info                                     # Gray in -> 4:4:4 out
    assert (info.num_planes, info.subsampling_w, info.subsampling_h) == (3, 0, 0)
    assert list(info.plane_width) == [320] * 3 and list(info.plane_height) == [192] * 3
    mv.Mask(gray, 320, 192, subsampling=(0, 0))                                        # 4:4:4 has the same ratios
    for w, h in ((8, 64), (64, 8)):
        tiny = mv.Analyse(mv.Super(w, h, 8), isb=1, blksize=8, overlap=0).ad
        assert _err(lambda: mv.Mask(tiny, w, h)) == BLOCKS
        assert _err(lambda: mv.Mask(tiny, w, h, bits=16)) == FORMAT                    # the reference's checks come first
    assert "multiples of 16" in _err(lambda: mv.Mask(ad, 320, 192, dst_pitch=[328, 160, 160]))
    assert "multiples of 16" in _err(lambda: mv.Mask(ad, 320, 192, dst_pitch=[320, 160, 176]))
    info = mv.Mask(ad, 320, 192, subsampling=(1, 1)).info
    assert list(info.plane_width) == [320, 160, 160] and list(info.plane_height) == [192, 96, 96]


def test_struct_layouts_match_the_header(mv, tmp_path):
    root = os.path.dirname(HERE)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "mvtools_amd.h"\nint main(void) { printf("%d %d %d %d\\n", (int)sizeof(mvx_mask_args), '
                   '(int)sizeof(mvx_mask_clip), (int)sizeof(mvx_mask_info), (int)sizeof(mvx_mask_job)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(mv.MaskArgs), C.sizeof(mv.MaskClip), C.sizeof(mv.MaskInfo), C.sizeof(mv.MaskJob)] == [56, 24, 60, 40]


@pytest.mark.parametrize("kw,time256", [(dict(time=0.39062499), 0), (dict(time=37.5), 96), (dict(time=100.0), 256), (dict(time=0.0), 0),
                                        (dict(time=99.99999), 255), (dict(ml=3.0), 256), (dict(ml=1000.0, gamma=0.7), 256), (dict(gamma=0.1), 256)])
def test_argument_rounding(mv, kw, time256):
    """time is a double argument: time256 is formed in double (MVMask.c:334; 0.39062499 gives 1 in float).  ml and gamma are float arguments
    and the three factors are floats formed from them (MVMask.c:304-307): at ml = 3 and gamma = 0.7 the doubles differ.  The library
    (mvx_mask_get_info) and the restatement agree bit for bit."""
    ad = _ad(mv)
    info = mv.Mask(ad, 320, 192, **kw).info
    ref = mask_ref.Mask(ad, **kw)
    assert info.time256 == ref.time256 == time256
    f32 = np.float32
    ml, gamma = f32(kw.get("ml", 100.0)), f32(kw.get("gamma", 1.0))
    want = (f32(1.0) / ml, (f32(1.0) / ml) * (f32(1.0) / ml), gamma * f32(0.5))
    got = (f32(info.fMaskNormFactor), f32(info.fMaskNormFactor2), f32(info.fHalfGamma))
    assert got == want == (ref.fMaskNormFactor, ref.fMaskNormFactor2, ref.fHalfGamma)
    assert int(f32(0.39062499) * f32(256.0) / f32(100.0)) == 1
    if "ml" in kw:
        assert float(want[0]) != 1.0 / kw["ml"] and float(want[1]) != (1.0 / kw["ml"]) ** 2
    if kw.get("gamma") in (0.7, 0.1):
        assert float(want[2]) != kw["gamma"] * 0.5


# ---------------------------------------------------------------- the restatement on hand-computed fields

def _hand(vx, vy, sad, isb=0, pel=2, blk=8, valid=1):
    """analysis data and a one-level blob of a hand-made field (blocks of blk x blk without overlap)"""
    vx, vy, sad = np.asarray(vx, np.int32), np.asarray(vy, np.int32), np.asarray(sad, np.int64)
    nby, nbx = vx.shape
    ad = mvoracle.AnalysisData(nBlkSizeX=blk, nBlkSizeY=blk, nOverlapX=0, nOverlapY=0, nBlkX=nbx, nBlkY=nby, nWidth=nbx * blk + 3, nHeight=nby * blk + 2,
                               nPel=pel, nLvCount=1, nDeltaFrame=1, isBackward=isb, xRatioUV=2, yRatioUV=2, bitsPerSample=8, nHPadding=16, nVPadding=16)
    blob = np.zeros(12 + 16 * nbx * nby, np.uint8)
    blob[0:4].view(np.int32)[0] = blob.size
    blob[4:8].view(np.int32)[0] = valid
    blob[8:12].view(np.int32)[0] = 4 + 16 * nbx * nby
    rec = blob[12:].view(np.int32).reshape(nby, nbx, 4)
    rec[:, :, 0], rec[:, :, 1] = vx, vy
    blob[12:].view(np.int64).reshape(nby, nbx, 2)[:, :, 1] = sad
    return ad, blob


Z = [[0, 0, 0], [0, 0, 0]]


def test_kind0_by_hand():
    """(3, 4) at pel 2: norme = 25 / 4; ml = 5: fMaskNormFactor2 = 0.04f = 0.0400000028, so the base is 0.25 and a little.  gamma 2 (exponent
    1): 255 * 0.25.. = 63.75.. -> 63; gamma 1: 255 * sqrt = 127.5.. -> 127; gamma 0: pow = 1 -> 255, for the zero vector too (pow(0, 0) = 1);
    the zero vector at gamma 1 gives 0; (30, 40): 255 * 2.5 is cut"""
    ad, blob = _hand([[3, 0, 30], [0, 0, 0]], [[4, 0, 40], [0, 0, 0]], Z)
    for gamma, want in ((2.0, [63, 0, 255]), (1.0, [127, 0, 255]), (0.0, [255, 255, 255])):
        stats = {}
        small, v = mask_ref.Mask(ad, ml=5.0, gamma=gamma, kind=0).small_masks(blob, stats)
        assert v is None and list(small[0]) == want and list(small[1]) == [want[1]] * 3, gamma
        assert stats.get("cut", 0) == (1 if gamma else 0)


def test_kind1_by_hand():
    """8 x 8 blocks, ml = 5: factor = 4 * 0.2f / 64 = 0.0125 and a little; SAD 40 -> 127.5.. -> 127, SAD 100 -> cut, SAD 0 -> 0.  time 0, pel 2:
    time4096X = 256 * 16 / 16 = 256.  vx = 16 takes the SAD of the block one to the left (block 0: outside, falls back to itself);
    vx = -17: -17 * 256 / 4096 = -1 in C (floor: -2), the block one to the right.  At time 100 nothing moves.  gamma 0.5: sqrt(0.5) * 255 = 180.3"""
    ad, blob = _hand([[16, 16, -17], [0, 0, 0]], Z, [[40, 100, 0], [0, 40, 100]])
    stats = {}
    small, _ = mask_ref.Mask(ad, ml=5.0, kind=1, time=0.0).small_masks(blob, stats)
    assert [list(r) for r in small] == [[127, 127, 0], [0, 127, 255]]           # block (0,2): its source (0,3) is outside, falls back
    assert stats == dict(back=2, moved=1, trunc=1, cut=1)
    ad, blob = _hand([[16, 16, -17], [0, 0, 0]], Z, [[40, 100, 0], [40, 0, 0]])
    stats = {}
    small, _ = mask_ref.Mask(ad, ml=5.0, kind=1, time=0.0).small_masks(blob, stats)
    assert list(small[0]) == [127, 127, 0] and stats["back"] == 2
    ad, blob = _hand([[16, 16, -17, 0], [0, 0, 0, 0]], [[0] * 4] * 2, [[40, 100, 0, 40], [0, 0, 0, 0]])
    stats = {}
    small, _ = mask_ref.Mask(ad, ml=5.0, kind=1, time=0.0).small_masks(blob, stats)
    assert list(small[0]) == [127, 127, 127, 127] and stats == dict(back=1, moved=2, trunc=1)   # block 2 takes block 3's SAD: truncation
    small, _ = mask_ref.Mask(ad, ml=5.0, kind=1, time=100.0).small_masks(blob, {})
    assert list(small[0]) == [127, 255, 0, 127]
    small, _ = mask_ref.Mask(ad, ml=5.0, kind=1, time=100.0, gamma=0.5).small_masks(blob, {})
    assert list(small[0]) == [180, 255, 0, 180]


def test_kind2_by_hand():
    """step 8, pel 2, ml = 100: dMaskNormDivider = 1 / 0.01f = 100.0000022, occnorm = 80 / (that * 16) just below 0.05.  A fall of 4 between
    blocks 0 and 1: 255 * 4 * occnorm = 50.999998.. -> 50 (51 with a double ml); forward at time 100: time4096 = 256, 4 * 256 / 4096 = 0: the
    range is blocks 0..1.  gamma 2: 255 * (0.2-)^2 = 10.19.. -> 10.  A fall of 40: saturated; 40 * 256 / 4096 = 2, so the forward range
    0..min(1 - 2, 2) is empty, while the backward one is max(0, 1 - 2)..1.  Vertical falls likewise, down the column."""
    ad, blob = _hand([[4, 0, 0], [0, 0, 0]], Z, Z)
    for gamma, want in ((1.0, 50), (2.0, 10)):
        small, _ = mask_ref.Mask(ad, kind=2, gamma=gamma).small_masks(blob, {})
        assert [list(r) for r in small] == [[want, want, 0], [0, 0, 0]]
    assert int(255 * 4 * (80.0 / (100.0 * 8 * 2))) == 51
    ad, blob = _hand([[40, 0, 0], [0, 0, 0]], Z, Z)
    assert not mask_ref.Mask(ad, kind=2).small_masks(blob, {})[0].any()
    adb, blobb = _hand([[0, 40, 0], [0, 0, 0]], Z, Z, isb=1)
    stats = {}
    small, _ = mask_ref.Mask(adb, kind=2).small_masks(blobb, stats)
    assert [list(r) for r in small] == [[255, 255, 255], [0, 0, 0]] and stats == dict(span=1, cut=1)
    ad, blob = _hand(Z, [[0, 4, 0], [0, 0, 0]], Z)
    small, _ = mask_ref.Mask(ad, kind=2).small_masks(blob, {})
    assert [list(r) for r in small] == [[0, 50, 0], [0, 50, 0]]
    # gamma 0: pow(x, 0) = 1 -> 255 wherever there is an occlusion at all; time 0 leaves both ends of every range in place
    small, _ = mask_ref.Mask(ad, kind=2, gamma=0.0, time=0.0).small_masks(blob, {})
    assert [list(r) for r in small] == [[0, 255, 0], [0, 255, 0]]
    # beyond the int range the library saturates (the reference's cast is undefined there)
    assert mask_ref.Mask(ad, kind=2, gamma=30.0).occ_value(4000, 1.0, {}) == 255


def test_kinds_3_4_5_by_hand():
    """ml = 100: 7 * 0.01f * 100 + 128 = 135 in float; -200 -> below 0; 200 -> above 255.  ml = 3: 3 * (1/3)f * 100 + 128 = 228; -1 -> 94.67 -> 94;
    a negative value is truncated towards zero before the clamp: -129 * 0.01f * 100 + 128 = -1.0 and a little -> (int) -1 -> 0"""
    ad, blob = _hand([[7, -200, 200], [0, -1, 3]], [[0, 1, -129], [-7, 200, -200]], Z)
    stats = {}
    x, none = mask_ref.Mask(ad, kind=3).small_masks(blob, stats)
    assert none is None and [list(r) for r in x] == [[135, 0, 255], [128, 127, 131]] and stats["cut"] == 1
    y, _ = mask_ref.Mask(ad, kind=4).small_masks(blob, {})
    assert [list(r) for r in y] == [[128, 129, 0], [121, 255, 0]]
    u, v = mask_ref.Mask(ad, kind=5).small_masks(blob, {})
    assert np.array_equal(u, x) and np.array_equal(v, y)
    x3, _ = mask_ref.Mask(ad, kind=3, ml=3.0).small_masks(blob, {})
    assert [list(r) for r in x3] == [[255, 0, 255], [128, 94, 228]]


def test_frame_geometry_and_fallbacks_by_hand():
    """a constant small mask gives constant planes, edges included; U = V; kind 5 keeps the clip's luma; an unusable blob gives ysc"""
    ad, blob = _hand([[7] * 3] * 2, [[-7] * 3] * 2, Z)                                 # 27 x 18, the grid covers 24 x 16
    stats = {}
    y, u, v = mask_ref.Mask(ad, kind=3).frame(blob, None, stats)
    assert y.shape == (18, 27) and u.shape == v.shape == (9, 13) and np.all(y == 135) and np.all(u == 135) and np.array_equal(u, v)
    assert stats == dict(edgex=3 * 16 + 1 * 8, edgey=2 * 27 + 1 * 13)
    luma = np.arange(18 * 32, dtype=np.uint8).reshape(18, 32)
    y, u, v = mask_ref.Mask(ad, kind=5).frame(blob, luma, {})
    assert np.array_equal(y, luma[:, :27]) and np.all(u == 135) and np.all(v == 121)
    for b in (None, _hand([[7] * 3] * 2, [[-7] * 3] * 2, Z, valid=0)[1]):
        stats = {}
        y, u, v = mask_ref.Mask(ad, kind=5, ysc=200).frame(b, luma, stats)
        assert np.array_equal(y, luma[:, :27]) and np.all(u == 200) and np.all(v == 200) and stats == dict(sc=1)
        y, u, v = mask_ref.Mask(ad, kind=1, ysc=7).frame(b, None, {})
        assert np.all(y == 7) and np.all(u == 7) and np.all(v == 7)
    # a ramp: the right fill repeats column nWidthB - 1 of each row, the bottom fill repeats row nHeightB - 1 after that
    ad, blob = _hand([[0, 40, 80], [120, 160, 200]], Z, Z)
    y, u, _ = mask_ref.Mask(ad, kind=3, ml=200.0).frame(blob, None, {})
    assert np.array_equal(y[:16, :24], flow_ref.upsize_u8(np.array([[128, 148, 168], [188, 208, 228]], np.uint8), 24, 16))
    assert np.all(y[:16, 24:] == y[:16, 23:24]) and np.all(y[16:, :] == y[15:16, :]) and len(set(y[0])) > 3
    assert np.all(u[:8, 12:] == u[:8, 11:12]) and np.all(u[8:, :] == u[7:8, :])


def test_truncating_division():
    assert [mask_ref.cdiv(a, 4096) for a in (-4352, 4352, -4096, -1, 0, 8191)] == [-1, 1, -1, 0, 0, 1]
    assert -4352 // 4096 == -2


def test_pow_distance_definition():
    assert mask_ref.pow_distance(10.25, 0.3, 1.0) is None and mask_ref.pow_distance(0.0, 0.0, 0.5) is None
    assert mask_ref.pow_distance(255.0, 0.3, 0.0) is None
    assert mask_ref.pow_distance(10.25, 0.3, 0.5) == 0.25 and mask_ref.pow_distance(10.75, 0.3, 0.5) == 0.25
    assert mask_ref.pow_distance(255.5, 1.1, 0.5) == 0.5 and mask_ref.pow_distance(300.0, 1.1, 0.5) == 45.0


# ---------------------------------------------------------------- the upsizer on Mask's geometries

def _field(sw, sh, seed):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    f[::3, ::5] = 255
    f[1::4, 2::7] = 0
    return f


def ref_resize_u8(lib, sw, sh, dw, dh):
    """SimpleResize_AVX2.cpp's uint8_t form through oracle/_ref's ref_simple_resize_u8_avx2, with the tables as simpleInit packs them"""
    vp = C.c_void_p
    lib.ref_simple_resize_u8_avx2.argtypes = [vp, C.c_int, vp, C.c_int] + [C.c_int] * 4 + [vp] * 4
    src = np.zeros((sh + 1, sw + 8), np.uint8)   # (+1 row: the last output rows read offset + 1; +8: the gathers' over-read)
    src[:sh, :sw] = _field(sw, sh, sw * 100 + dw)
    vo, vw = flow_ref.resize_tables(dh, sh)
    ho, hw = np.zeros(dw + 8, np.int32), np.zeros(dw + 8, np.int32)
    ho[:dw], hw[:dw] = flow_ref.resize_tables(dw, sw)
    hw[:dw] = (hw[:dw] << 16) | (16384 - hw[:dw])
    dst = np.zeros((dh, dw + 8), np.uint8)
    lib.ref_simple_resize_u8_avx2(dst.ctypes.data, dst.shape[1], src.ctypes.data, src.shape[1], dw, dh, sw, sh, vo.ctypes.data, vw.ctypes.data,
                                  ho.ctypes.data, hw.ctypes.data)
    return dst[:, :dw]


def test_upsizer_on_mask_geometries():
    """the restatement's upsizer on Mask's unpadded geometries against the reference's AVX2 object code (oracle/_ref when built, else the
    digests recorded from it in tests/golden/mask_ref_objects.json)"""
    lib = test_flow_ref.ref_lib()
    with open(RECORD) as f:
        rec = json.load(f)["simpleResize_uint8_t_avx2"]
    assert len(rec) == len(GEOMETRIES)
    for g, want in zip(GEOMETRIES, rec):
        sw, sh, dw, dh = g
        ours = flow_ref.upsize_u8(_field(sw, sh, sw * 100 + dw), dw, dh)
        if lib is not None:
            assert np.array_equal(ours, ref_resize_u8(lib, *g)), g
        assert test_flow_ref.digest(ours) == want, g


def test_geometries_are_those_of_the_cases():
    """every luma / chroma geometry of the GPU cases whose grid does not cover the frame is among the pinned ones"""
    have = set(GEOMETRIES)
    for c in mc.CASES + mc.FULL_CASES:
        fmt, w, h, _, _, akw, _, _, _, claims = c
        if "edgex" not in claims and "edgey" not in claims or akw.get("blksizev"):
            continue
        bs, ov = akw["blksize"], akw["overlap"]
        nbx, nby = (w - ov) // (bs - ov), (h - ov) // (bs - ov)
        wb, hb = nbx * (bs - ov) + ov, nby * (bs - ov) + ov
        sub = mc.FORMATS[fmt].get("subsampling", (0, 0))
        assert (nbx, nby, wb, hb) in have and (nbx, nby, wb >> sub[0], hb >> sub[1]) in have, c


# ---------------------------------------------------------------- the GPU cases: what they cover and the condition on their inputs

def test_cases_cover_what_the_feature_has():
    cases = mc.CASES + mc.FULL_CASES
    mk = [c[6] for c in cases]
    assert {k["kind"] for k in mk} == set(range(6))
    for kind in (0, 1, 2):
        assert {k.get("gamma", 1.0) for k in mk if k["kind"] == kind} >= {1.0, 0.5, 2.0, 0.0, 0.7}
    assert {k.get("ml", 100.0) for k in mk} >= {100.0, 3.0, 1000.0}
    assert {k.get("time", 100.0) for k in mk if k["kind"] in (1, 2)} >= {0.0, 37.5, 100.0}
    assert {(k["kind"], c[5]["isb"]) for c, k in zip(cases, mk)} >= {(kind, isb) for kind in range(6) for isb in (0, 1)}
    assert {k.get("ysc", 0) for k in mk} == {0, 200}
    assert {c[4].get("pel", 2) for c in cases} == {1, 2, 4}
    blocks = {(c[5]["blksize"], c[5].get("blksizev", c[5]["blksize"]), c[5]["overlap"], c[5].get("overlapv", c[5]["overlap"])) for c in cases}
    assert blocks >= {(8, 8, 4, 4), (16, 16, 8, 8), (8, 8, 0, 0), (16, 8, 4, 2)}
    assert {(c[1], c[2]) for c in cases} >= {(128, 96), (206, 118), (1920, 1080)}
    assert {c[0] for c in cases} == {"420", "422", "444", "gray"}
    assert any(c[3] == 16 and c[6]["kind"] == 1 for c in cases)
    assert any(c[6].get("thscd1") == 20 and c[6].get("thscd2") == 10 for c in cases)
    recipes = {(c[7].name, c[6]["kind"], c[6].get("gamma", 1.0)) for c in cases if c[7] is not None}
    assert {r[0] for r in recipes} == {"limits", "sad_edges", "occlusion", "scene_count", "invalid"}
    assert ("sad_edges", 1, 1.0) in recipes and ("occlusion", 2, 1.0) in recipes and ("occlusion", 2, 2.0) in recipes
    assert set(k for c in cases for k in c[-1].split(",")) == {"moved", "back", "cut", "span", "edgex", "edgey", "sc", "trunc"}


@pytest.mark.parametrize("case", mc.CASES + mc.FULL_CASES, ids=mc.ids(mc.CASES + mc.FULL_CASES))
def test_gpu_case_inputs_keep_pow_away_from_integers(oracle, case):
    """the condition of tests/mask_cases.py on every GPU case, through the oracle's vectors: no 255 * pow(...) whose byte another pow could
    change lies within POW_MARGIN of the integer it must not cross; and the case reaches the branches it claims"""
    ad, blobs = mc.oracle_vectors(oracle, case)
    _, lumas = mc.frames_of(case)
    _, kinds, dist = mc.expected(case, ad, blobs, lumas)
    print("pow distance %.3g" % dist)
    assert dist >= mc.POW_MARGIN
    assert kinds == case[-1]
