"""CPU tests of the creation of mv.Degrain, mv.Compensate, mv.BlockFPS and of mv.SCDetection's argument check (none of them touches a
device before its checks are through): the reference's messages (MVDegrains.cpp:511-730, MVCompensate.c:457-541, MVBlockFPS.c:780-926,
MVSCDetection.c:105-121, MVAnalysisData.c:7-31,68-98) and the order in which this library runs the checks, BlockFPS's output frame
count, rate and frame mapping against tests/flow_ref.py (FlowFPS shares that arithmetic, MVBlockFPS.c:245-254,278-292,888-909).

Where the order differs from the reference's it is the library's, pinned here so that it cannot move unnoticed: the thscd1 limit is
reported before a mismatch of the two vector clips (the reference lets the mismatch overwrite it), BlockFPS reports the FIRST mismatching
field (adataCheckSimilarity the last) and does not compare subsampling or bit depth, and Compensate checks `fields` after the frame size.
The radius, 3x3-block and U/V-pitch messages are the library's own."""
import ctypes as C

import pytest

import flow_ref

INT_MAX = 2147483647


def _clips(mv, w=320, h=192, bits=8, sup_kw=None, **akw):
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


def _split_uv_pitch(sup):
    """the same super clip, described with a V pitch that differs from the U pitch"""
    sup.pitch = [sup.pitch[0], sup.pitch[1], sup.pitch[1] + 256]
    return sup


def _scaled_thscd1(ad, thscd1):
    """MVAnalysisData.c:20-28 scaleThSCD, thscd1 only"""
    s = thscd1 * (ad.nBlkSizeX * ad.nBlkSizeY) // 64
    if ad.nMotionFlags & 8:  # MOTION_USE_CHROMA_MOTION
        s += s // (ad.xRatioUV * ad.yRatioUV) * 2
    return int(float(s) * ((1 << ad.bitsPerSample) - 1) / 255.0 + 0.5)


PITCH = [320, 160, 160]


def _degrain(mv, sup, ad, radius=1, **kw):
    return mv.Degrain(radius, sup, ad, PITCH, **kw)


def _bfps(mv, sup, bw, fw, fps=(24, 1), **kw):
    return mv.BlockFPS(sup, bw, fw, 10, PITCH, fps[0], fps[1], **kw)


def test_degrain_argument_checks(mv):
    sup, bw, _ = _clips(mv)
    assert _err(lambda: _degrain(mv, sup, bw, radius=0)) == "Degrain: radius must be between 1 and 6."
    assert _err(lambda: _degrain(mv, sup, bw, radius=7, plane=9)) == "Degrain: radius must be between 1 and 6."
    assert _err(lambda: _degrain(mv, sup, bw, plane=5)) == "Degrain1: plane must be between 0 and 4 (inclusive)."
    assert _err(lambda: _degrain(mv, sup, bw, radius=3, plane=-1, thscd1=99999)) == "Degrain3: plane must be between 0 and 4 (inclusive)."
    assert _err(lambda: _degrain(mv, sup, bw, radius=2, thscd1=16321)) == "Degrain2: thscd1 can be at most 16320."
    _degrain(mv, sup, bw, thscd1=16320)
    # thscd1 before the thsad overflow, the overflow before the frame size, the size before the limits
    assert _err(lambda: _degrain(mv, sup, bw, thscd1=16321, thsad=1 << 40)) == "Degrain1: thscd1 can be at most 16320."
    sup2 = mv.Super(336, 192, 8)
    assert _err(lambda: _degrain(mv, sup2, bw)) == "Degrain1: wrong source or super clip frame size."
    assert _err(lambda: _degrain(mv, sup2, bw, thsad=1 << 40)).startswith("Degrain1: with this block size and video format, thsad must")
    assert _err(lambda: _degrain(mv, sup2, bw, limit=256)) == "Degrain1: wrong source or super clip frame size."
    assert _err(lambda: _degrain(mv, mv.Super(320, 192, 8, pel=4), bw)) == "Degrain1: wrong source or super clip frame size."
    assert _err(lambda: _degrain(mv, mv.Super(320, 200, 8), bw)) == "Degrain1: wrong source or super clip frame size."
    assert _err(lambda: _degrain(mv, sup, bw, radius=6, limit=256)) == "Degrain6: limit must be between 0 and 255 (inclusive)."
    assert _err(lambda: _degrain(mv, sup, bw, limit=-1, limitc=999)) == "Degrain1: limit must be between 0 and 255 (inclusive)."
    assert _err(lambda: _degrain(mv, sup, bw, limitc=256)) == "Degrain1: limitc must be between 0 and 255 (inclusive)."
    assert _err(lambda: _degrain(mv, sup, bw, limitc=-1)) == "Degrain1: limitc must be between 0 and 255 (inclusive)."
    _degrain(mv, sup, bw, limit=255, limitc=0)
    sup16, bw16, _ = _clips(mv, bits=16)
    assert _err(lambda: mv.Degrain(1, sup16, bw16, [640, 320, 320], limit=65536)) == "Degrain1: limit must be between 0 and 65535 (inclusive)."
    # the library's own checks come last
    supo, bwo, _ = _clips(mv, overlap=4)
    assert _err(lambda: _degrain(mv, supo, _copy(mv, bwo, nBlkX=2))) == "overlap needs at least 3x3 blocks (window selection divides by nBlk-2)."
    assert _err(lambda: _degrain(mv, supo, _copy(mv, bwo, nBlkY=2), limitc=256)) == "Degrain1: limitc must be between 0 and 255 (inclusive)."
    assert _err(lambda: _degrain(mv, _split_uv_pitch(mv.Super(320, 192, 8)), bw)) == "U and V super planes must share one pitch."
    assert _err(lambda: _degrain(mv, _split_uv_pitch(mv.Super(320, 192, 8)), _copy(mv, bwo, nBlkX=2))) == \
        "overlap needs at least 3x3 blocks (window selection divides by nBlk-2)."


@pytest.mark.parametrize("bits,thscd1", [(16, None), (16, 200), (16, 16320), (10, 37)])
def test_degrain_thsad_overflow_reports_the_limit_from_the_unscaled_thscd1(mv, bits, thscd1):
    """MVDegrains.cpp:658-666: thsad is scaled by nSCD1 / nSCD1_old, and the message's maximum is INT_MAX * nSCD1_old / nSCD1"""
    sup, bw, _ = _clips(mv, bits=bits, blksize=16)
    old = 400 if thscd1 is None else thscd1
    new = _scaled_thscd1(bw, old)
    assert new != old
    maximum = INT_MAX * old // new
    pitch = [640, 320, 320]
    msg = "Degrain2: with this block size and video format, thsad%s must not exceed %d or some calculations would overflow."
    over = maximum + 2  # (thsad * new / old truncates: maximum + 1 may still scale to INT_MAX - 1)
    assert over * new // old >= INT_MAX
    assert _err(lambda: mv.Degrain(2, sup, bw, pitch, thsad=over, thscd1=thscd1)) == msg % ("", maximum)
    assert _err(lambda: mv.Degrain(2, sup, bw, pitch, thsad=400, thsadc=over, thscd1=thscd1)) == msg % ("c", maximum)
    assert _err(lambda: mv.Degrain(2, sup, bw, pitch, thsad=over, thsadc=over, thscd1=thscd1)) == msg % ("", maximum)
    ok = maximum - 1
    assert ok * new // old < INT_MAX
    mv.Degrain(2, sup, bw, pitch, thsad=ok, thsadc=ok, thscd1=thscd1)


def test_compensate_argument_checks(mv):
    sup, bw, _ = _clips(mv)
    comp = lambda s, ad, **kw: mv.Compensate(s, ad, **kw)
    assert _err(lambda: comp(sup, bw, time=-0.5)) == "Compensate: time must be between 0.0 and 100.0 (inclusive)."
    assert _err(lambda: comp(sup, bw, time=100.5, thscd1=99999)) == "Compensate: time must be between 0.0 and 100.0 (inclusive)."
    assert _err(lambda: comp(sup, bw, thscd1=16321)) == "Compensate: thscd1 can be at most 16320."
    comp(sup, bw, thscd1=16320, time=0.0)
    comp(sup, bw, time=100.0, fields=1)
    sup2 = mv.Super(336, 192, 8)
    assert _err(lambda: comp(sup2, bw)) == "Compensate: wrong source or super clip frame size."
    assert _err(lambda: comp(sup2, bw, thscd1=16321)) == "Compensate: thscd1 can be at most 16320."
    assert _err(lambda: comp(mv.Super(320, 192, 8, pel=1), bw)) == "Compensate: wrong source or super clip frame size."
    sup1, bw1, _ = _clips(mv, sup_kw=dict(pel=1))
    assert _err(lambda: comp(sup1, bw1, fields=1)) == "Compensate: fields option requires pel > 1."
    comp(sup1, bw1, fields=0)
    assert _err(lambda: comp(sup, bw1, fields=1)) == "Compensate: wrong source or super clip frame size."  # the size check comes first
    supo, bwo, _ = _clips(mv, overlap=4)
    assert _err(lambda: comp(supo, _copy(mv, bwo, nBlkY=2))) == "overlap needs at least 3x3 blocks (window selection divides by nBlk-2)."
    assert _err(lambda: comp(_split_uv_pitch(mv.Super(320, 192, 8)), bw)) == "U and V super planes must share one pitch."
    assert _err(lambda: comp(_split_uv_pitch(mv.Super(320, 192, 8, pel=1)), bw1, fields=1)) == "Compensate: fields option requires pel > 1."


def test_blockfps_argument_checks(mv):
    sup, bw, fw = _clips(mv)
    assert _err(lambda: _bfps(mv, sup, bw, fw, mode=9)) == "BlockFPS: mode must be between 0 and 8 (inclusive)."
    assert _err(lambda: _bfps(mv, sup, bw, fw, mode=-1, thscd1=99999)) == "BlockFPS: mode must be between 0 and 8 (inclusive)."
    assert _err(lambda: _bfps(mv, sup, bw, fw, thscd1=16321)) == "BlockFPS: thscd1 can be at most 16320."
    _bfps(mv, sup, bw, fw, thscd1=16320, mode=8)
    assert _err(lambda: _bfps(mv, sup, bw, _copy(mv, fw, nWidth=336), thscd1=16321)) == "BlockFPS: thscd1 can be at most 16320."
    assert _err(lambda: _bfps(mv, sup, bw, _copy(mv, fw, nWidth=336))) == "BlockFPS: mvbw and mvfw have different widths."
    assert _err(lambda: _bfps(mv, sup, bw, _copy(mv, fw, nHeight=200))) == "BlockFPS: mvbw and mvfw have different heights."
    assert _err(lambda: _bfps(mv, sup, bw, _copy(mv, fw, nBlkSizeX=16))) == "BlockFPS: mvbw and mvfw have different block sizes."
    assert _err(lambda: _bfps(mv, sup, bw, _copy(mv, fw, nBlkSizeY=16))) == "BlockFPS: mvbw and mvfw have different block sizes."
    assert _err(lambda: _bfps(mv, sup, bw, _copy(mv, fw, nPel=4))) == "BlockFPS: mvbw and mvfw have different pel precision."
    assert _err(lambda: _bfps(mv, sup, bw, _copy(mv, fw, nOverlapX=2))) == "BlockFPS: mvbw and mvfw have different overlap."
    assert _err(lambda: _bfps(mv, sup, bw, _copy(mv, fw, nOverlapY=2))) == "BlockFPS: mvbw and mvfw have different overlap."
    # the FIRST mismatching field is reported
    assert _err(lambda: _bfps(mv, sup, bw, _copy(mv, fw, nWidth=336, nPel=4))) == "BlockFPS: mvbw and mvfw have different widths."
    assert _err(lambda: _bfps(mv, sup, bw, _copy(mv, fw, nHeight=200, nOverlapX=2))) == "BlockFPS: mvbw and mvfw have different heights."
    assert _err(lambda: _bfps(mv, sup, bw, _copy(mv, fw, nPel=4, nDeltaFrame=0))) == "BlockFPS: mvbw and mvfw have different pel precision."
    # subsampling and bit depth are not compared
    _bfps(mv, sup, bw, _copy(mv, fw, xRatioUV=1, yRatioUV=1, bitsPerSample=16))
    assert _err(lambda: _bfps(mv, sup, _copy(mv, bw, nDeltaFrame=0), _copy(mv, fw, nDeltaFrame=0))) == \
        "BlockFPS: cannot use motion vectors with absolute frame references."
    assert _err(lambda: _bfps(mv, sup, bw, _copy(mv, fw, nDeltaFrame=-3))) == "BlockFPS: cannot use motion vectors with absolute frame references."
    assert _err(lambda: _bfps(mv, sup, bw, _copy(mv, fw, nDeltaFrame=2))) == "BlockFPS: mvbw and mvfw must be generated with the same delta."
    assert _err(lambda: _bfps(mv, sup, fw, _copy(mv, fw, nDeltaFrame=2))) == "BlockFPS: mvbw and mvfw must be generated with the same delta."
    assert _err(lambda: _bfps(mv, sup, fw, fw)) == "BlockFPS: mvbw must be generated with isb=True."
    assert _err(lambda: _bfps(mv, sup, fw, bw)) == "BlockFPS: mvbw must be generated with isb=True."
    assert _err(lambda: _bfps(mv, sup, bw, bw)) == "BlockFPS: mvfw must be generated with isb=False."
    assert _err(lambda: _bfps(mv, sup, bw, bw, fps=(0, 1))) == "BlockFPS: mvfw must be generated with isb=False."
    assert _err(lambda: _bfps(mv, sup, bw, fw, fps=(0, 1))) == "BlockFPS: The input clip must have a frame rate. Invoke AssumeFPS if necessary."
    assert _err(lambda: _bfps(mv, sup, bw, fw, fps=(24, 0))) == "BlockFPS: The input clip must have a frame rate. Invoke AssumeFPS if necessary."
    sup2 = mv.Super(336, 192, 8)
    assert _err(lambda: _bfps(mv, sup2, bw, fw)) == "BlockFPS: wrong source or super clip frame size."
    assert _err(lambda: _bfps(mv, sup2, bw, fw, fps=(0, 1))) == "BlockFPS: The input clip must have a frame rate. Invoke AssumeFPS if necessary."
    assert _err(lambda: _bfps(mv, mv.Super(320, 192, 8, pel=4), bw, fw)) == "BlockFPS: wrong source or super clip frame size."
    assert _err(lambda: _bfps(mv, mv.Super(320, 200, 8), bw, fw)) == "BlockFPS: wrong source or super clip frame size."
    supo, bwo, fwo = _clips(mv, overlap=4)
    assert _err(lambda: _bfps(mv, supo, _copy(mv, bwo, nBlkX=2), fwo)) == "overlap needs at least 3x3 blocks (window selection divides by nBlk-2)."
    assert _err(lambda: _bfps(mv, _split_uv_pitch(mv.Super(320, 192, 8)), bw, fw)) == "U and V super planes must share one pitch."
    assert _err(lambda: _bfps(mv, _split_uv_pitch(mv.Super(336, 192, 8)), bw, fw)) == "BlockFPS: wrong source or super clip frame size."


@pytest.mark.parametrize("num,den,fps,delta", [(48, 1, (24, 1), 1), (60, 1, (24, 1), 1), (60000, 1001, (24000, 1001), 1), (0, 0, (25, 1), 1),
                                               (None, None, (30, 1), 1), (50, 1, (24, 1), 2), (30, 1, (60, 1), 1)])
def test_blockfps_frames_rate_and_map(mv, num, den, fps, delta):
    sup, bw, fw = _clips(mv, delta=delta)
    g = _bfps(mv, sup, bw, fw, fps=fps, num=num, den=den)
    ref = flow_ref.Flow(bw, fw, 10, 3, 16, 16, fps=fps, num=num, den=den)
    assert (g.num_frames, g.fps_num, g.fps_den) == (ref.num_frames,) + ref.fps
    info = mv.BlockFPSInfo()
    mv.lib().mvx_blockfps_get_info(g.h, C.byref(info))
    assert (info.num_frames, info.fps_num, info.fps_den) == (ref.num_frames,) + ref.fps
    for n in range(g.num_frames + 3):
        assert g.map(n) == ref.map(n), n


def test_blockfps_negative_rate_gives_no_output_rate(mv):
    """setFPS, MVBlockFPS.c:703-718: a non-positive numerator or denominator leaves the output clip without a frame rate (0 / 1)"""
    sup, bw, fw = _clips(mv)
    g = _bfps(mv, sup, bw, fw, num=-50, den=1)
    assert (g.fps_num, g.fps_den) == (0, 1)


def test_scdetect_argument_check(mv):
    """MVSCDetection.c:113 -> scaleThSCD's limit; checked before any device call, and only when there is a blob to judge"""
    _, bw, _ = _clips(mv)
    L = mv.lib()
    ad = mv.AnalysisData.from_buffer_copy(bytes(bw))
    blobs, out, err = (C.c_void_p * 1)(), (C.c_int32 * 1)(7), C.create_string_buffer(mv.ERRLEN)
    assert L.mvx_scdetect(C.byref(ad), 16321, mv.UNSET, 1, blobs, out, None, err) != 0
    assert err.value.decode() == "SCDetection: thscd1 can be at most 16320."
    assert L.mvx_last_error().decode() == "SCDetection: thscd1 can be at most 16320."
    assert out[0] == 7
    assert L.mvx_scdetect(C.byref(ad), 1 << 40, 5, 1, blobs, out, None, None) != 0   # err may be NULL
    assert L.mvx_last_error().decode() == "SCDetection: thscd1 can be at most 16320."
    assert L.mvx_scdetect(C.byref(ad), 16321, mv.UNSET, 0, blobs, out, None, err) == 0
    assert err.value == b""


# ------------------------------------------------------------------------------------------------ plane layouts (include/mvtools_amd.h, "Plane layouts")

def _pitch_msg(what, plane, row):
    return "%s pitch of plane %d must hold a row of %d bytes and be a multiple of the sample size." % (what, plane, row)


def _super_msg(plane, row, name=""):
    return "%ssuper pitch of plane %d must hold a row of %d bytes and be a multiple of 16 bytes." % (name, plane, row)


def _with_pitch(sup, pitch):
    sup.pitch = list(pitch)
    return sup


def test_clip_side_pitches_the_legal_edges_and_the_refusals(mv):
    """320 x 192, 4:2:0: rows of 320 / 160 / 160 samples.  Legal: a tight pitch, one sample more than a row (odd at 8 bits, 2 mod 4 at 16), U
    and V of different pitch, src and dst of different pitch.  Refused: a pitch shorter than a row, a pitch that is no multiple of the sample."""
    sup, bw, fw = _clips(mv)
    sup16, bw16, fw16 = _clips(mv, bits=16)
    for src, dst in (([320, 160, 160], None), ([321, 161, 161], [320, 160, 160]), ([512, 256, 512], [320, 160, 416]), ([320, 160, 160], [1024, 161, 160])):
        mv.Degrain(1, sup, bw, src, dst)
        mv.DegrainN(7, sup, bw, src, dst)
        mv.BlockFPS(sup, bw, fw, 10, src, dst_pitch=dst)
        mv.Compensate(sup, bw, dst or src)
        mv.CompensateN(2, sup, bw, dst or src)
    mv.Degrain(1, sup16, bw16, [642, 322, 322], [640, 320, 324])           # 16 bit: 2 mod 4
    mv.DegrainN(2, sup, bw, [320, 160, 160], [640, 322, 320], out16=True)  # out16: the dst rows are 16-bit samples
    for make in (lambda s, d: mv.Degrain(1, sup, bw, s, d), lambda s, d: mv.DegrainN(3, sup, bw, s, d)):
        assert _err(lambda: make([319, 160, 160], [320, 160, 160])) == _pitch_msg("src", 0, 320)
        assert _err(lambda: make([320, 160, 159], [320, 160, 160])) == _pitch_msg("src", 2, 160)
        assert _err(lambda: make([320, 160, 160], [320, 100, 160])) == _pitch_msg("dst", 1, 160)
        assert _err(lambda: make([0, 160, 160], [320, 160, 160])) == _pitch_msg("src", 0, 320)
        assert _err(lambda: make([-320, 160, 160], [320, 160, 160])) == _pitch_msg("src", 0, 320)
    assert _err(lambda: mv.Degrain(1, sup16, bw16, [641, 320, 320])) == _pitch_msg("src", 0, 640)      # odd for 16-bit samples
    assert _err(lambda: mv.Degrain(1, sup16, bw16, [640, 320, 320], [640, 321, 320])) == _pitch_msg("dst", 1, 320)
    assert _err(lambda: mv.Degrain(1, sup16, bw16, [320, 320, 320])) == _pitch_msg("src", 0, 640)      # an 8-bit row's pitch
    assert _err(lambda: mv.DegrainN(2, sup, bw, [320, 160, 160], [320, 160, 160], out16=True)) == _pitch_msg("dst", 0, 640)
    assert _err(lambda: mv.DegrainN(2, sup, bw, [320, 160, 160], [640, 321, 320], out16=True)) == _pitch_msg("dst", 1, 320)
    assert _err(lambda: mv.Compensate(sup, bw, [320, 159, 160])) == _pitch_msg("dst", 1, 160)
    assert _err(lambda: mv.CompensateN(1, sup16, bw16, [640, 320, 323])) == _pitch_msg("dst", 2, 320)
    assert _err(lambda: mv.BlockFPS(sup, bw, fw, 10, [320, 160, 100])) == _pitch_msg("clip", 2, 160)
    assert _err(lambda: mv.BlockFPS(sup, bw, fw, 10, [320, 160, 160], dst_pitch=[300, 160, 160])) == _pitch_msg("dst", 0, 320)
    # after the filter's own checks and the two older checks of the library
    assert _err(lambda: mv.Degrain(1, sup, bw, [1, 1, 1], limit=999)) == "Degrain1: limit must be between 0 and 255 (inclusive)."
    assert _err(lambda: mv.Degrain(1, _split_uv_pitch(mv.Super(320, 192, 8)), bw, [1, 1, 1])) == "U and V super planes must share one pitch."


def test_super_pitches_what_mvx_super_frames_writes(mv):
    """the consumers and the search take super planes as mvx_super_frames writes them: a pitch that holds a row and is a multiple of 16"""
    sup, bw, fw = _clips(mv)
    row = [sup.info.plane_width[p] for p in range(3)]
    ok = [(r + 15) // 16 * 16 + 16 for r in row]
    for pitch in (ok, [(r + 15) // 16 * 16 for r in row]):
        s = _with_pitch(mv.Super(320, 192, 8), pitch)
        mv.Analyse(s, isb=1)
        mv.Recalculate(s, bw, blksize=8)
        mv.Degrain(1, s, bw, PITCH)
        mv.Compensate(s, bw, PITCH)
        mv.BlockFPS(s, bw, fw, 10, PITCH)
    bad8, short = [ok[0] + 8, ok[1], ok[2]], [ok[0], row[1] // 16 * 16 - 16, row[1] // 16 * 16 - 16]
    assert _err(lambda: mv.Analyse(_with_pitch(mv.Super(320, 192, 8), bad8))) == _super_msg(0, row[0], "Analyse: ")
    assert _err(lambda: mv.Analyse(_with_pitch(mv.Super(320, 192, 8), short))) == _super_msg(1, row[1], "Analyse: ")
    assert _err(lambda: mv.Recalculate(_with_pitch(mv.Super(320, 192, 8), bad8), bw, blksize=8)) == _super_msg(0, row[0], "Recalculate: ")
    assert _err(lambda: mv.Degrain(1, _with_pitch(mv.Super(320, 192, 8), bad8), bw, PITCH)) == _super_msg(0, row[0])
    assert _err(lambda: mv.DegrainN(9, _with_pitch(mv.Super(320, 192, 8), short), bw, PITCH)) == _super_msg(1, row[1])
    assert _err(lambda: mv.Compensate(_with_pitch(mv.Super(320, 192, 8), bad8), bw, PITCH)) == _super_msg(0, row[0])
    assert _err(lambda: mv.BlockFPS(_with_pitch(mv.Super(320, 192, 8), short), bw, fw, 10, PITCH)) == _super_msg(1, row[1])
    with pytest.raises(ValueError):
        mv.Super(320, 192, 8, pitch=bad8)
    assert mv.Super(320, 192, 8, pitch=ok).pitch == ok and mv.Super(320, 192, 8).pitch == [(r + 255) // 256 * 256 for r in row]


def test_plane_addresses_are_checked_before_anything_is_launched(mv):
    """*_frames refuses a missing plane and an address that is no multiple of the sample size (clip side) or of 16 (super side) with
    MVX_E_ARG before it touches a device: this runs without one"""
    L = mv.lib()
    sup16, bw16, fw16 = _clips(mv, bits=16)
    A = 0x10000  # never dereferenced

    def refused(call, msg):
        assert call() == -1 and L.mvx_last_error().decode() == msg

    dg = mv.Degrain(1, sup16, bw16, [640, 320, 320])
    job = (mv.DegrainJob * 1)()

    def fill(src=(A, A, A), dst=(A, A, A), ref=(A, A, A)):
        for p in range(3):
            job[0].src[p], job[0].dst[p], job[0].refs[0][p], job[0].refs[1][p] = src[p], dst[p], ref[p], None
        return lambda: L.mvx_degrain_frames(dg.h, 1, job, None)
    refused(fill(src=(A + 1, A, A)), "mvx_degrain_frames: src plane 0 must be aligned to 2 bytes")
    refused(fill(src=(A, A, None)), "mvx_degrain_frames: src plane 2 is required")
    refused(fill(dst=(A, A + 3, A)), "mvx_degrain_frames: dst plane 1 must be aligned to 2 bytes")
    refused(fill(dst=(None, A, A)), "mvx_degrain_frames: dst plane 0 is required")
    refused(fill(ref=(A + 8, A, A)), "mvx_degrain_frames: reference super plane 0 must be aligned to 16 bytes")

    comp = mv.Compensate(sup16, bw16, [640, 320, 320])
    cj = (mv.CompensateJob * 1)()

    def cfill(src=(A, A, A), dst=(A, A, A)):
        for p in range(3):
            cj[0].src_super[p], cj[0].dst[p], cj[0].ref_super[p] = src[p], dst[p], None
        return lambda: L.mvx_compensate_frames(comp.h, 1, cj, None)
    refused(cfill(src=(A, A + 4, A)), "mvx_compensate_frames: source super plane 1 must be aligned to 16 bytes")
    refused(cfill(src=(None, A, A)), "mvx_compensate_frames: source super plane 0 is required")
    refused(cfill(dst=(A, A, A + 1)), "mvx_compensate_frames: dst plane 2 must be aligned to 2 bytes")

    bf = mv.BlockFPS(sup16, bw16, fw16, 10, [640, 320, 320])
    bj = (mv.BlockFPSJob * 1)()

    def bfill(left=(A, A, A), dst=(A, A, A)):
        bj[0].time256 = 0
        for p in range(3):
            bj[0].clip_left[p], bj[0].dst[p] = left[p], dst[p]
        return lambda: L.mvx_blockfps_frames(bf.h, 1, bj, None)
    refused(bfill(left=(None, A, A)), "mvx_blockfps_frames: clip_left / clip_right are required")
    refused(bfill(left=(A, A + 1, A)), "mvx_blockfps_frames: clip_left plane 1 must be aligned to 2 bytes")
    refused(bfill(dst=(A, A, None)), "mvx_blockfps_frames: dst plane 2 is required")
    # an 8-bit clip has no alignment to miss: the same odd addresses pass these checks (and then need a device)
    sup, bw, _ = _clips(mv)
    c8 = mv.Compensate(sup, bw, PITCH)
    for p in range(3):
        cj[0].src_super[p], cj[0].dst[p] = A, None
    refused(lambda: L.mvx_compensate_frames(c8.h, 1, cj, None), "mvx_compensate_frames: dst plane 0 is required")


def test_compensate_frames_limits_the_jobs_of_a_call_before_it_looks_at_one(mv):
    """The output kernel's grid holds (job, chroma plane) in z, 65535 at most: an integer handle refuses 32768 jobs with MVX_E_ARG before it
    looks at any of them (these are all zero: no plane, no blob) or at a device; a call of no jobs is a no-op"""
    L = mv.lib()
    sup, bw, _ = _clips(mv)
    comp = mv.Compensate(sup, bw, PITCH)
    many = (mv.CompensateJob * 32768)()
    assert L.mvx_compensate_frames(comp.h, 32768, many, None) == -1
    assert L.mvx_last_error().decode() == "mvx_compensate_frames: at most 32767 jobs per call"
    assert L.mvx_compensate_frames(comp.h, 32767, many, None) == -1  # inside the limit the jobs are looked at
    assert L.mvx_last_error().decode() == "mvx_compensate_frames: source super plane 0 is required"
    assert L.mvx_compensate_frames(comp.h, 0, many, None) == 0
    assert L.mvx_compensate_frames(comp.h, 0, None, None) == 0


def test_finest_layouts_are_checked_before_anything_is_launched(mv):
    """mvx_finest_frames: pitches that hold a row, planes that are there, all multiples of the sample size; U and V may differ"""
    L = mv.lib()
    sup = mv.Super(320, 192, 16)
    w, h = C.c_int32(), C.c_int32()
    L.mvx_finest_size(sup.h, C.byref(w), C.byref(h))
    rows = [w.value * 2, w.value, w.value]
    A = 0x10000  # never dereferenced
    three = lambda l: (C.c_ssize_t * 3)(*l)
    ptrs = lambda l: (C.c_void_p * 3)(*l)

    def call(src=(A, A, A), dst=(A, A, A), spitch=None, dpitch=None):
        rc = L.mvx_finest_frames(sup.h, 1, ptrs(src), three(spitch or sup.pitch), ptrs(dst), three(dpitch or rows), None)
        return rc, L.mvx_last_error().decode()
    pitches = "mvx_finest_frames: pitches must hold a row of their plane and be multiples of the sample size"
    planes = "mvx_finest_frames: planes are required and must be aligned to the sample size"
    assert call(dpitch=[rows[0] - 2, rows[1], rows[2]]) == (-1, pitches)
    assert call(dpitch=[rows[0], rows[1] + 1, rows[2]]) == (-1, pitches)
    assert call(spitch=[sup.pitch[0], sup.pitch[1], 64]) == (-1, pitches)
    assert call(dst=(A, A + 1, A)) == (-1, planes)
    assert call(src=(A + 1, A, A)) == (-1, planes)
    assert call(dst=(A, A, None)) == (-1, planes)
    # legal: a tight pitch (rows), one sample more, U != V -- these pass the checks; a tight 16-bit row of 2 mod 4 bytes needs no more
    assert call(dst=(A, A, None), dpitch=[rows[0] + 2, rows[1], rows[2] + 256])[1] == planes
