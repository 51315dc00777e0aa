"""CPU tests of mv.FlowInter / mv.FlowFPS creation (mvx_flowinter_create / mvx_flowfps_create touch no device): the reference's checks
and messages in its order (MVFlowInter.c:506-652, MVFlowFPS.c:606-802, MVAnalysisData.c:7-31,68-98), output frame count, rate and
frame mapping against tests/flow_ref.py."""
import pytest

import flow_ref


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


def _inter(mv, sup, bw, fw, **kw):
    return mv.FlowInter(sup, bw, fw, 10, [320, 160, 160], **kw)


def _fps(mv, sup, bw, fw, fps=(24, 1), **kw):
    return mv.FlowFPS(sup, bw, fw, 10, [320, 160, 160], fps[0], fps[1], **kw)


def test_flowinter_argument_checks(mv):
    sup, bw, fw = _pair(mv)
    assert _err(lambda: _inter(mv, sup, bw, fw, time=-0.5)) == "FlowInter: time must be between 0 and 100 % (inclusive)."
    assert _err(lambda: _inter(mv, sup, bw, fw, time=100.5)) == "FlowInter: time must be between 0 and 100 % (inclusive)."
    assert _err(lambda: _inter(mv, sup, bw, fw, ml=0.0)) == "FlowInter: ml must be greater than 0."
    assert _err(lambda: _inter(mv, sup, bw, fw, time=200.0, ml=0.0)).startswith("FlowInter: time")   # time is checked first
    assert _err(lambda: _inter(mv, sup, bw, fw, thscd1=16321)) == "FlowInter: thscd1 can be at most 16320."
    _inter(mv, sup, bw, fw, thscd1=16320)
    # the similarity check: the LAST mismatching field's message wins
    assert _err(lambda: _inter(mv, sup, bw, _copy(mv, fw, nWidth=336))) == "FlowInter: mvbw and mvfw have different widths."
    assert _err(lambda: _inter(mv, sup, bw, _copy(mv, fw, nWidth=336, nPel=4))) == "FlowInter: mvbw and mvfw have different pel precision."
    assert _err(lambda: _inter(mv, sup, bw, _copy(mv, fw, nHeight=200, bitsPerSample=16))) == "FlowInter: mvbw and mvfw have different bit depths."
    assert _err(lambda: _inter(mv, sup, bw, _copy(mv, fw, xRatioUV=1, nOverlapX=2))) == "FlowInter: mvbw and mvfw have different horizontal subsampling."
    assert _err(lambda: _inter(mv, sup, bw, _copy(mv, fw, nWidth=336), thscd1=99999)) == "FlowInter: thscd1 can be at most 16320."
    assert _err(lambda: _inter(mv, sup, _copy(mv, bw, nDeltaFrame=0), _copy(mv, fw, nDeltaFrame=0))) == \
        "FlowInter: cannot use motion vectors with absolute frame references."
    assert _err(lambda: _inter(mv, sup, bw, _copy(mv, fw, nDeltaFrame=2))) == "FlowInter: mvbw and mvfw must be generated with the same delta."
    assert _err(lambda: _inter(mv, sup, fw, fw)) == "FlowInter: mvbw must be generated with isb=True."
    assert _err(lambda: _inter(mv, sup, bw, bw)) == "FlowInter: mvfw must be generated with isb=False."
    sup2 = mv.Super(336, 192, 8)
    assert _err(lambda: _inter(mv, sup2, bw, fw)) == "FlowInter: wrong source or super clip frame size."
    sup4 = mv.Super(320, 192, 8, pel=4)
    assert _err(lambda: _inter(mv, sup4, bw, fw)) == "FlowInter: wrong source or super clip frame size."


def test_flowfps_argument_checks(mv):
    sup, bw, fw = _pair(mv)
    assert _err(lambda: _fps(mv, sup, bw, fw, mask=3)) == "FlowFPS: mask must be 0, 1, or 2."
    assert _err(lambda: _fps(mv, sup, bw, fw, mask=-1, ml=-1.0)) == "FlowFPS: mask must be 0, 1, or 2."
    assert _err(lambda: _fps(mv, sup, bw, fw, ml=0.0)) == "FlowFPS: ml must be greater than 0."
    assert _err(lambda: _fps(mv, sup, bw, fw, thscd1=20000)) == "FlowFPS: thscd1 can be at most 16320."
    assert _err(lambda: _fps(mv, sup, bw, _copy(mv, fw, nBlkSizeX=16, nOverlapY=2))) == "FlowFPS: mvbw and mvfw have different overlap."
    # the one deliberate divergence: the reference accepts these and then reads negative frame numbers
    assert _err(lambda: _fps(mv, sup, _copy(mv, bw, nDeltaFrame=-1), _copy(mv, fw, nDeltaFrame=-1))) == \
        "FlowFPS: cannot use motion vectors with absolute frame references."
    assert _err(lambda: _fps(mv, sup, bw, _copy(mv, fw, nDeltaFrame=3))) == "FlowFPS: mvbw and mvfw must be generated with the same delta."
    assert _err(lambda: _fps(mv, sup, fw, fw)) == "FlowFPS: mvbw must be generated with isb=True."
    assert _err(lambda: _fps(mv, sup, bw, bw)) == "FlowFPS: mvfw must be generated with isb=False."
    assert _err(lambda: _fps(mv, sup, bw, fw, fps=(0, 1))) == "FlowFPS: The input clip must have a frame rate. Invoke AssumeFPS if necessary."
    assert _err(lambda: _fps(mv, mv.Super(336, 192, 8), bw, fw)) == "FlowFPS: inconsistent source and vector frame size."
    assert _err(lambda: _fps(mv, mv.Super(320, 192, 8, pel=1), bw, fw)) == "FlowFPS: wrong source or super clip frame size."
    assert _err(lambda: _fps(mv, sup, _copy(mv, bw, nHPadding=8), fw)) == \
        "FlowFPS: inconsistent clips frame size! Incomprehensible error messages are the best, right?"


@pytest.mark.parametrize("num,den,fps,delta", [(48, 1, (24, 1), 1), (60, 1, (24, 1), 1), (60000, 1001, (24000, 1001), 1), (0, 0, (25, 1), 1),
                                               (None, None, (30, 1), 1), (50, 1, (24, 1), 2), (30, 1, (60, 1), 1)])
def test_flowfps_frames_rate_and_map(mv, num, den, fps, delta):
    sup, bw, fw = _pair(mv, delta=delta)
    g = _fps(mv, sup, bw, fw, fps=fps, num=num, den=den)
    ref = flow_ref.Flow(bw, fw, 10, 3, 16, 16, fps=fps, num=num, den=den)
    assert (g.num_frames, g.fps_num, g.fps_den) == (ref.num_frames,) + ref.fps
    for n in range(g.num_frames + 3):
        assert g.map(n) == ref.map(n), n


def test_flowinter_time256_is_formed_in_float(mv):
    sup, bw, fw = _pair(mv, delta=2)
    for time, want in [(0.39062499, 1), (50.0, 128), (0.0, 0), (100.0, 256), (33.3, 85), (99.9, 255)]:
        g = _inter(mv, sup, bw, fw, time=time)
        assert g.map(5) == (5, 7, want), time
        assert flow_ref.Flow(bw, fw, 10, 3, 16, 16, time=time).map(5) == (5, 7, want)
        assert g.num_frames == 10
    assert int(0.39062499 * 256.0 / 100.0) == 0  # the same argument in double would give time256 0
