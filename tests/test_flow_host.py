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


# ------------------------------------------------------------------------------------------------ plane layouts (include/mvtools_amd.h, "Plane layouts")

def _makers(mv, sup, bw, fw):
    return {"FlowInter": lambda c, d=None: mv.FlowInter(sup, bw, fw, 10, c, dst_pitch=d), "FlowFPS": lambda c, d=None: mv.FlowFPS(sup, bw, fw, 10, c, 24, 1, dst_pitch=d),
            "Flow": lambda c, d=None: mv.Flow(sup, bw, 10, c, dst_pitch=d), "FlowBlur": lambda c, d=None: mv.FlowBlur(sup, bw, fw, 10, c, dst_pitch=d)}


@pytest.mark.parametrize("name", ["FlowInter", "FlowFPS", "Flow", "FlowBlur"])
def test_flow_filters_plane_layouts_at_creation(mv, name):
    """the contract of the block filters (tests/test_block_host.py), with the filter's name in front as in every message of the flow filters"""
    sup, bw, fw = _pair(mv)
    make = _makers(mv, sup, bw, fw)[name]
    msg = lambda what, p, row: "%s: %s pitch of plane %d must hold a row of %d bytes and be a multiple of the sample size." % (name, what, p, row)
    make([320, 160, 160])                           # tight
    make([321, 161, 161], [320, 160, 160])          # one sample more than a row; clip and dst differ
    make([512, 256, 512], [320, 160, 416])          # U != V
    assert _err(lambda: make([319, 160, 160])) == msg("clip", 0, 320)
    assert _err(lambda: make([320, 160, 100])) == msg("clip", 2, 160)
    assert _err(lambda: make([320, 160, 160], [320, 159, 160])) == msg("dst", 1, 160)
    sup16, bw16, fw16 = _pair(mv, bits=16)
    make16 = _makers(mv, sup16, bw16, fw16)[name]
    make16([642, 322, 322], [640, 320, 324])        # 2 mod 4
    assert _err(lambda: make16([641, 320, 320])) == msg("clip", 0, 640)
    assert _err(lambda: make16([640, 320, 320], [640, 320, 321])) == msg("dst", 2, 320)
    row = sup.info.plane_width[0]
    s = mv.Super(320, 192, 8)
    s.pitch = [s.pitch[0] + 8, s.pitch[1], s.pitch[2]]
    assert _err(lambda: _makers(mv, s, bw, fw)[name]([320, 160, 160])) == \
        "%s: super pitch of plane 0 must hold a row of %d bytes and be a multiple of 16 bytes." % (name, row)


def test_flow_plane_addresses_are_checked_before_anything_is_launched(mv):
    L = mv.lib()
    sup16, bw16, fw16 = _pair(mv, bits=16)
    A = 0x10000  # never dereferenced
    g = mv.FlowInter(sup16, bw16, fw16, 10, [640, 320, 320])
    job = (mv.FlowJob * 1)()

    def fill(left=(A, A, A), right=(A, A, A), dst=(A, A, A), sup=(None, None, None)):
        job[0].time256 = 128
        for p in range(3):
            job[0].clip_left[p], job[0].clip_right[p], job[0].dst[p], job[0].super_left[p] = left[p], right[p], dst[p], sup[p]
        return L.mvx_flow_frames(g.h, 1, job, None), L.mvx_last_error().decode()
    assert fill(left=(None, A, A)) == (-1, "mvx_flow_frames: dst / clip_left / clip_right are required")
    assert fill(left=(A, None, A)) == (-1, "mvx_flow_frames: clip_left plane 1 is required")
    assert fill(left=(A + 1, A, A)) == (-1, "mvx_flow_frames: clip_left plane 0 must be aligned to 2 bytes")
    assert fill(right=(A, A, A + 1)) == (-1, "mvx_flow_frames: clip_right plane 2 must be aligned to 2 bytes")
    assert fill(dst=(A, A + 1, A)) == (-1, "mvx_flow_frames: dst plane 1 must be aligned to 2 bytes")
    assert fill(sup=(A + 2, A, A)) == (-1, "mvx_flow_frames: super_left plane 0 must be aligned to 16 bytes")
    fc = mv.Flow(sup16, bw16, 10, [640, 320, 320])
    cj = (mv.FlowCompJob * 1)()
    for p in range(3):
        cj[0].clip[p], cj[0].dst[p] = A, A + (1 if p == 2 else 0)
    assert L.mvx_flowcomp_frames(fc.h, 1, cj, None) == -1 and L.mvx_last_error().decode() == "mvx_flowcomp_frames: dst plane 2 must be aligned to 2 bytes"
    fb = mv.FlowBlur(sup16, bw16, fw16, 10, [640, 320, 320])
    bj = (mv.FlowBlurJob * 1)()
    for p in range(3):
        bj[0].clip[p], bj[0].dst[p] = A + (1 if p == 0 else 0), A
    assert L.mvx_flowblur_frames(fb.h, 1, bj, None) == -1 and L.mvx_last_error().decode() == "mvx_flowblur_frames: clip plane 0 must be aligned to 2 bytes"
