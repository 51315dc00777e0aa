"""CPU tests of the float Flow / FlowBlur entries (mvx_flowcomp_create_float, mvx_flowblur_create_float; no create touches a device and *_frames
checks its jobs before any launch): creation and every message in its order, the integer entries' unchanged refusal of a float super clip, the
float entries' refusal of an integer one, fields = 1, the pitch and alignment rules for 4-byte samples, the job checks of both *_frames, and
the package's sample_float keyword."""
import numpy as np

from test_block_host import _clips, _copy, _err, _split_uv_pitch

ROWS = [320 * 4, 160 * 4, 160 * 4]   # rows of 320 / 160 float samples
FPITCH = [1280, 768, 768]            # ... rounded up to 256 bytes


def _fsup(mv, w=320, h=192, **kw):
    return mv.Super(w, h, 32, sample_float=True, **kw)


def _flow(mv, sup, ad, pitch=FPITCH, **kw):
    return mv.Flow(sup, ad, 10, pitch, sample_float=True, **kw)


def _blur(mv, sup, bw, fw, pitch=FPITCH, **kw):
    return mv.FlowBlur(sup, bw, fw, 10, pitch, sample_float=True, **kw)


def test_flow_float_messages_and_their_order(mv):
    isup, bw, fw = _clips(mv)
    fsup = _fsup(mv)
    needs, size = "Flow: the float entry needs a float super clip.", "Flow: wrong source or super clip frame size."
    fields = "Flow: fields is not supported on float clips."
    assert _err(lambda: _flow(mv, fsup, bw, time=-0.5)) == "Flow: time must be between 0 and 100 % (inclusive)."
    assert _err(lambda: _flow(mv, fsup, bw, time=100.5, mode=7)) == "Flow: time must be between 0 and 100 % (inclusive)."
    assert _err(lambda: _flow(mv, isup, bw, time=100.5)) == "Flow: time must be between 0 and 100 % (inclusive)."   # (before the kind of super clip)
    assert _err(lambda: _flow(mv, fsup, bw, mode=2)) == "Flow: mode must be 0 or 1."
    assert _err(lambda: _flow(mv, fsup, bw, mode=-1, thscd1=16321)) == "Flow: mode must be 0 or 1."
    assert _err(lambda: _flow(mv, fsup, bw, thscd1=16321)) == "Flow: thscd1 can be at most 16320."
    assert _err(lambda: _flow(mv, _fsup(mv, w=336), bw, thscd1=16321)) == "Flow: thscd1 can be at most 16320."
    _flow(mv, fsup, bw, thscd1=16320, time=0.0)
    _flow(mv, fsup, fw, mode=1)
    _flow(mv, fsup, _copy(mv, fw, nDeltaFrame=-3))                       # absolute references, either direction, any delta
    _flow(mv, fsup, _copy(mv, bw, nDeltaFrame=2), mode=1)
    assert _err(lambda: _flow(mv, _fsup(mv, w=336), bw)) == size
    assert _err(lambda: _flow(mv, _fsup(mv, pel=4), bw)) == size
    # an integer super clip handed to the float entry: after the frame size, before the geometry, the pitches and fields
    assert _err(lambda: _flow(mv, isup, bw)) == needs
    assert _err(lambda: _flow(mv, isup, bw, fields=1)) == needs
    assert _err(lambda: _flow(mv, isup, bw, pitch=[4, 4, 4])) == needs
    assert _err(lambda: _flow(mv, mv.Super(336, 192, 8), bw)) == size
    sup16, bw16, _ = _clips(mv, bits=16)
    assert _err(lambda: _flow(mv, sup16, bw16)) == needs
    _flow(mv, fsup, bw16)                                                # vectors of a 16-bit search
    tiny = _fsup(mv, w=8, h=64)
    tad = mv.Analyse(mv.Super(8, 64, 8), isb=1, blksize=8, overlap=0).ad
    assert _err(lambda: mv.Flow(tiny, tad, 10, [32, 16, 16], sample_float=True)) == "Flow: the frame must be at least two blocks wide and two blocks high."
    assert _err(lambda: mv.Flow(mv.Super(8, 64, 8), tad, 10, [32, 16, 16], sample_float=True)) == needs
    assert _err(lambda: _flow(mv, _split_uv_pitch(_fsup(mv)), bw)) == "Flow: U and V super planes must share one pitch."
    # fields = 1 is refused last
    assert _err(lambda: _flow(mv, fsup, bw, fields=1)) == fields
    assert _err(lambda: _flow(mv, fsup, bw, fields=1, mode=1)) == fields
    assert _err(lambda: _flow(mv, fsup, bw, fields=1, time=101.0)) == "Flow: time must be between 0 and 100 % (inclusive)."
    assert _err(lambda: _flow(mv, _fsup(mv, w=336), bw, fields=1)) == size
    assert _err(lambda: _flow(mv, fsup, bw, fields=1, pitch=[ROWS[0] - 4, ROWS[1], ROWS[2]])).startswith("Flow: clip pitch of plane 0 must hold a row of 1280 bytes")
    assert _err(lambda: _flow(mv, _split_uv_pitch(_fsup(mv)), bw, fields=1)) == "Flow: U and V super planes must share one pitch."
    _flow(mv, fsup, bw, fields=0)
    # the integer entry keeps its refusal, first of all, and still takes fields
    assert _err(lambda: mv.Flow(fsup, bw, 10, FPITCH, time=500.0, mode=9)) == "Flow: float super clips are not supported."
    mv.Flow(isup, bw, 10, [320, 160, 160], fields=1)


def test_flowblur_float_messages_and_their_order(mv):
    isup, bw, fw = _clips(mv)
    fsup = _fsup(mv)
    needs, size = "FlowBlur: the float entry needs a float super clip.", "FlowBlur: wrong source or super clip frame size."
    assert _err(lambda: _blur(mv, fsup, bw, fw, blur=-0.5)) == "FlowBlur: blur must be between 0 and 200 % (inclusive)."
    assert _err(lambda: _blur(mv, isup, bw, fw, blur=200.5, prec=0)) == "FlowBlur: blur must be between 0 and 200 % (inclusive)."
    assert _err(lambda: _blur(mv, fsup, bw, fw, prec=0, thscd1=99999)) == "FlowBlur: prec must be at least 1."
    assert _err(lambda: _blur(mv, fsup, bw, fw, thscd1=16321)) == "FlowBlur: thscd1 can be at most 16320."
    _blur(mv, fsup, bw, fw, thscd1=16320, prec=64, blur=200.0)
    assert _err(lambda: _blur(mv, fsup, bw, _copy(mv, fw, nWidth=336))) == "FlowBlur: mvbw and mvfw have different widths."
    assert _err(lambda: _blur(mv, isup, bw, _copy(mv, fw, nWidth=336, nPel=4))) == "FlowBlur: mvbw and mvfw have different pel precision."
    assert _err(lambda: _blur(mv, fsup, _copy(mv, bw, nDeltaFrame=0), _copy(mv, fw, nDeltaFrame=0))) == \
        "FlowBlur: cannot use motion vectors with absolute frame references."
    assert _err(lambda: _blur(mv, fsup, bw, _copy(mv, fw, nDeltaFrame=2))) == "FlowBlur: mvbw and mvfw must be generated with the same delta."
    assert _err(lambda: _blur(mv, fsup, fw, fw)) == "FlowBlur: mvbw must be generated with isb=True."
    assert _err(lambda: _blur(mv, isup, bw, bw)) == "FlowBlur: mvfw must be generated with isb=False."
    assert _err(lambda: _blur(mv, _fsup(mv, w=336), bw, fw)) == size
    assert _err(lambda: _blur(mv, _fsup(mv, pel=1), bw, fw)) == size
    assert _err(lambda: _blur(mv, _fsup(mv, w=336), bw, bw)) == "FlowBlur: mvfw must be generated with isb=False."
    assert _err(lambda: _blur(mv, isup, bw, fw)) == needs
    assert _err(lambda: _blur(mv, isup, bw, fw, pitch=[4, 4, 4])) == needs
    assert _err(lambda: _blur(mv, mv.Super(336, 192, 8), bw, fw)) == size
    sup16, bw16, fw16 = _clips(mv, bits=16)
    assert _err(lambda: _blur(mv, sup16, bw16, fw16)) == needs
    _blur(mv, fsup, bw16, fw16)
    tiny = _fsup(mv, w=64, h=8)
    isup8 = mv.Super(64, 8, 8)
    tb, tf = mv.Analyse(isup8, isb=1, blksize=8, overlap=0).ad, mv.Analyse(isup8, isb=0, blksize=8, overlap=0).ad
    assert _err(lambda: mv.FlowBlur(tiny, tb, tf, 10, [256, 128, 128], sample_float=True)) == "FlowBlur: the frame must be at least two blocks wide and two blocks high."
    assert _err(lambda: _blur(mv, _split_uv_pitch(_fsup(mv)), bw, fw)) == "FlowBlur: U and V super planes must share one pitch."
    assert _err(lambda: mv.FlowBlur(fsup, bw, bw, 10, FPITCH, blur=500.0)) == "FlowBlur: float super clips are not supported."


def test_pitches_of_the_float_entries(mv):
    """clip and dst: any pitch that holds a row and is a multiple of 4; super: multiples of 16"""
    _, bw, fw = _clips(mv)
    fsup = _fsup(mv)
    msg = lambda name, what, p: "%s: %s pitch of plane %d must hold a row of %d bytes and be a multiple of the sample size." % (name, what, p, ROWS[p])
    for name, make in (("Flow", lambda **kw: _flow(mv, fsup, bw, **kw)), ("FlowBlur", lambda **kw: _blur(mv, fsup, bw, fw, **kw))):
        assert make().dst_pitch == FPITCH
        make(pitch=ROWS)
        make(pitch=[ROWS[0] + 4, ROWS[1], ROWS[2] + 256])                # an odd number of samples; U and V differ
        make(pitch=ROWS, dst_pitch=[ROWS[0] + 12, ROWS[1] + 4, ROWS[2]])
        assert _err(lambda: make(pitch=[ROWS[0] + 2, ROWS[1], ROWS[2]])) == msg(name, "clip", 0)
        assert _err(lambda: make(pitch=[ROWS[0], ROWS[1] - 4, ROWS[2]])) == msg(name, "clip", 1)
        assert _err(lambda: make(pitch=[ROWS[0], ROWS[1], ROWS[2] + 1])) == msg(name, "clip", 2)
        assert _err(lambda: make(pitch=ROWS, dst_pitch=[ROWS[0], ROWS[1] + 2, ROWS[2]])) == msg(name, "dst", 1)
        assert _err(lambda: make(pitch=ROWS, dst_pitch=[ROWS[0] - 4, ROWS[1], ROWS[2]])) == msg(name, "dst", 0)
        assert _err(lambda: make(pitch=[320, 160, 160])) == msg(name, "clip", 0)      # the integer clip's pitches
    odd = _fsup(mv)
    odd.pitch = [odd.pitch[0] + 8, odd.pitch[1], odd.pitch[2]]
    assert _err(lambda: _flow(mv, odd, bw)).startswith("Flow: super pitch of plane 0 must hold a row of ")
    assert _err(lambda: _blur(mv, odd, bw, fw)).startswith("FlowBlur: super pitch of plane 0 must hold a row of ")


def test_reference_frame_is_the_integer_objects(mv):
    isup, bw, fw = _clips(mv)
    for ad in (bw, fw, _copy(mv, bw, nDeltaFrame=2), _copy(mv, fw, nDeltaFrame=-3), _copy(mv, bw, nDeltaFrame=0)):
        new, old = _flow(mv, _fsup(mv), ad), mv.Flow(isup, ad, 10, [320, 160, 160])
        assert [new.ref(n) for n in range(10)] == [old.ref(n) for n in range(10)]


def test_flowcomp_frames_checks_its_jobs_before_any_device_call(mv):
    _, bw, _ = _clips(mv)
    L, A = mv.lib(), 0x10000  # never dereferenced
    g = _flow(mv, _fsup(mv), bw, mode=1)
    job = (mv.FlowCompJob * 1)()

    def fill(clip=(A, A, A), out=(A, A, A), ref=(A, A, A), blob=A):
        for p in range(3):
            job[0].clip[p], job[0].ref_super[p], job[0].dst[p] = clip[p], ref[p], out[p]
        job[0].blob = blob
        assert L.mvx_flowcomp_frames(g.h, 1, job, None) == -1
        return L.mvx_last_error().decode()
    assert fill(out=(None, A, A)) == "mvx_flowcomp_frames: dst / clip are required"
    assert fill(clip=(None, A, A), ref=(None, None, None), blob=None) == "mvx_flowcomp_frames: dst / clip are required"
    assert fill(out=(A + 2, A, A)) == "mvx_flowcomp_frames: dst plane 0 must be aligned to 4 bytes"
    assert fill(out=(A, A, A + 1)) == "mvx_flowcomp_frames: dst plane 2 must be aligned to 4 bytes"
    assert fill(out=(A, None, A)) == "mvx_flowcomp_frames: dst plane 1 is required"
    assert fill(clip=(A, A + 2, A)) == "mvx_flowcomp_frames: clip plane 1 must be aligned to 4 bytes"
    assert fill(clip=(A, A, None)) == "mvx_flowcomp_frames: clip plane 2 is required"
    assert fill(ref=(A + 4, A, A)) == "mvx_flowcomp_frames: ref_super plane 0 must be aligned to 16 bytes"
    assert fill(ref=(A, A, A + 8)) == "mvx_flowcomp_frames: ref_super plane 2 must be aligned to 16 bytes"
    assert fill(ref=(None, None, A + 8), blob=None) == "mvx_flowcomp_frames: ref_super plane 2 must be aligned to 16 bytes"
    assert L.mvx_flowcomp_frames(g.h, 0, job, None) == 0


def test_flowblur_frames_checks_its_jobs_before_any_device_call(mv):
    _, bw, fw = _clips(mv)
    L, A = mv.lib(), 0x10000
    g = _blur(mv, _fsup(mv), bw, fw)
    job = (mv.FlowBlurJob * 1)()

    def fill(clip=(A, A, A), out=(A, A, A), sup=(A, A, A)):
        for p in range(3):
            job[0].clip[p], job[0].super[p], job[0].dst[p] = clip[p], sup[p], out[p]
        job[0].blob_bw = job[0].blob_fw = A
        assert L.mvx_flowblur_frames(g.h, 1, job, None) == -1
        return L.mvx_last_error().decode()
    assert fill(clip=(None, A, A)) == "mvx_flowblur_frames: dst / clip are required"
    assert fill(out=(A + 6, A, A)) == "mvx_flowblur_frames: dst plane 0 must be aligned to 4 bytes"
    assert fill(out=(A, A, None)) == "mvx_flowblur_frames: dst plane 2 is required"
    assert fill(clip=(A, A + 3, A)) == "mvx_flowblur_frames: clip plane 1 must be aligned to 4 bytes"
    assert fill(sup=(A, A + 4, A)) == "mvx_flowblur_frames: super plane 1 must be aligned to 16 bytes"
    assert L.mvx_flowblur_frames(g.h, 0, job, None) == 0


def test_the_keyword_selects_the_float_entries_and_nothing_else_changes(mv):
    isup, bw, fw = _clips(mv)
    fsup = _fsup(mv)
    pairs = ((lambda s: _flow(mv, s, bw), lambda s: mv.Flow(s, bw, 10, [320, 160, 160])),
             (lambda s: _blur(mv, s, bw, fw), lambda s: mv.FlowBlur(s, bw, fw, 10, [320, 160, 160])))
    for make, plain in pairs:
        new, old = make(fsup), plain(isup)
        assert new.is_float and not old.is_float
        assert new.dst_pitch == FPITCH and old.dst_pitch == [320, 160, 160]
        assert _err(lambda: plain(fsup)).endswith("float super clips are not supported.")
        assert _err(lambda: make(isup)).endswith("the float entry needs a float super clip.")
    assert np.dtype(fsup.dtype) == np.float32
    # FlowInter and FlowFPS have no float entry: their creates refuse the float super clip as before
    assert _err(lambda: mv.FlowInter(fsup, bw, fw, 10, FPITCH)) == "FlowInter: float super clips are not supported."
    assert _err(lambda: mv.FlowFPS(fsup, bw, fw, 10, FPITCH)) == "FlowFPS: float super clips are not supported."
