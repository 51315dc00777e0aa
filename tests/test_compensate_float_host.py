"""CPU tests of the float Compensate entries (mvx_compensate_create_float, mvx_compensate_n_create_float; no create touches a device and
*_frames checks its jobs before any launch): both creates' messages and their order, the float entries handed integer super clips, both refusals
of `fields`, the output map, the job checks of both *_frames, and the package's sample_float keyword."""
import ctypes as C

import numpy as np
import pytest

from test_block_host import _clips, _copy, _err, _split_uv_pitch

FPITCH = [1280, 768, 768]  # rows of 320 / 160 float samples, rounded up to 256 bytes


def _fsup(mv, w=320, h=192, **kw):
    return mv.Super(w, h, 32, sample_float=True, **kw)


def _c(mv, sup, ad, **kw):
    return mv.Compensate(sup, ad, sample_float=True, **kw)


def _cn(mv, sup, ad, tr=2, **kw):
    return mv.CompensateN(tr, sup, ad, sample_float=True, **kw)


def test_compensate_n_float_messages_and_their_order(mv):
    isup, bw, _ = _clips(mv)
    fsup = _fsup(mv)
    tr = "CompensateN: tr must be between 1 and 24."
    needs = "CompensateN: the float entry needs a float super clip."
    size = "CompensateN: wrong source or super clip frame size."
    assert _err(lambda: _cn(mv, fsup, bw, tr=0)) == tr
    assert _err(lambda: _cn(mv, fsup, bw, tr=25, time=-1.0)) == tr
    assert _err(lambda: _cn(mv, isup, bw, tr=25)) == tr                # (the radius comes before the kind of super clip)
    _cn(mv, fsup, bw, tr=1)
    _cn(mv, fsup, bw, tr=24)
    assert _err(lambda: _cn(mv, fsup, bw, time=-0.5)) == "CompensateN: time must be between 0.0 and 100.0 (inclusive)."
    assert _err(lambda: _cn(mv, fsup, bw, time=100.5, thscd1=99999)) == "CompensateN: time must be between 0.0 and 100.0 (inclusive)."
    assert _err(lambda: _cn(mv, fsup, bw, thscd1=16321)) == "CompensateN: thscd1 can be at most 16320."
    _cn(mv, fsup, bw, thscd1=16320, time=0.0)
    assert _err(lambda: _cn(mv, _fsup(mv, w=336), bw)) == size
    assert _err(lambda: _cn(mv, _fsup(mv, w=336), bw, thscd1=16321)) == "CompensateN: thscd1 can be at most 16320."
    assert _err(lambda: _cn(mv, _fsup(mv, pel=1), bw)) == size
    # an integer super clip handed to the float entry: after the frame size, before fields
    assert _err(lambda: _cn(mv, isup, bw)) == needs
    assert _err(lambda: _cn(mv, isup, bw, fields=1)) == needs
    assert _err(lambda: _cn(mv, isup, bw, thscd1=16321)) == "CompensateN: thscd1 can be at most 16320."
    assert _err(lambda: _cn(mv, mv.Super(336, 192, 8), bw)) == size
    sup16, bw16, _ = _clips(mv, bits=16)
    assert _err(lambda: _cn(mv, sup16, bw16)) == needs
    _cn(mv, fsup, bw16)                                                # vectors of a 16-bit search
    sup1, bw1, _ = _clips(mv, sup_kw=dict(pel=1))
    assert _err(lambda: _cn(mv, _fsup(mv, pel=1), bw1, fields=1)) == "CompensateN: fields option requires pel > 1."
    assert _err(lambda: _cn(mv, sup1, bw1, fields=1)) == needs
    _cn(mv, _fsup(mv, pel=1), bw1, fields=0)
    assert _err(lambda: _cn(mv, fsup, bw, fields=1)) == "CompensateN: fields is not supported."
    _, bwo, _ = _clips(mv, overlap=4)
    assert _err(lambda: _cn(mv, fsup, _copy(mv, bwo, nBlkY=2))) == "overlap needs at least 3x3 blocks (window selection divides by nBlk-2)."
    assert _err(lambda: _cn(mv, fsup, _copy(mv, bwo, nBlkY=2), fields=1)) == "CompensateN: fields is not supported."
    assert _err(lambda: _cn(mv, _split_uv_pitch(_fsup(mv)), bw)) == "U and V super planes must share one pitch."
    # the integer entry keeps its refusal, first of all
    assert _err(lambda: mv.CompensateN(99, fsup, bw, time=500.0)) == "CompensateN: float super clips are not supported."


def test_compensate_float_messages_and_their_order(mv):
    isup, bw, fw = _clips(mv)
    fsup = _fsup(mv)
    needs = "Compensate: the float entry needs a float super clip."
    size = "Compensate: wrong source or super clip frame size."
    assert _err(lambda: _c(mv, fsup, bw, time=-0.5)) == "Compensate: time must be between 0.0 and 100.0 (inclusive)."
    assert _err(lambda: _c(mv, fsup, bw, time=100.5, thscd1=99999)) == "Compensate: time must be between 0.0 and 100.0 (inclusive)."
    assert _err(lambda: _c(mv, fsup, bw, thscd1=16321)) == "Compensate: thscd1 can be at most 16320."
    _c(mv, fsup, bw, thscd1=16320, time=0.0)
    _c(mv, fsup, fw)
    _c(mv, fsup, _copy(mv, bw, nDeltaFrame=2))                          # any isb, any delta
    assert _err(lambda: _c(mv, _fsup(mv, w=336), bw)) == size
    assert _err(lambda: _c(mv, _fsup(mv, pel=1), bw)) == size
    assert _err(lambda: _c(mv, isup, bw)) == needs
    assert _err(lambda: _c(mv, isup, bw, fields=1)) == needs
    assert _err(lambda: _c(mv, mv.Super(336, 192, 8), bw)) == size
    sup16, bw16, _ = _clips(mv, bits=16)
    assert _err(lambda: _c(mv, sup16, bw16)) == needs
    _c(mv, fsup, bw16)
    _, bw1, _ = _clips(mv, sup_kw=dict(pel=1))
    assert _err(lambda: _c(mv, _fsup(mv, pel=1), bw1, fields=1)) == "Compensate: fields option requires pel > 1."
    assert _err(lambda: _c(mv, fsup, bw, fields=1)) == "Compensate: fields is not supported on float clips."
    _c(mv, fsup, bw, fields=0)
    _, bwo, _ = _clips(mv, overlap=4)
    assert _err(lambda: _c(mv, fsup, _copy(mv, bwo, nBlkX=2))) == "overlap needs at least 3x3 blocks (window selection divides by nBlk-2)."
    assert _err(lambda: _c(mv, fsup, _copy(mv, bwo, nBlkX=2), fields=1)) == "Compensate: fields is not supported on float clips."
    assert _err(lambda: _c(mv, _split_uv_pitch(_fsup(mv)), bw)) == "U and V super planes must share one pitch."
    assert _err(lambda: mv.Compensate(fsup, bw, time=500.0)) == "Compensate: float super clips are not supported."
    mv.Compensate(isup, bw, fields=1)                                   # the integer entry still takes fields


def test_pitches_of_the_float_entries(mv):
    """dst: any pitch that holds a row and is a multiple of 4; super: multiples of 16"""
    _, bw, _ = _clips(mv)
    fsup = _fsup(mv)
    rows = [320 * 4, 160 * 4, 160 * 4]
    msg = lambda p: "dst pitch of plane %d must hold a row of %d bytes and be a multiple of the sample size." % (p, rows[p])
    for make in (_c, _cn):
        assert make(mv, fsup, bw).dst_pitch == FPITCH
        make(mv, fsup, bw, dst_pitch=rows)
        make(mv, fsup, bw, dst_pitch=[rows[0] + 4, rows[1], rows[2] + 256])
        assert _err(lambda: make(mv, fsup, bw, dst_pitch=[rows[0] + 2, rows[1], rows[2]])) == msg(0)
        assert _err(lambda: make(mv, fsup, bw, dst_pitch=[rows[0], rows[1] - 4, rows[2]])) == msg(1)
        assert _err(lambda: make(mv, fsup, bw, dst_pitch=[rows[0], rows[1], rows[2] + 1])) == msg(2)
        odd = _fsup(mv)
        odd.pitch = [odd.pitch[0] + 8, odd.pitch[1], odd.pitch[2]]
        assert _err(lambda: make(mv, odd, bw)).startswith("super pitch of plane 0 must hold a row of ")


@pytest.mark.parametrize("tr", [1, 3])
def test_map_is_the_integer_objects(mv, tr):
    isup, bw, _ = _clips(mv)
    new, old = _cn(mv, _fsup(mv), bw, tr=tr), mv.CompensateN(tr, isup, bw)
    assert [new.map(k) for k in range(2 * tr + 1)] == [old.map(k) for k in range(2 * tr + 1)]
    assert new.map(tr) == (0, -1) and new.map(0) == (-tr, 2 * tr - 1) and new.map(2 * tr) == (tr, 2 * tr - 2)
    assert _err(lambda: new.map(2 * tr + 1)) == "mvx_compensate_n_map: output %d of %d" % (2 * tr + 1, 2 * tr + 1)


def test_compensate_n_frames_checks_its_jobs_before_any_device_call(mv):
    _, bw, _ = _clips(mv)
    L, A = mv.lib(), 0x10000  # never dereferenced
    cn = _cn(mv, _fsup(mv), bw, tr=24)
    limit = 65535 // (49 * 2)
    many = (mv.CompensateNJob * (limit + 1))()
    assert L.mvx_compensate_n_frames(cn.h, limit + 1, many, None) == -1
    assert L.mvx_last_error().decode() == "mvx_compensate_n_frames: at most %d jobs per call at tr 24" % limit
    assert L.mvx_compensate_n_frames(cn.h, 1, many, None) == -1
    assert L.mvx_last_error().decode() == "mvx_compensate_n_frames: a job needs its source, its reference table, its blob and its output table"
    cn = _cn(mv, _fsup(mv), bw, tr=1)
    stride = (mv.AnalyseN(mv.Super(320, 192, 8), 1).field_stride)
    job = (mv.CompensateNJob * 1)()
    refs, dst = ((C.c_void_p * 3) * 2)(), ((C.c_void_p * 3) * 3)()
    job[0].refs, job[0].dst = C.cast(refs, C.POINTER(C.c_void_p * 3)), C.cast(dst, C.POINTER(C.c_void_p * 3))
    job[0].blob, job[0].field_stride = A, stride

    def fill(src=(A, A, A), out=(A, A, A), ref=(A, A, A), k=1):
        for p in range(3):
            job[0].src_super[p] = src[p]
            for r in range(2):
                refs[r][p] = ref[p]
            for o in range(3):
                dst[o][p] = out[p] if o == k else A
        assert L.mvx_compensate_n_frames(cn.h, 1, job, None) == -1
        return L.mvx_last_error().decode()
    assert fill(out=(A + 2, A, A)) == "mvx_compensate_n_frames: dst plane 0 must be aligned to 4 bytes"
    assert fill(out=(A, A, A + 6), k=0) == "mvx_compensate_n_frames: dst plane 2 must be aligned to 4 bytes"
    assert fill(out=(A, None, A), k=2) == "mvx_compensate_n_frames: output 2 lacks plane 1"
    assert fill(src=(A + 4, A, A)) == "mvx_compensate_n_frames: source super plane 0 must be aligned to 16 bytes"
    assert fill(ref=(A, A + 8, A)) == "mvx_compensate_n_frames: reference super plane 1 must be aligned to 16 bytes"
    job[0].field_stride = 8
    assert fill().startswith("mvx_compensate_n_frames: field_stride must be a multiple of 16 and hold a field's ")


def test_compensate_frames_checks_its_jobs_before_any_device_call(mv):
    _, bw, _ = _clips(mv)
    L, A = mv.lib(), 0x10000
    comp = _c(mv, _fsup(mv), bw)
    job = (mv.CompensateJob * 1)()

    def fill(src=(A, A, A), out=(A, A, A), ref=(A, A, A), blob=A, shift=0):
        for p in range(3):
            job[0].src_super[p], job[0].ref_super[p], job[0].dst[p] = src[p], ref[p], out[p]
        job[0].blob, job[0].field_shift = blob, shift
        assert L.mvx_compensate_frames(comp.h, 1, job, None) == -1
        return L.mvx_last_error().decode()
    assert fill(shift=1) == "mvx_compensate_frames: field_shift is not supported on float clips"
    assert fill(shift=-2, out=(A + 2, A, A)) == "mvx_compensate_frames: field_shift is not supported on float clips"
    assert fill(blob=None) == "mvx_compensate_frames: a job needs its blob"
    assert fill(out=(A + 2, A, A)) == "mvx_compensate_frames: dst plane 0 must be aligned to 4 bytes"
    assert fill(out=(A, A, None)) == "mvx_compensate_frames: dst plane 2 is required"
    assert fill(src=(A, A + 4, A)) == "mvx_compensate_frames: source super plane 1 must be aligned to 16 bytes"
    assert fill(src=(None, A, A)) == "mvx_compensate_frames: source super plane 0 is required"
    assert fill(ref=(A + 8, A, A)) == "mvx_compensate_frames: reference super plane 0 must be aligned to 16 bytes"
    many = (mv.CompensateJob * 32768)()
    assert L.mvx_compensate_frames(comp.h, 32768, many, None) == -1
    assert L.mvx_last_error().decode() == "mvx_compensate_frames: at most 32767 jobs per call on float clips"
    assert L.mvx_compensate_frames(comp.h, 0, many, None) == 0


def test_the_keyword_selects_the_float_entries_and_nothing_else_changes(mv):
    isup, bw, _ = _clips(mv)
    fsup = _fsup(mv)
    for make, plain in ((_c, lambda s, **kw: mv.Compensate(s, bw, **kw)), (lambda m, s, a, **kw: _cn(m, s, a, **kw), lambda s, **kw: mv.CompensateN(2, s, bw, **kw))):
        new, old = make(mv, fsup, bw), plain(isup)
        assert new.is_float and not old.is_float
        assert new.dst_pitch == FPITCH and old.dst_pitch == [512, 256, 256]
        assert _err(lambda: plain(fsup)).endswith("float super clips are not supported.")
        assert _err(lambda: make(mv, isup, bw)).endswith("the float entry needs a float super clip.")
    assert np.dtype(fsup.dtype) == np.float32
