"""CPU tests of the creation of AnalyseN and CompensateN (neither touches a device): the messages -- mvx_analyse_create's and
mvx_compensate_create's texts and order under the new names, the radius / tr limits, isb and delta refused, fields refused --, the
MVTools_MVAnalysisData of every field against the Analyse it stands for, the layout of the multi blob, and the map from CompensateN's
output k to (frame, field), the clip ends included."""
import pytest

from test_block_host import _clips, _copy, _err, _split_uv_pitch

INVALID_ANALYSE = [dict(search=9), dict(search_coarse=-1), dict(dct=11), dict(blksize=16, blksizev=2, dct=5), dict(dct=1), dict(divide=3), dict(blksize=12),
                   dict(plevel=3), dict(pnew=300), dict(pzero=-1), dict(pglobal=257), dict(overlap=6), dict(blksize=4, overlap=2, divide=1),
                   dict(blksize=8, overlap=2, divide=1), dict(blksize=8, overlap=3), dict(levels=99), dict(levels=1, search=9, divide=3)]


@pytest.mark.parametrize("kw", INVALID_ANALYSE, ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_analyse_n_reports_analyses_messages_under_its_name(mv, kw):
    sup = mv.Super(320, 192, 8)
    want = _err(lambda: mv.Analyse(sup, **kw))
    assert want.startswith("Analyse: ")
    assert _err(lambda: mv.AnalyseN(sup, 3, **kw)) == "AnalyseN: " + want[len("Analyse: "):]


def test_analyse_n_checks_radius_then_isb_and_delta_then_analyses(mv):
    sup = mv.Super(320, 192, 8)
    radius = "AnalyseN: radius must be between 1 and 24."
    fixed = "AnalyseN: isb and delta are set by the radius."
    assert mv.DEGRAIN_N_MAX_RADIUS == 24
    assert _err(lambda: mv.AnalyseN(sup, 0)) == radius
    assert _err(lambda: mv.AnalyseN(sup, 25, isb=1, search=9)) == radius
    assert _err(lambda: mv.AnalyseN(sup, -1, delta=2)) == radius
    assert _err(lambda: mv.AnalyseN(sup, 3, isb=1)) == fixed
    assert _err(lambda: mv.AnalyseN(sup, 3, isb=0)) == fixed
    assert _err(lambda: mv.AnalyseN(sup, 3, delta=1)) == fixed
    assert _err(lambda: mv.AnalyseN(sup, 3, delta=2, search=9)) == fixed
    assert _err(lambda: mv.AnalyseN(sup, 3, search=9, divide=3)) == "AnalyseN: search must be between 0 and 7 (inclusive)."
    assert _err(lambda: mv.AnalyseN(_split_uv_pitch(mv.Super(320, 192, 8)), 3)) == "AnalyseN: the U and V planes of the super clip must share one pitch."
    mv.AnalyseN(sup, 1)
    mv.AnalyseN(sup, 24, num_frames=3)  # (a radius beyond the clip is fine: those fields are invalid blobs)


def test_analyse_n_keeps_dct_1_to_4_behind_the_switch(mv):
    sup = mv.Super(320, 192, 8)
    assert _err(lambda: mv.AnalyseN(sup, 2, dct=3)) == "AnalyseN: dct 1..4 (FFTW3 DCT cost) are not implemented on the GPU path."
    was = mv.enable_dct_float(True)
    try:
        assert mv.AnalyseN(sup, 2, dct=3).ad(0).nBlkSizeX == 8
        assert _err(lambda: mv.AnalyseN(sup, 2, dct=3, blksize=64)) == "AnalyseN: dct 1..4 are implemented for blocks up to 32x32."
    finally:
        mv.enable_dct_float(was)


GEOMETRIES = [(320, 192, 8, {}, {}), (204, 116, 16, {}, dict(blksize=16, overlap=8)), (320, 192, 8, {}, dict(blksize=16, overlap=8, divide=1)),
              (133, 77, 8, dict(subsampling=(0, 0), pel=1), dict(blksize=8, blksizev=4, chroma=0)), (320, 192, 10, dict(gray=True), dict(overlap=4, levels=2))]


@pytest.mark.parametrize("radius", [1, 3, 24])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "%dx%d-%dbit" % g[:3])
def test_every_field_reports_the_data_of_its_analyse(mv, geo, radius):
    w, h, bits, skw, akw = geo
    sup = mv.Super(w, h, bits, **skw)
    an = mv.AnalyseN(sup, radius, **akw)
    for r in range(2 * radius):
        one = mv.Analyse(sup, isb=int(r % 2 == 0), delta=r // 2 + 1, **akw)
        assert bytes(an.ad(r)) == bytes(one.ad), "field %d" % r
        assert (an.ad(r).isBackward, an.ad(r).nDeltaFrame) == (int(r % 2 == 0), r // 2 + 1)
    assert _err(lambda: an.ad(-1)) == "mvx_analyse_n_get_data: field -1 of %d" % (2 * radius)
    assert _err(lambda: an.ad(2 * radius)) == "mvx_analyse_n_get_data: field %d of %d" % (2 * radius, 2 * radius)
    assert an.radius == radius
    assert an.field_size == one.blob_size
    assert an.field_stride == (one.blob_size + 255) // 256 * 256 and an.field_stride % 256 == 0
    assert an.blob_size == 2 * radius * an.field_stride


def test_multi_refs_is_the_order_of_the_fields(mv):
    assert mv.multi_refs(5, 2, 20) == [6, 4, 7, 3]
    assert mv.multi_refs(0, 3, 20) == [1, None, 2, None, 3, None]
    assert mv.multi_refs(19, 2, 20) == [None, 18, None, 17]
    assert mv.multi_refs(1, 3, 4) == [2, 0, 3, None, None, None]


def _cn(mv, sup, ad, tr=2, **kw):
    return mv.CompensateN(tr, sup, ad, **kw)


def test_compensate_n_argument_checks_are_compensates_in_compensates_order(mv):
    sup, bw, _ = _clips(mv)
    tr = "CompensateN: tr must be between 1 and 24."
    assert _err(lambda: _cn(mv, sup, bw, tr=0)) == tr
    assert _err(lambda: _cn(mv, sup, bw, tr=25, time=-1.0)) == tr
    _cn(mv, sup, bw, tr=1)
    _cn(mv, sup, bw, tr=24)
    assert _err(lambda: _cn(mv, sup, bw, time=-0.5)) == "CompensateN: time must be between 0.0 and 100.0 (inclusive)."
    assert _err(lambda: _cn(mv, sup, bw, time=100.5, thscd1=99999)) == "CompensateN: time must be between 0.0 and 100.0 (inclusive)."
    assert _err(lambda: _cn(mv, sup, bw, thscd1=16321)) == "CompensateN: thscd1 can be at most 16320."
    _cn(mv, sup, bw, thscd1=16320, time=0.0)
    sup2 = mv.Super(336, 192, 8)
    assert _err(lambda: _cn(mv, sup2, bw)) == "CompensateN: wrong source or super clip frame size."
    assert _err(lambda: _cn(mv, sup2, bw, thscd1=16321)) == "CompensateN: thscd1 can be at most 16320."
    assert _err(lambda: _cn(mv, mv.Super(320, 192, 8, pel=1), bw)) == "CompensateN: wrong source or super clip frame size."
    sup1, bw1, _ = _clips(mv, sup_kw=dict(pel=1))
    assert _err(lambda: _cn(mv, sup1, bw1, fields=1)) == "CompensateN: fields option requires pel > 1."
    _cn(mv, sup1, bw1, fields=0)
    assert _err(lambda: _cn(mv, sup, bw1, fields=1)) == "CompensateN: wrong source or super clip frame size."  # the size check comes first
    # fields is refused in this form of the filter, after Compensate's own checks
    assert _err(lambda: _cn(mv, sup, bw, fields=1)) == "CompensateN: fields is not supported."
    _cn(mv, sup, bw, fields=0)
    supo, bwo, _ = _clips(mv, overlap=4)
    assert _err(lambda: _cn(mv, supo, _copy(mv, bwo, nBlkY=2))) == "overlap needs at least 3x3 blocks (window selection divides by nBlk-2)."
    assert _err(lambda: _cn(mv, supo, _copy(mv, bwo, nBlkY=2), fields=1)) == "CompensateN: fields is not supported."
    assert _err(lambda: _cn(mv, _split_uv_pitch(mv.Super(320, 192, 8)), bw)) == "U and V super planes must share one pitch."
    assert _err(lambda: _cn(mv, _split_uv_pitch(mv.Super(320, 192, 8, pel=1)), bw1, fields=1)) == "CompensateN: fields option requires pel > 1."
    # Compensate itself keeps its name and still takes fields
    assert _err(lambda: mv.Compensate(sup, bw, time=-0.5)) == "Compensate: time must be between 0.0 and 100.0 (inclusive)."
    mv.Compensate(sup, bw, fields=1)


@pytest.mark.parametrize("tr", [1, 2, 5])
def test_output_k_maps_to_its_frame_and_field(mv, tr):
    """temporal order: before the centre the forward field (odd) of distance tr - k, behind it the backward field (even) of distance k - tr"""
    sup = mv.Super(320, 192, 8)
    an = mv.AnalyseN(sup, tr)
    cn = mv.CompensateN(tr, sup, an.ad(0))
    seen = []
    for k in range(2 * tr + 1):
        off, field = cn.map(k)
        assert off == k - tr
        if k == tr:
            assert field == -1
            continue
        ad = an.ad(field)
        assert ad.nDeltaFrame == abs(off) and bool(ad.isBackward) == (off > 0)
        seen.append(field)
    assert sorted(seen) == list(range(2 * tr))
    assert _err(lambda: cn.map(-1)) == "mvx_compensate_n_map: output -1 of %d" % (2 * tr + 1)
    assert _err(lambda: cn.map(2 * tr + 1)) == "mvx_compensate_n_map: output %d of %d" % (2 * tr + 1, 2 * tr + 1)
    # at the clip's ends the frame of an output lies outside the clip exactly where its field's reference does
    nframes = 2 * tr + 3
    for n in (0, 1, tr + 1, nframes - 2, nframes - 1):
        refs = mv.multi_refs(n, tr, nframes)
        for k in range(2 * tr + 1):
            off, field = cn.map(k)
            if field >= 0:
                inside = 0 <= n + off < nframes
                assert refs[field] == (n + off if inside else None), (n, k)


def test_frames_refuse_incomplete_jobs_and_too_many_before_any_device_call(mv):
    import ctypes as C
    sup, bw, _ = _clips(mv)
    L = mv.lib()
    an = mv.AnalyseN(sup, 2)
    assert L.mvx_analyse_n_frames(an.h, 1, (mv.AnalyseNJob * 1)(), None) == -1
    assert L.mvx_last_error().decode() == "mvx_analyse_n_frames: a job needs its reference table and its blob"
    cn = mv.CompensateN(24, sup, bw)
    limit = 65535 // (49 * 2)  # a grid's z holds 65535 (job, output, chroma plane) triples
    jobs = (mv.CompensateNJob * (limit + 1))()
    assert L.mvx_compensate_n_frames(cn.h, limit + 1, jobs, None) == -1
    assert L.mvx_last_error().decode() == "mvx_compensate_n_frames: at most %d jobs per call at tr 24" % limit
    assert L.mvx_compensate_n_frames(cn.h, 1, jobs, None) == -1
    assert L.mvx_last_error().decode() == "mvx_compensate_n_frames: a job needs its source, its reference table, its blob and its output table"
    fake = C.c_void_p(4096)
    refs, dst = ((C.c_void_p * 3) * 48)(), ((C.c_void_p * 3) * 49)()
    for k in range(49):
        for p in range(3):
            dst[k][p] = 4096
    jobs[0].src_super[0], jobs[0].blob, jobs[0].field_stride = fake, fake, 8
    jobs[0].refs, jobs[0].dst = C.cast(refs, C.POINTER(C.c_void_p * 3)), C.cast(dst, C.POINTER(C.c_void_p * 3))
    assert L.mvx_compensate_n_frames(cn.h, 1, jobs, None) == -1
    assert L.mvx_last_error().decode().startswith("mvx_compensate_n_frames: field_stride must be a multiple of 16 and hold a field's ")
