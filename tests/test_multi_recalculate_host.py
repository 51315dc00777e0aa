"""CPU tests of RecalculateN's creation and job checks (neither touches a device): the radius limit, the field-0 check, then
mvx_recalculate_create's messages and order under the new name; the MVTools_MVAnalysisData of every field against the Recalculate created
on that field's old data; the layout of the multi blob; and the job checks that run before any device call."""
import ctypes as C

import pytest

from test_block_host import _copy, _err, _split_uv_pitch

RADIUS = "RecalculateN: radius must be between 1 and 24."
FIELD0 = "RecalculateN: vectors_data must be field 0 of a multi blob."

INVALID = [dict(search=9), dict(search=-1, dct=11), dict(dct=11), dict(blksize=16, blksizev=2, dct=5), dict(dct=1), dict(dct=4, divide=3), dict(divide=3),
           dict(blksize=12), dict(blksize=12, pnew=300), dict(pnew=300), dict(pnew=-1, overlap=6), dict(overlap=6), dict(blksize=4, overlap=2, divide=1),
           dict(blksize=8, overlap=3), dict(blksize=8, overlap=2, divide=1), dict(chroma=1, overlap=5, search=8)]


def _old(mv, w=320, h=192, bits=8, sup_kw=None, **akw):
    sup = mv.Super(w, h, bits, **(sup_kw or {}))
    return sup, mv.AnalyseN(sup, 1, **akw).ad(0)


@pytest.mark.parametrize("kw", INVALID, ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_recalculate_n_reports_recalculates_messages_under_its_name(mv, kw):
    sup, ad = _old(mv)
    want = _err(lambda: mv.Recalculate(sup, ad, **kw))
    assert want.startswith("Recalculate: ")
    assert _err(lambda: mv.RecalculateN(sup, ad, 3, **kw)) == "RecalculateN: " + want[len("Recalculate: "):]


def test_recalculate_n_checks_radius_then_field_0_then_recalculates(mv):
    sup, ad = _old(mv)
    fw1, bw2 = _copy(mv, ad, isBackward=0), _copy(mv, ad, nDeltaFrame=2)
    assert mv.DEGRAIN_N_MAX_RADIUS == 24
    assert _err(lambda: mv.RecalculateN(sup, ad, 0)) == RADIUS
    assert _err(lambda: mv.RecalculateN(sup, fw1, 25, search=9)) == RADIUS
    assert _err(lambda: mv.RecalculateN(sup, bw2, -1)) == RADIUS
    assert _err(lambda: mv.RecalculateN(sup, fw1, 3)) == FIELD0
    assert _err(lambda: mv.RecalculateN(sup, bw2, 3)) == FIELD0
    assert _err(lambda: mv.RecalculateN(sup, fw1, 3, search=9)) == FIELD0
    for r in (1, 2, 5):  # every other field of a multi blob
        assert _err(lambda: mv.RecalculateN(sup, mv.AnalyseN(sup, 3).ad(r), 3)) == FIELD0
    assert _err(lambda: mv.RecalculateN(sup, ad, 3, search=9, divide=3)) == "RecalculateN: search must be between 0 and 7 (inclusive)."
    # the checks behind the arguments, in Recalculate's order
    assert _err(lambda: mv.RecalculateN(mv.Super(336, 192, 8), ad, 3)) == "RecalculateN: wrong frame size."
    assert _err(lambda: mv.RecalculateN(mv.Super(336, 192, 8), ad, 3, pnew=300)) == "RecalculateN: pnew must be between 0 and 256 (inclusive)."
    assert _err(lambda: mv.RecalculateN(mv.Super(320, 192, 8, subsampling=(0, 0)), ad, 3)) == "RecalculateN: wrong frame size."
    assert _err(lambda: mv.RecalculateN(mv.Super(320, 192, 8, chroma=False), ad, 3)) == "RecalculateN: super clip does not contain needed colour data."
    mv.RecalculateN(mv.Super(320, 192, 8, chroma=False), ad, 3, chroma=0)
    assert _err(lambda: mv.RecalculateN(_split_uv_pitch(mv.Super(320, 192, 8)), ad, 3)) == "RecalculateN: the U and V planes of the super clip must share one pitch."
    mv.RecalculateN(sup, ad, 1)
    mv.RecalculateN(sup, ad, 24)
    # Recalculate itself keeps its name and takes any field
    assert _err(lambda: mv.Recalculate(sup, fw1, search=9)) == "Recalculate: search must be between 0 and 7 (inclusive)."
    mv.Recalculate(sup, bw2)


def test_recalculate_n_keeps_dct_1_to_4_behind_the_switch(mv):
    sup, ad = _old(mv)
    assert _err(lambda: mv.RecalculateN(sup, ad, 2, dct=3)) == "RecalculateN: dct 1..4 (FFTW3 DCT cost) are not implemented on the GPU path."
    was = mv.enable_dct_float(True)
    try:
        assert mv.RecalculateN(sup, ad, 2, dct=3).get_data(0).nBlkSizeX == 8
        assert _err(lambda: mv.RecalculateN(sup, ad, 2, dct=3, blksize=64)) == "RecalculateN: dct 1..4 are implemented for blocks up to 32x32."
    finally:
        mv.enable_dct_float(was)


# w, h, bits, super kwargs, analyse kwargs, recalculate kwargs: 16 -> 8 blocks, overlap, divide=1
GEOMETRIES = [(320, 192, 8, {}, dict(blksize=16, overlap=8), dict(blksize=8, overlap=4)),
              (204, 116, 16, {}, dict(blksize=8, overlap=4), dict(blksize=8, overlap=0, thsad=100, smooth=0)),
              (320, 192, 8, dict(pel=1), dict(blksize=16), dict(blksize=8, overlap=4, divide=1)),
              (133, 77, 8, dict(subsampling=(0, 0)), dict(blksize=16, overlap=8, divide=1), dict(blksize=8, blksizev=4, chroma=0))]


@pytest.mark.parametrize("radius", [1, 3, 24])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "%dx%d-%dbit-%s" % (g[0], g[1], g[2], "-".join("%s%s" % kv for kv in g[5].items())))
def test_every_field_reports_the_data_of_its_recalculate(mv, geo, radius):
    w, h, bits, skw, akw, rkw = geo
    sup = mv.Super(w, h, bits, **skw)
    an = mv.AnalyseN(sup, radius, **akw)
    rn = mv.RecalculateN(sup, an.ad(0), radius, **rkw)
    for r in range(2 * radius):
        one = mv.Recalculate(sup, an.ad(r), **rkw)
        got = rn.get_data(r)
        assert bytes(got) == bytes(one.ad), "field %d" % r
        assert (got.isBackward, got.nDeltaFrame) == (int(r % 2 == 0), r // 2 + 1)
    assert _err(lambda: rn.get_data(-1)) == "mvx_recalculate_n_get_data: field -1 of %d" % (2 * radius)
    assert _err(lambda: rn.get_data(2 * radius)) == "mvx_recalculate_n_get_data: field %d of %d" % (2 * radius, 2 * radius)
    assert rn.radius == radius
    assert rn.field_size == one.blob_size
    assert rn.field_stride == (one.blob_size + 255) // 256 * 256 and rn.field_stride % 256 == 0
    assert rn.blob_size == 2 * radius * rn.field_stride
    L = mv.lib()
    assert (L.mvx_recalculate_n_field_size(rn.h), L.mvx_recalculate_n_field_stride(rn.h), L.mvx_recalculate_n_blob_size(rn.h)) \
        == (rn.field_size, rn.field_stride, rn.blob_size)


def test_the_geometries_leave_pad_bytes(mv):
    for w, h, bits, skw, akw, rkw in GEOMETRIES:
        sup = mv.Super(w, h, bits, **skw)
        rn = mv.RecalculateN(sup, mv.AnalyseN(sup, 1, **akw).ad(0), 1, **rkw)
        assert 0 < rn.field_size < rn.field_stride


def test_frames_refuse_incomplete_and_misaligned_jobs_before_any_device_call(mv):
    sup, ad = _old(mv)
    L = mv.lib()
    rn = mv.RecalculateN(sup, ad, 2, blksize=8, overlap=4)
    jobs = (mv.RecalculateNJob * 1)()
    need = "mvx_recalculate_n_frames: a job needs its reference table and its blob"
    aligned = "mvx_recalculate_n_frames: blobs must be 16-byte aligned"

    def run():
        rc = L.mvx_recalculate_n_frames(rn.h, 1, jobs, None)
        return rc, L.mvx_last_error().decode()

    assert L.mvx_recalculate_n_frames(rn.h, 0, jobs, None) == 0
    assert run() == (-1, need)
    refs = ((C.c_void_p * 3) * 4)()  # every reference NULL: no plane would be read
    jobs[0].refs = C.cast(refs, C.POINTER(C.c_void_p * 3))
    assert run() == (-1, need)
    jobs[0].blob = 4096
    assert run() == (-1, "mvx_recalculate_n_frames: old_blob is required")
    jobs[0].old_blob, jobs[0].old_field_stride = 8192, 256
    jobs[0].blob = 4096 + 8
    assert run() == (-1, aligned)
    jobs[0].blob, jobs[0].old_blob = 4096, 8192 + 4
    assert run() == (-1, aligned)
    jobs[0].old_blob, jobs[0].old_field_stride = 8192, 264
    assert run() == (-1, aligned)
