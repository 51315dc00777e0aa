"""CPU tests of ScaleVect's host side (creation touches no device): the refusals and their order, the analysis data of the scaled clip
against what Analyse reports on the target super clip, the unchanged blob size, and the restatement (tests/scale_vect_ref.py) on a field
on the limits of its legal rectangles.  tests/test_gpu_scale_vect.py runs the same cases through the kernel and the consumers."""
import ctypes as C

import numpy as np
import pytest

import pipeline as pl
import scale_vect_cases as sc
import scale_vect_ref as ref
import synth
import vector_fields as vf

ALL = sc.CASES + [sc.MULTI]
ids = [c.name for c in ALL]


def _supers(mv, case):
    (w, h), (tw, th) = sc.sizes(case)
    return mv.Super(w, h, case.bits, **sc.super_kwargs(case, False)), mv.Super(tw, th, case.tbits, **sc.super_kwargs(case, True))


def _message(fn):
    with pytest.raises(Exception) as e:
        fn()
    return str(e.value)


def _fields(ad):
    return {k: getattr(ad, k) for k, _ in ad._fields_}


# ------------------------------------------------------------------ the refusals, in order

def test_refusals_in_order(mv):
    small = mv.Super(96, 64, 8, pel=4)
    ad = mv.Analyse(small, isb=1, blksize=16, overlap=0).ad
    ad.nBlkSizeY, ad.nBlkY = 2, 32                                                    # 16x2: at 2 the scaled block 32x4 is not in the list
    wrong_all = mv.Super(200, 128, 8, subsampling=(0, 0), pel=1)                      # wrong size, wrong ratios, pel 4 -> 1
    right_size = mv.Super(192, 128, 8, subsampling=(0, 0), pel=1)                     # wrong ratios, block, pel
    right_fmt = mv.Super(192, 128, 8, pel=1)                                          # block, pel
    for scale, target, want in ((3, wrong_all, ref.E_SCALE), (0, wrong_all, ref.E_SCALE), (2, wrong_all, ref.E_SIZE), (2, right_size, ref.E_CHROMA),
                                (2, right_fmt, ref.E_BLOCK)):
        assert _message(lambda: mv.ScaleVect(ad, target, scale)) == want
        assert _message(lambda: ref.scaled_data(ad, scale, target.info)) == want
    ad8 = mv.Analyse(small, isb=1, blksize=8, overlap=4).ad
    assert _message(lambda: mv.ScaleVect(ad8, right_fmt, 2)) == ref.E_PEL             # pel 4 to a pel-1 super clip at 2: m = 1 / 2
    assert _message(lambda: ref.scaled_data(ad8, 2, right_fmt.info)) == ref.E_PEL
    assert _message(lambda: mv.ScaleVect(ad8, mv.Super(192, 128, 8, pel=1), 4)) == ref.E_SIZE
    assert mv.ScaleVect(ad8, mv.Super(192, 128, 8, pel=2), 2).ad.nPel == 2            # m = 1


def test_each_size_condition_and_the_chroma_flag(mv):
    small = mv.Super(96, 64, 8)
    ad = mv.Analyse(small, isb=1, blksize=8, overlap=4).ad
    for tw, th in ((192, 130), (194, 128), (96, 64)):
        assert _message(lambda: mv.ScaleVect(ad, mv.Super(tw, th, 8), 2)) == ref.E_SIZE
    assert _message(lambda: mv.ScaleVect(ad, mv.Super(192, 128, 8, chroma=0), 2)) == ref.E_CHROMA   # the SADs include chroma, the super clip has none
    assert _message(lambda: mv.ScaleVect(ad, mv.Super(192, 128, 8, subsampling=(1, 0)), 2)) == ref.E_CHROMA
    luma_only = mv.Analyse(small, isb=1, blksize=8, overlap=4, chroma=0).ad
    assert mv.ScaleVect(luma_only, mv.Super(192, 128, 8, chroma=0), 2).ad.nBlkSizeX == 16


# ------------------------------------------------------------------ the analysis data of the scaled clip

@pytest.mark.parametrize("case", ALL, ids=ids)
def test_data_is_what_analyse_reports_on_the_target(mv, case):
    """every field, nLvCount and nBlkX/Y included.  nCPUFlags is compared too: the library always writes 0 there (the reference's value
    depends on the host, the library runs no CPU kernels), as it does for nMagicKey and nVersion."""
    ssup, tsup = _supers(mv, case)
    for isb, delta, levels in ((1, 1, None), (0, 1, None), (1, 2, None), (0, 1, 2), (1, 1, -1)):
        kw = dict(isb=isb, delta=delta, levels=levels)
        small = mv.Analyse(ssup, **dict(case.akw, **kw))
        want = mv.Analyse(tsup, **dict(sc.target_analyse_kwargs(case), **kw))
        sv = mv.ScaleVect(small.ad, tsup, case.scale)
        assert _fields(sv.ad) == _fields(want.ad)
        assert _fields(ref.scaled_data(small.ad, case.scale, tsup.info)) == _fields(want.ad)
        # the blob keeps its size and its layout
        size = mv.lib().mvx_vectors_size
        assert size(C.byref(sv.ad)) == size(C.byref(small.ad)) == small.blob_size == want.blob_size == sv.blob_size == ref.vectors_size(sv.ad)
        probe = np.zeros(small.blob_size, np.uint8)
        for level in range(small.ad.nLvCount):
            assert vf.level_span(probe, small.ad, level) == vf.level_span(probe, sv.ad, level)


def test_level_grids_do_not_change_with_the_scale(mv):
    """floor(s * n / 2^i) exceeds s * floor(n / 2^i) by less than s, which cannot cross a multiple of s * (blk - ov): swept over block
    counts, block sizes, overlaps and scales, every level of the scaled geometry has the grid of the original"""
    def grids(blk, ov, n, levels):
        nb = (blk - ov) * n + ov
        return [((nb >> i) - ov) // (blk - ov) for i in range(levels)]
    checked = 0
    for blk, ovs in ((4, (0, 2)), (8, (0, 2, 4)), (16, (0, 2, 4, 8)), (32, (0, 4, 16))):
        for ov in ovs:
            for n in range(1, 300):
                levels = 0
                while ((((blk - ov) * n + ov) >> levels) - ov) // (blk - ov) > 0:
                    levels += 1
                for s in (2, 4):
                    assert grids(blk, ov, n, levels) == grids(s * blk, s * ov, n, levels), (blk, ov, n, s)
                    checked += 1
    assert checked > 5000


# ------------------------------------------------------------------ the restatement on a limits field

def _small_blob(oracle, case):
    (w, h), _ = sc.sizes(case)
    frames = synth.survey_clip(w, h, case.bits, 2)
    osup = oracle.Super(w, h, case.bits, **sc.super_kwargs(case, False))
    oan = oracle.Analyse(osup, isb=1, **case.akw)
    sf = [osup.frame(f) for f in frames]
    return oan.frame(sf[0], sf[1]), oan.ad


def _case(name):
    return next(c for c in ALL if c.name == name)


@pytest.mark.parametrize("name", ["420-limits-pad32", "420-limits-pad16", "420-limits-pad16-8to16-pel1to2", "420-limits-pad16-scale4", "420-limits-pad16-16to8"])
def test_restatement_is_the_identity_or_clamps(oracle, mv, name):
    case = _case(name)
    blob, ad = _small_blob(oracle, case)
    _, tsup = _supers(mv, case)
    out_ad = ref.scaled_data(ad, case.scale, tsup.info)
    small = sc.edit_small(case, blob, ad, 0)
    big = ref.scale_blob(small, ad, out_ad, case.scale)
    m = case.scale * case.tpel // case.pel
    sx, sy, ssad = pl.blob_vectors(small, ad)
    bx, by, bsad = pl.blob_vectors(big, out_ad)
    shift = case.tbits - case.bits
    assert np.array_equal(bsad, ssad * case.scale ** 2 << shift if shift >= 0 else ssad * case.scale ** 2 >> -shift)
    assert bsad[0, 0] == (vf.SAD_HIGH * case.scale ** 2 << shift if shift >= 0 else vf.SAD_HIGH * case.scale ** 2 >> -shift)
    xmin, xmax, ymin, ymax = vf.legal_rect(out_ad)
    assert np.all(bx >= xmin[None, :]) and np.all(bx <= xmax[None, :]) and np.all(by >= ymin[:, None]) and np.all(by <= ymax[:, None])
    ux, uy = sx.astype(np.int64) * m, sy.astype(np.int64) * m
    if case.tpad >= 16 * case.scale:
        assert np.array_equal(bx, ux) and np.array_equal(by, uy), "the clamp is the identity when the padding is scale times the small clip's"
        lo, hi = vf.legal_rect(ad)[:2]
        assert np.any(sx == lo[None, :]) and np.any(sx == hi[None, :]), "the field does not reach the limits"
    else:
        sides = [np.count_nonzero((ux < xmin[None, :]) & (bx == xmin[None, :])), np.count_nonzero((ux > xmax[None, :]) & (bx == xmax[None, :])),
                 np.count_nonzero((uy < ymin[:, None]) & (by == ymin[:, None])), np.count_nonzero((uy > ymax[:, None]) & (by == ymax[:, None]))]
        assert all(n > 0 for n in sides), sides
        inside = (ux >= xmin[None, :]) & (ux <= xmax[None, :])
        assert np.array_equal(bx[inside], ux[inside]) and inside.any()
    # a coarser level is scaled and not clamped: the low 32 bits of the 64-bit product
    cx, cy, csad = pl.blob_vectors(big, out_ad, 1)
    assert (cx[0, 0], cy[0, 0]) == (100000 * m, -100000 * m)
    assert (int(cx[-1, -1]), int(cy[-1, -1])) == (int(np.int64(-2 ** 30 * m).astype(np.int32)), int(np.int64(2 ** 30 * m).astype(np.int32)))
    assert csad[-1, -1] == (-3 * case.scale ** 2 << shift if shift >= 0 else -3 * case.scale ** 2 >> -shift)


def test_restatement_copies_an_invalid_blob_and_multi_gaps(oracle, mv):
    case = _case("420-invalid")
    blob, ad = _small_blob(oracle, case)
    _, tsup = _supers(mv, case)
    out_ad = ref.scaled_data(ad, case.scale, tsup.info)
    bad = sc.edit_small(case, blob, ad, 0)
    assert np.array_equal(ref.scale_blob(bad, ad, out_ad, case.scale), bad) and not np.array_equal(ref.scale_blob(blob, ad, out_ad, case.scale), blob)
    stride = (blob.size + 255) // 256 * 256
    multi = np.full(3 * stride, 0xA5, np.uint8)
    for r in range(3):
        multi[r * stride:r * stride + blob.size] = blob
    out = ref.scale_multi(multi, ad, out_ad, case.scale, 3, stride)
    for r in range(3):
        assert np.array_equal(out[r * stride:r * stride + blob.size], ref.scale_blob(blob, ad, out_ad, case.scale))
        assert np.all(out[r * stride + blob.size:(r + 1) * stride] == 0xA5)


# ------------------------------------------------------------------ the input of the end-to-end GPU case

def test_pan_clip_is_found_by_the_oracle(oracle):
    """the condition on the input of test_gpu_scale_vect.py::test_end_to_end_pan: the oracle alone finds (2 * pel, 1 * pel) on at least 90 %
    of the interior blocks of the small clip"""
    full, small = sc.pan_clips(256, 160, 2)
    assert full[0][0].shape == (160, 256) and small[0][0].shape == (80, 128)
    osup = oracle.Super(128, 80, 8)
    oan = oracle.Analyse(osup, isb=1, blksize=8, overlap=4)
    sf = [osup.frame(f) for f in small]
    x, y, _ = pl.blob_vectors(oan.frame(sf[0], sf[1]), oan.ad)
    hit = (sc.interior(x) == 2 * oan.ad.nPel) & (sc.interior(y) == 1 * oan.ad.nPel)
    assert hit.mean() >= 0.9, hit.mean()
