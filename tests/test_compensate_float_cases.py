"""CPU: the searched cases of tests/test_gpu_compensate_float.py test what they claim.  The float clip's quantised copy is the integer clip
(degrain_float_cases.float_clip asserts it), so the vectors are the integer clip's; through the oracle's search alone, on the middle frame of
each case: beyond distance 1 (tr 1: at every distance) at least multi_cases.USED of the (block, field) pairs have a SAD below the case's scaled
thsad -- their block is compensated -- and at least multi_cases.UNUSED have not -- theirs comes from the source.  A float Compensate that never
compensated, or one that ignored thsad, could not pass those cases.  The crafted fields state their shares by construction."""
import numpy as np
import pytest

import compensate_float_cases as cc
import degrain_float_cases as fc
import degrain_n_cases as dc
import multi_cases as mc
import pipeline as pl
import vector_fields


@pytest.mark.parametrize("case", cc.SEARCHED, ids=cc.case_id)
def test_far_blocks_are_mostly_compensated_and_sometimes_not(oracle, case):
    fmt, bits, blk, tr, w, h, thsad = case
    frames = dc.clip(w, h, bits, mc.nframes(tr), fmt)
    fc.float_clip(frames[:1], bits, seed=9)  # (asserts that the quantised copy of the float clip is the integer clip)
    osup = oracle.Super(w, h, bits, **dict(dc.FORMATS[fmt], **blk[1]))
    osf = [osup.frame(f) for f in frames]
    n, sads = tr + 1, []
    for r in range(2 * tr):
        isb, d = mc.field_of(r)
        oan = oracle.Analyse(osup, isb=isb, delta=d, **blk[2])
        sads.append(pl.blob_vectors(oan.frame(osf[n], osf[n + d if isb else n - d]), oan.ad)[2])
    used, unused = mc.far_shares(sads, oan.ad, thsad, tr)
    print("%s: %.3f of the pairs below thsad %d, %.3f not" % (cc.case_id(case), used, thsad, unused))
    assert used >= mc.USED and unused >= mc.UNUSED, "beyond distance 1: %.3f of the pairs below thsad, %.3f not" % (used, unused)


def test_crafted_fields_fall_back_on_a_tenth_of_their_blocks(oracle):
    osup = oracle.Super(70, 54, 16)
    oan = oracle.Analyse(osup, isb=1, blksize=8, overlap=4)
    frames = dc.clip(70, 54, 16, 2)
    blob = oan.frame(osup.frame(frames[0]), osup.frame(frames[1]))
    crafted = cc.with_fallbacks(blob, oan.ad, 5, 300)
    sad = pl.blob_vectors(crafted, oan.ad)[2]
    th = vector_fields.scaled_thresholds(oan.ad, 300)[0]
    share = float((sad >= th).mean())
    assert mc.UNUSED <= share <= 0.2 and float((sad < th).mean()) >= mc.USED
    xmin, xmax, ymin, ymax = vector_fields.legal_rect(oan.ad)
    vx, vy, _ = pl.blob_vectors(crafted, oan.ad)
    assert (vx == xmin[None, :]).any() and (vx == xmax[None, :]).any() and (vy == ymin[:, None]).any() and (vy == ymax[:, None]).any()
