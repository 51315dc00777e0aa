"""CPU: the CompensateN cases of tests/test_gpu_multi.py test what they claim.  Through the oracle's search alone (whose vectors the GPU
search reproduces bit for bit), on the middle frame of each case: beyond distance 1 at least half of the (block, field) pairs have a SAD
below the case's thsad -- their block is compensated -- and at least a fiftieth have not -- theirs is taken from the source.  A CompensateN
that never compensated, or one that ignored thsad, could not pass those cases."""
import pytest

import degrain_n_cases as dc
import multi_cases as mc
import pipeline as pl


@pytest.mark.parametrize("case", mc.cases(), ids=mc.case_id)
def test_far_blocks_are_mostly_compensated_and_sometimes_not(oracle, case):
    fmt, bits, blk, radius = case
    frames = mc.clip(fmt, bits, radius)
    osup = oracle.Super(mc.W, mc.H, bits, **dict(dc.FORMATS[fmt], **blk[1]))
    osf = [osup.frame(f) for f in frames]
    n, sads = radius + 1, []
    for r in range(2 * radius):
        isb, d = mc.field_of(r)
        oan = oracle.Analyse(osup, isb=isb, delta=d, **blk[2])
        sads.append(pl.blob_vectors(oan.frame(osf[n], osf[n + d if isb else n - d]), oan.ad)[2])
    used, unused = mc.far_shares(sads, oan.ad, mc.THSAD, radius)
    assert used >= mc.USED and unused >= mc.UNUSED, "beyond distance 1: %.3f of the pairs below thsad, %.3f not" % (used, unused)
