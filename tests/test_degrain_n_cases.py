"""CPU: the cases of tests/test_gpu_degrain_n.py test what they claim.  Through the oracle's search alone (whose vectors the GPU search
reproduces bit for bit): in every case that is compared with the restatement beyond radius 6, at least half of the (block, reference) pairs
beyond distance 6 carry a weight and at least a fiftieth carry none -- a DegrainN that ignored the far references, or one that never dropped
any, could not pass them.  And the clip of identical frames gives the weights its test names."""
import numpy as np
import pytest

import degrain_n_cases as dc


CASES = [(c, None) for c in dc.LARGE_CASES] + [(dc.RANGE_GEO + (8, {}), gen) for gen in dc.RANGE_GENS]


@pytest.mark.parametrize("case,gen", CASES, ids=lambda v: v if v is None or isinstance(v, str) else dc.case_id(v))
def test_far_references_are_mostly_used_and_sometimes_not(oracle, case, gen):
    fmt, w, h, bits, skw, akw, radius, dkw = case
    n = 2 * radius + 1
    frames = dc.range_clip(gen, n) if gen else dc.clip(w, h, bits, n, fmt)
    osup = oracle.Super(w, h, bits, **dict(dc.FORMATS[fmt], **skw))
    osf = [osup.frame(f) for f in frames]
    refs, blobs = [], []
    for r, isb, d, nref in dc.neighbours(radius, radius, n):
        oan = oracle.Analyse(osup, isb=isb, delta=d, **akw)
        blobs.append(oan.frame(osf[radius], osf[nref]))
        refs.append(osf[nref])
    ref = dc.restatement(oracle, radius, oan.ad, *dc.tables(oan.ad, radius, dkw), dkw, gray=fmt == "gray")
    ref.weigh(refs, blobs)
    ok, what = dc.far_shares_ok(ref)
    assert ok, what
    if gen:  # ... and the blend holds samples on both rails
        out = ref.frame(frames[radius], refs, blobs)
        assert np.count_nonzero(out[0] != frames[radius][0]) > 1000
        assert gen == "step" or (np.count_nonzero(out[0] == 0) > 1000 and np.count_nonzero(out[0] == 65535) > 1000)
        assert gen == "rails" or (frames[radius][0].min() < 2100 and frames[radius + 1][0].max() > 63400)


def test_identical_frames_give_48_weights_of_5(oracle):
    fmt, w, h, bits, skw, akw = dc.A
    frame = dc.clip(w, h, bits, 1, fmt, noise=0)[0]
    osup = oracle.Super(w, h, bits)
    sf = osup.frame(frame)
    blobs = [oracle.Analyse(osup, isb=isb, delta=d, **akw).frame(sf, sf) for r, isb, d, _ in dc.neighbours(24, 24, 49)]
    ad = oracle.Analyse(osup, isb=1, **akw).ad
    ref = dc.restatement(oracle, 24, ad, *dc.tables(ad, 24, {}), {})
    out = ref.frame(frame, [sf] * 48, blobs)
    for c in range(2):
        assert np.all(ref.plan[c][0] == 16) and np.all(ref.plan[c][1] == 5)
    for p in range(3):
        assert np.array_equal(out[p], frame[p])
