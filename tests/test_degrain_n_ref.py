"""CPU: the numpy restatement of Degrain at any radius (tests/degrain_n_ref.py) against the oracle, byte for byte, at the radii the oracle
has -- 1, 2, 3 and 6.  Beyond 6 the oracle's arrays end and the restatement is what mv.DegrainN is held to (tests/test_gpu_degrain_n.py), so
it has to earn that here: every path it has (overlap and none, uncovered strips, sub-pel planes of pel 1 and 2, 8 / 10 / 16 bits, 4:2:0 /
4:4:4 / Gray, the plane selection, the limits, references outside the clip) on vectors the oracle searched itself."""
import numpy as np
import pytest

import degrain_n_cases as dc
import pipeline as pl

MAXR = 6
CASES = [
    # fmt, w, h, bits, super kwargs, analyse kwargs, degrain kwargs, target frame (None: the middle one)
    ("420", 128, 96, 8, {}, dict(blksize=8, overlap=4), {}, None),                       # plane 4
    ("420", 204, 116, 16, {}, dict(blksize=16, overlap=8), {}, None),                    # a 4-sample strip right and below that no block covers
    ("420", 160, 96, 8, dict(pel=1), dict(blksize=8, overlap=0), {}, None),
    ("420", 144, 80, 10, {}, dict(blksize=16, overlap=4), {}, None),                     # steps of 12 (chroma: 6)
    ("444", 128, 96, 8, {}, dict(blksize=8, overlap=4), dict(plane=0), None),
    ("gray", 128, 96, 16, {}, dict(blksize=8, overlap=4), dict(limit=300), None),
    ("420", 128, 96, 8, {}, dict(blksize=8, overlap=4), dict(limit=2, limitc=1, thsadc=250), 0),   # frame 0: every forward reference lies outside the clip
]
_cache = {}


def _searched(oracle, case):
    """per case, once: the clip, its super frames and the oracle's vectors at delta 1..6 for the target frame"""
    if case not in _cache:
        fmt, w, h, bits, skw, akw, _, target = CASES[case]
        n = 2 * MAXR + 1
        target = MAXR if target is None else target
        frames = dc.clip(w, h, bits, n, fmt, seed=41 + case)
        osup = oracle.Super(w, h, bits, **dict(dc.FORMATS[fmt], **skw))
        osf = [osup.frame(f) for f in frames]
        refs, blobs = [], []
        for r, isb, d, nref in dc.neighbours(target, MAXR, n):
            oan = oracle.Analyse(osup, isb=isb, delta=d, **akw)
            blobs.append(oan.frame(osf[target], osf[nref] if nref is not None else None))
            refs.append(osf[nref] if nref is not None else None)
        _cache[case] = (frames[target], osup, oan.ad, refs, blobs)
    return _cache[case]


@pytest.mark.parametrize("radius", [1, 2, 3, 6])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_restatement_is_the_oracle_up_to_radius_6(oracle, case, radius):
    fmt, _, _, _, _, _, dkw, target = CASES[case]
    src, osup, ad, refs, blobs = _searched(oracle, case)
    refs, blobs = refs[:2 * radius], blobs[:2 * radius]
    odg = oracle.Degrain(radius, osup, ad, **dkw)
    want = odg.frame(src, refs, blobs)
    ref = dc.restatement(oracle, radius, ad, [odg.d.thSAD[0]] * radius, [odg.d.thSAD[1]] * radius, dkw, gray=fmt == "gray")
    assert (ref.nscd1, ref.nscd2) == (odg.d.nSCD1, odg.d.nSCD2)
    got = ref.frame(src, refs, blobs)
    assert len(got) == len(want)
    for p in range(len(want)):
        assert pl.first_diff(got[p], want[p]) == "", "plane %d" % p
    if target == 0:
        assert all(refs[r] is None for r in range(1, 2 * radius, 2)) and np.all(ref.plan[0][1][:, 1::2] == 0)
    else:
        assert np.count_nonzero(ref.plan[0][1]) > 0 and not np.array_equal(got[0], src[0])  # the case filters something
