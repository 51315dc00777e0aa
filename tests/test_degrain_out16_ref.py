"""CPU: the yardstick of mv.DegrainN's out16 (tests/degrain_out16_ref.py) against the oracle's 8-bit Degrain at the radii the oracle has --
1, 2, 3 and 6 -- on vectors the oracle searched itself, and the share condition of the GPU cases that tests/test_degrain_n_cases.py does not
already cover (tests/test_gpu_degrain_out16.py).

Blocks side by side: the 16-bit value of a sample is S = WSrc * src + sum of W_r * ref_r and the oracle's byte is (S + 128) >> 8, so
(out16 + 128) >> 8 must be the oracle's plane, byte for byte (a sample passed through is src << 8, and ((src << 8) + 128) >> 8 = src).

Overlapping blocks: the two pipelines round in different places and only a bound ties them; see test_overlap_within_the_rounding_bound."""
import numpy as np
import pytest

import degrain_n_cases as dc
import degrain_out16_ref as o16
import pipeline as pl

MAXR = 6
SIDE_BY_SIDE = [
    # fmt, w, h, super kwargs, analyse kwargs, degrain kwargs, target frame (None: the middle one)
    ("420", 160, 96, dict(pel=1), dict(blksize=8, overlap=0), {}, None),
    ("420", 132, 100, {}, dict(blksize=16, overlap=0), {}, None),          # a 4-sample strip right and below that no block covers
    ("444", 128, 96, {}, dict(blksize=8, overlap=0), dict(plane=0), None),
    ("gray", 128, 96, {}, dict(blksize=8, blksizev=4, overlap=0), {}, 0),  # frame 0: every forward reference lies outside the clip
]
OVERLAP = [
    ("420", 128, 96, {}, dict(blksize=8, overlap=4), {}, None),
    ("420", 204, 116, {}, dict(blksize=16, overlap=8), {}, None),          # uncovered strips
    ("420", 144, 80, dict(pel=1), dict(blksize=16, overlap=4), {}, None),  # steps of 12 (chroma: 6): samples under 1, 2 and 4 blocks
    ("444", 128, 96, {}, dict(blksize=8, blksizev=4, overlap=4, overlapv=2), dict(plane=0), 0),
]
# the windows (block width, height, overlaps) whose weights total 2048 on every sample; overInit rounds each window on its own
# (Overlap.cpp:40-125), and those of 16x16 / 8 and 8x4 / 4x2 total 2047..2049
EXACT_2048 = {(8, 8, 4, 4), (4, 4, 2, 2), (16, 16, 4, 4), (8, 8, 2, 2)}
_cache = {}


def _searched(oracle, case):
    """per case, once: the clip's target frame, the oracle's super clip, its analysis data, reference super frames and vectors at delta 1..6"""
    key = _key(case)
    if key not in _cache:
        fmt, w, h, skw, akw, _, target = case
        n = 2 * MAXR + 1
        target = MAXR if target is None else target
        frames = dc.clip(w, h, 8, n, fmt, seed=53 + (SIDE_BY_SIDE + OVERLAP).index(case))
        osup = oracle.Super(w, h, 8, **dict(dc.FORMATS[fmt], **skw))
        osf = [osup.frame(f) for f in frames]
        refs, blobs = [], []
        for r, isb, d, nref in dc.neighbours(target, MAXR, n):
            oan = oracle.Analyse(osup, isb=isb, delta=d, **akw)
            blobs.append(oan.frame(osf[target], osf[nref] if nref is not None else None))
            refs.append(osf[nref] if nref is not None else None)
        _cache[key] = (frames[target], osup, oan.ad, refs, blobs)
    return _cache[key]


def _key(case):
    return case[:3] + tuple(tuple(sorted(d.items())) for d in case[3:6]) + (case[6],)


def _both(oracle, case, radius):
    """-> (the oracle's 8-bit planes, the yardstick's 16-bit planes, the source planes, the yardstick)"""
    fmt, dkw = case[0], case[5]
    src, osup, ad, refs, blobs = _searched(oracle, case)
    refs, blobs = refs[:2 * radius], blobs[:2 * radius]
    odg = oracle.Degrain(radius, osup, ad, **dkw)
    want8 = odg.frame(src, refs, blobs)
    ref = o16.restatement(oracle, radius, ad, [odg.d.thSAD[0]] * radius, [odg.d.thSAD[1]] * radius, dkw, gray=fmt == "gray")
    assert (ref.nscd1, ref.nscd2) == (odg.d.nSCD1, odg.d.nSCD2) and ref.ad.bitsPerSample == 16 and ad.bitsPerSample == 8
    got16 = o16.frame(ref, src, refs, blobs)
    assert len(got16) == len(want8) and all(g.dtype == np.uint16 for g in got16)
    assert np.count_nonzero(ref.plan[0][1]) > 0 and not np.array_equal(want8[0], src[0])  # the case filters something
    return want8, got16, src, ref


@pytest.mark.parametrize("radius", [1, 2, 3, 6])
@pytest.mark.parametrize("case", SIDE_BY_SIDE, ids=lambda c: "%s-%dx%d" % c[:3])
def test_side_by_side_rounds_to_the_oracles_bytes(oracle, case, radius):
    want8, got16, src, ref = _both(oracle, case, radius)
    for p in range(len(want8)):
        assert pl.first_diff(((got16[p].astype(np.int64) + 128) >> 8).astype(np.uint8), want8[p]) == "", "plane %d" % p
        assert int(got16[p].max()) <= 65280
    assert np.count_nonzero(got16[0] & 255) > got16[0].size // 4  # ... and carries more than the bytes: low bits that are not 0
    if case[5].get("plane") == 0:
        assert np.array_equal(got16[1], src[1].astype(np.uint16) << 8)  # a plane that is not processed


@pytest.mark.parametrize("radius", [1, 2, 3, 6])
@pytest.mark.parametrize("case", OVERLAP, ids=lambda c: "%s-%dx%d" % c[:3])
def test_overlap_within_the_rounding_bound(oracle, case, radius):
    """-256 <= out16 - 256 * out8 <= 288 on every sample.  With S_b the exact value of block b (an integer, 0..65280), w_b >= 0 the window
    weights of the <= 4 blocks covering the sample, which total T = 2048, and E = sum of S_b * w_b / 2048:

      16-bit   acc = sum of floor(S_b * w_b / 64): each floor loses less than 1, so 32 E - 4 < acc <= 32 E; out16 = floor((acc + 16) / 32),
               which loses less than 1 again: E - 1/8 + 1/2 - 1 < out16 <= E + 1/2.
      8-bit    v_b = floor((S_b + 128) / 256) = S_b / 256 + d_b with -1/2 < d_b <= 1/2; the weighted mean of the d_b, D, lies in the same
               interval.  The same two steps on v_b: E / 256 + D - 5/8 < out8 <= E / 256 + D + 1/2, so E - 288 < 256 * out8 <= E + 256.
      neither clamp binds: (255 * 2048 / 64 + 16) >> 5 = 255 and (65280 * 32 + 16) >> 5 = 65280, and the 8-bit accumulator stays below 2^16.

    Hence -5/8 - 256 < out16 - 256 * out8 < 1/2 + 288, integers: -256..288 (per covering block each pipeline loses less than 1/32, half a step
    in the final rounding, and the 8-bit one another half step of 256 in its >> 8).  Samples that are passed through differ by 0.

    T = 2048 is asserted on the windows of EXACT_2048, and every case here uses at least one of them or says why not.  Some of the reference's
    windows total 2047 or 2049 on some samples (asserted: nothing else).  Both pipelines use the same windows, so E keeps its meaning; only
    |D| <= T / 4096 grows, by 256 / 4096 = 1/16 of an output step: -256 - 11/16 < out16 - 256 * out8 < 288 + 9/16 -- the same integers.  The
    clamps still do not bind: (65280 * 2049 / 64 + 16) >> 5 = 65311 and (8163 + 16) >> 5 = 255."""
    want8, got16, src, ref = _both(oracle, case, radius)
    ad = ref.ad
    assert ref.win, "no window was used"
    for (bw, bh, ox, oy), win in ref.win.items():
        total, smallest = o16.window_totals(win, ad.nBlkX, ad.nBlkY, bw, bh, ox, oy)
        assert smallest >= 0 and int(total.min()) >= 2047 and int(total.max()) <= 2049, (bw, bh, ox, oy)
        assert (bw, bh, ox, oy) not in EXACT_2048 or np.all(total == 2048), (bw, bh, ox, oy)
    assert case[0] == "444" or set(ref.win) & EXACT_2048  # (the 4:4:4 case is there for its 8x4 blocks: 2048..2049)
    lo, hi = 0, 0
    for p in range(len(want8)):
        d = got16[p].astype(np.int64) - 256 * want8[p].astype(np.int64)
        assert -256 <= int(d.min()) and int(d.max()) <= 288, "plane %d: %d..%d" % (p, d.min(), d.max())
        lo, hi = min(lo, int(d.min())), max(hi, int(d.max()))
    assert lo < -64 and hi > 64  # the 16-bit planes are not the 8-bit ones shifted


# ------------------------------------------------------------------------------------------------ the GPU cases beyond radius 6 that are new here

NEW_FAR = [
    (("422", 160, 96, 8, {}, dc.B168, 7, {}), None),
    (("420", 204, 116, 8, {}, dc.B168, 8, {}), None),
    (dc.A + (8, {}), "step"),
    (dc.A + (8, {}), "rails"),
]


def range_clip8(gen, n):
    """the ends of the 8-bit range on A's geometry, as degrain_n_cases.range_clip has them at 16 bits"""
    import sample_range as sr
    _, w, h, _, _, _ = dc.A
    return sr.step(w, h, 8, n, 0, 255) if gen == "step" else sr.rails(w, h, 8, n, motion=(1, 0))


@pytest.mark.parametrize("case,gen", NEW_FAR, ids=lambda v: v if v is None or isinstance(v, str) else dc.case_id(v))
def test_new_far_cases_use_most_far_references_and_drop_some(oracle, case, gen):
    """as tests/test_degrain_n_cases.py shows for the rows of LARGE_CASES (whose 8-bit rows the out16 suite runs with the same clips, vectors and
    thresholds): through the oracle's search alone, beyond distance 6 at least half of the pairs carry a weight and a fiftieth none"""
    fmt, w, h, bits, skw, akw, radius, dkw = case
    n = 2 * radius + 1
    frames = range_clip8(gen, n) if gen else dc.clip(w, h, bits, n, fmt)
    osup = oracle.Super(w, h, bits, **dict(dc.FORMATS[fmt], **skw))
    osf = [osup.frame(f) for f in frames]
    refs, blobs = [], []
    for r, isb, d, nref in dc.neighbours(radius, radius, n):
        oan = oracle.Analyse(osup, isb=isb, delta=d, **akw)
        blobs.append(oan.frame(osf[radius], osf[nref]))
        refs.append(osf[nref])
    ref = o16.restatement(oracle, radius, oan.ad, *dc.tables(oan.ad, radius, dkw), dkw)
    ref.weigh(refs, blobs)
    ok, what = dc.far_shares_ok(ref)
    assert ok, what
    if gen:  # the blend reaches both ends of the output's range: 0 and 255 << 8
        out = o16.frame(ref, frames[radius], refs, blobs)
        assert np.count_nonzero(out[0] != frames[radius][0].astype(np.uint16) << 8) > 1000
        assert gen == "step" or (np.count_nonzero(out[0] == 0) > 1000 and np.count_nonzero(out[0] == 65280) > 1000 and int(out[0].max()) == 65280)
