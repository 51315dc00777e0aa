"""CPU: tests/degrain_float_ref.py (the yardstick of the float DegrainN) anchored to tests/degrain_n_ref.py, which tests/test_degrain_n_ref.py
holds to the oracle: on float clips whose samples are integers the float cell must round to the integer filter's samples (overlap 0), or stay
within a derived bound of them (overlap > 0); and a flat clip must stay flat."""
import numpy as np
import pytest

import degrain_float_cases as fc
import degrain_n_cases as dc
import sample_range as sr
import super_float_ref as sf
import synth
import vector_fields

W, H = 96, 64


def _frames(gen, bits, n):
    if gen == "texture":
        return synth.survey_clip(W, H, bits, n)
    return sr.make(gen, W, H, bits, n, **(dict(motion=(1, 0)) if gen == "rails" else {}))


def _both(oracle, gen, bits, radius, akw, pel, dkw=None):
    """-> (integer restatement's planes, float restatement's planes) of the middle frame of 2 * radius + 1"""
    # (checker: the search cannot follow it; thresholds at their maxima keep every reference in the blend, tests/sample_range.py)
    dkw = dict(sr.CHECKER_BLEND) if gen == "checker" else (dkw or {})
    frames = _frames(gen, bits, 2 * radius + 1)
    osup, sfr, ad, nrefs, blobs = fc.oracle_job(oracle, frames, W, H, bits, radius, radius, akw, dict(pel=pel))
    thl, thc = dc.tables(ad, radius, dkw)
    want = dc.restatement(oracle, radius, ad, thl, thc, dkw).frame(frames[radius], [sfr[n] for n in nrefs], blobs)
    fsup = [[p.astype(np.float32) for p in sfr[n]] for n in nrefs]
    ref = fc.restatement(oracle, radius, ad, thl, thc, dkw)
    got = ref.frame(fc.integer_valued(frames)[radius], fsup, blobs)
    assert np.count_nonzero(ref.plan[0][1]) > 0  # (some reference carries a weight)
    return want, got


@pytest.mark.parametrize("radius", [1, 3, 7])
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("gen", ["rails", "checker", "texture"])
def test_without_overlap_the_float_cell_rounds_to_the_integer_filter(oracle, gen, bits, radius):
    """S = WSrc * s + sum of w * ref is an integer of at most 256 * 65535 < 2^24: exact in float32, as is S * (1 / 256); the integer filter's
    (128 + S) >> 8 is floor(S / 256 + 0.5)"""
    want, got = _both(oracle, gen, bits, radius, dict(blksize=8, overlap=0), 1, dict(thsad=1200 if radius == 7 else 400))
    for p in range(3):
        assert got[p].dtype == np.float32
        assert np.array_equal(np.floor(got[p].astype(np.float64) + 0.5).astype(want[p].dtype), want[p]), p


@pytest.mark.parametrize("akw", [dict(blksize=8, overlap=4), dict(blksize=16, overlap=8)], ids=["8/4", "16/8"])
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("gen", ["rails", "checker", "texture"])
def test_with_overlap_the_float_cell_stays_within_the_bound(oracle, gen, bits, akw):
    """|float - integer| <= 1.13 + peak / 2048 + the float rounding of peak: 1.25 at 8 bits, 33.2 at 16.
    The integer filter rounds a block's value V to an integer (error <= 0.5, weighted by the windows, whose total is <= 2049 / 2048: 0.5003),
    drops up to one unit in each of the <= 4 products' >> 6 (4 units of 1 / 32 after ToPixels' >> 5: 0.125) and rounds in ToPixels (0.5): 1.1253
    from sum(V * win) / 2048.  The float filter divides by the windows' own total, 2047..2049, instead of 2048: |V| * |1 - 2048 / wsum| <= peak / 2047
    ... the clamp at peak only moves the integer result towards the float one.  Float rounding: radius 3 gives at most 6 products and 6 sums in a
    block's value, one product for the source, a product and a sum per covering block and one division -- at most 22 operations per block chain, each
    off by at most 2^-24 of a value <= peak * 2049 / 2048; 32 * peak * 2^-24 covers them (0.125 at 16 bits, 0.0005 at 8)."""
    peak = (1 << bits) - 1
    bound = 1.13 + peak / 2048.0 + 32 * peak * 2.0 ** -24
    assert abs(bound - (1.25 if bits == 8 else 33.2)) < 0.06
    want, got = _both(oracle, gen, bits, 3, akw, 2)
    for p in range(3):
        err = float(np.abs(got[p].astype(np.float64) - want[p].astype(np.float64)).max())
        print("plane %d: max |float - integer| = %.4f (bound %.4f)" % (p, err, bound))
        assert err <= bound, p
    assert not np.array_equal(want[0], _frames(gen, bits, 7)[3][0])  # (the filter does change the frame)


@pytest.mark.parametrize("akw,radius", [(dict(blksize=8, overlap=4), 1), (dict(blksize=16, overlap=8), 3), (dict(blksize=8, overlap=0), 3)], ids=["8/4-r1", "16/8-r3", "8/0-r3"])
def test_a_flat_clip_stays_flat(oracle, akw, radius):
    """one value per plane, vectors on the limits of their legal rectangles and in between, every reference with a weight: |out - c| <= one ulp
    of c per covering block (4 with overlap, 1 without)"""
    n = 2 * radius + 1
    flat8 = [[np.full((H >> (1 if p else 0), W >> (1 if p else 0)), 128, np.uint8) for p in range(3)] for _ in range(n)]
    osup, sfr, ad, nrefs, blobs = fc.oracle_job(oracle, flat8, W, H, 8, radius, radius, akw, dict(pel=1))
    blobs = [vector_fields.limits(b, ad, 40 + r) for r, b in enumerate(blobs)]
    thl, thc = dc.tables(ad, radius, {})
    cover = 4 if akw["overlap"] else 1
    for values in [(0.25, -0.5, 1.0), (0.1, 0.1, -0.1), (1.0, 0.25, 0.1)]:
        src = [np.full(flat8[0][p].shape, values[p], np.float32) for p in range(3)]
        sup, _ = sf.frame(src, pel=1)
        ref = fc.restatement(oracle, radius, ad, thl, thc, {})
        out = ref.frame(src, [sup] * (2 * radius), blobs)
        assert np.all(ref.plan[0][1] > 0)
        for p in range(3):
            c = np.float32(values[p])
            err = float(np.abs(out[p].astype(np.float64) - float(c)).max())
            print("c = %g: max |out - c| = %.3g = %.2f ulp" % (values[p], err, err / float(np.spacing(np.abs(c)))))
            assert err <= cover * float(np.spacing(np.abs(c))), (values[p], p)


def test_what_is_passed_through_is_the_source_bit_for_bit(oracle):
    frames = dc.clip(W, H, 16, 3)
    osup, sfr, ad, nrefs, blobs = fc.oracle_job(oracle, frames, W, H, 16, 1, 1, dict(blksize=16, overlap=8), dict(pel=1))
    thl, thc = dc.tables(ad, 1, {})
    src = fc.float_clip(frames, 16)[1]
    fsup = [[p.astype(np.float32) / np.float32(65535) for p in sfr[n]] for n in nrefs]
    # plane=0: chroma untouched
    out = fc.restatement(oracle, 1, ad, thl, thc, dict(plane=0)).frame(src, fsup, blobs)
    assert np.array_equal(out[1].view(np.uint32), src[1].view(np.uint32)) and not np.array_equal(out[0], src[0])
    # no usable reference: every plane, also under overlap
    dead = [vector_fields.invalid(b, ad) for b in blobs]
    out = fc.restatement(oracle, 1, ad, thl, thc, {}).frame(src, fsup, dead)
    assert all(np.array_equal(out[p].view(np.uint32), src[p].view(np.uint32)) for p in range(3))
    out = fc.restatement(oracle, 1, ad, thl, thc, {}).frame(src, [None, None], blobs)
    assert all(np.array_equal(out[p].view(np.uint32), src[p].view(np.uint32)) for p in range(3))
    # limit 0 returns the source's values
    out = fc.restatement(oracle, 1, ad, thl, thc, dict(limit=0)).frame(src, fsup, blobs)
    assert all(np.array_equal(out[p], src[p]) for p in range(3))
    lim = fc.restatement(oracle, 1, ad, thl, thc, dict(limit=10, limitc=5)).frame(src, fsup, blobs)
    assert float(np.abs(lim[0] - src[0]).max()) <= 10 / 255.0 + 1e-6 and float(np.abs(lim[1] - src[1]).max()) <= 5 / 255.0 + 1e-6
