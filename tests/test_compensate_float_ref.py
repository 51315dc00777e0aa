"""CPU: tests/compensate_float_ref.py (the yardstick of the float Compensate / CompensateN) anchored to the oracle.  It is fed the oracle's integer
super frames converted to float32 (integer-valued samples; only their level-0 rows are read) and blobs from oracle.Analyse.

Without overlap every output sample is a copy, so the restatement must give oracle.Compensate's samples exactly.  With overlap it must stay
within a bound of them:

    integer   out = min(peak, (sum over the <= 4 covering blocks of ((v * win) >> 6) + 16) >> 5)
    float     out = (sum of v * win) / wsum, wsum the total of the same window weights

    With E = (sum of v * win) / 2048: each >> 6 drops less than one unit of the accumulator, which is 1 / 32 of an output unit after the >> 5 --
    four terms: 0.125; the + 16 and >> 5 round once: 0.5.  So |integer - E| <= 0.625 (the clamp at peak only moves the integer result towards the
    float one: E exceeds peak only where wsum is 2049, and the float result never exceeds peak).  The float filter divides by wsum, which differs
    from 2048 by at most 1 (asserted on every case: 2047..2049, the range include/mvtools_amd.h gives for DegrainN): |S / wsum - S / 2048| =
    (S / wsum) * |2048 - wsum| / 2048 <= peak / 2048.  Float rounding: the four products are off by 2^-24 of their values, together 2^-24 of a sum
    of at most peak * 2049; the three sums that follow the first (0 + x is exact) and the division are each off by 2^-24 of a value of at most
    that size: five operations at peak * 2049 / 2048 output units.

    bound = 0.625 + peak / 2048 + 5 * peak * (2049 / 2048) * 2^-24      (0.7496 at 8 bits, 32.64 at 16)

A flat clip stays flat to one ulp per covering block, negative and overshooting samples come through unclamped, and every copy is bit for bit."""
import numpy as np
import pytest

import compensate_float_cases as cc
import compensate_float_ref as cf
import degrain_n_cases as dc
import pipeline as pl
import vector_fields

F = np.float32
B80, B160, B84, B168, B42 = dict(blksize=8, overlap=0), dict(blksize=16, overlap=0), dict(blksize=8, overlap=4), dict(blksize=16, overlap=8), dict(blksize=4, overlap=2)
_jobs = {}


def _job(oracle, w, h, bits, skw, akw, isb=1, delta=1, fmt="420", n=4):
    """-> (oracle super, integer super frames, float32 super frames, analysis data, blobs[frame]) of a clip; blobs of the frames whose reference
    lies outside the clip are the oracle's invalid blobs"""
    key = (w, h, bits, tuple(sorted(skw.items())), tuple(sorted(akw.items())), isb, delta, fmt, n)
    if key not in _jobs:
        frames = dc.clip(w, h, bits, n, fmt)
        osup = oracle.Super(w, h, bits, **dict(dc.FORMATS[fmt], **skw))
        osf = [osup.frame(f) for f in frames]
        oan = oracle.Analyse(osup, num_frames=n, isb=isb, delta=delta, **akw)
        nref = lambda m: m + delta if isb else m - delta
        blobs = [oan.frame(osf[m], osf[nref(m)] if 0 <= nref(m) < n else None) for m in range(n)]
        fsf = [[p.astype(F) for p in fr] for fr in osf]
        _jobs[key] = (osup, osf, fsf, oan.ad, blobs, nref, frames)
    return _jobs[key]


def _exact(got, want, what):
    for p in range(len(want)):
        assert got[p].dtype == F
        assert pl.first_diff(got[p], want[p].astype(F)) == "", "%s plane %d" % (what, p)


@pytest.mark.parametrize("w,h,bits,skw,akw,ckw,isb,delta", [
    (96, 64, 8, dict(pel=1), B80, {}, 1, 1),
    (96, 64, 16, dict(pel=2), B160, dict(thsad=250), 0, 2),          # a thsad where blocks fall back; a forward field at distance 2
    (96, 64, 8, dict(pel=4), B80, dict(thsad=250, time=50.0), 1, 1),
    (96, 64, 16, dict(pel=2), B80, dict(time=50.0), 0, 1),
    (104, 70, 8, dict(pel=2), B160, dict(thsad=250, scbehavior=0), 1, 1),   # strips right and below that no block covers
    (104, 70, 16, dict(pel=1), B160, dict(thsad=250, scbehavior=1), 1, 1),
], ids=["pel1", "pel2-thsad-fw2", "pel4-thsad-time50", "pel2-time50", "strips-scb0", "strips-scb1"])
def test_without_overlap_it_is_the_oracles_compensate(oracle, w, h, bits, skw, akw, ckw, isb, delta):
    osup, osf, fsf, ad, blobs, nref, _ = _job(oracle, w, h, bits, skw, akw, isb, delta)
    ref = cc.restatement(oracle, ad, ckw)
    oc = oracle.Compensate(osup, ad, **ckw)
    fell_back = 0
    for m in range(len(osf)):
        r = nref(m)
        inside = 0 <= r < len(osf)
        want = oc.frame(osf[m], osf[r] if inside else None, blobs[m])
        _exact(ref.field(fsf[m], fsf[r] if inside else None, blobs[m]), want, "frame %d" % m)     # (both clip ends: a reference outside the clip)
        if inside:
            assert ref.from_ref is not None and ref.from_ref.any()
            fell_back += int((~ref.from_ref).sum())
            assert not np.array_equal(want[0], osup.finest(osf[m])[0][:h, :w]) or skw.get("pel", 2) != 1
    if "thsad" in ckw:
        assert fell_back > 0, "no block fell back on the source at this thsad"


@pytest.mark.parametrize("scbehavior", [0, 1])
@pytest.mark.parametrize("akw", [B80, B84], ids=["8/0", "8/4"])
def test_a_crafted_scene_change_per_scbehavior(oracle, akw, scbehavior):
    """one block too many above thscd1 (tests/vector_fields.py scene_count): the output is the reference frame at scbehavior 0, the source at 1 --
    copies, so exact with overlap too; with one block fewer the field is used"""
    osup, osf, fsf, ad, blobs, nref, frames = _job(oracle, 96, 64, 16, dict(pel=2), akw)
    th, s1, s2 = vector_fields.scaled_thresholds(ad, 10000)
    ckw = dict(scbehavior=scbehavior)
    ref, oc = cc.restatement(oracle, ad, ckw), oracle.Compensate(osup, ad, **ckw)
    over = vector_fields.scene_count(blobs[1], ad, 77, s1, s2 + 1, th)
    got = ref.field(fsf[1], fsf[2], over)
    _exact(got, oc.frame(osf[1], osf[2], over), "scene change")
    _exact(got, frames[1] if scbehavior else frames[2], "the frame itself")
    on = vector_fields.scene_count(blobs[1], ad, 77, s1, s2, th)
    assert ref.usable(fsf[2], on) and not ref.usable(fsf[2], over) and not ref.usable(None, on)


@pytest.mark.parametrize("w,h,bits,skw,akw,ckw", [
    (96, 64, 8, dict(pel=2), B84, dict(thsad=250)),
    (96, 64, 16, dict(pel=2), B84, dict(thsad=250)),
    (96, 64, 16, dict(pel=1), B168, {}),
    (96, 64, 8, dict(pel=4), B168, dict(time=50.0)),
    (96, 64, 16, dict(pel=2), B42, dict(thsad=250)),
    (104, 70, 16, dict(pel=2), B168, dict(thsad=250, scbehavior=0)),
    (70, 54, 8, dict(pel=2), dict(blksize=16, blksizev=8, overlap=8, overlapv=4), {}),
], ids=["8bit-8/4", "16bit-8/4", "16bit-16/8-pel1", "8bit-16/8-pel4-time50", "16bit-4/2", "16bit-16/8-strips", "8bit-16x8"])
def test_with_overlap_it_stays_within_the_bound(oracle, w, h, bits, skw, akw, ckw):
    osup, osf, fsf, ad, blobs, nref, _ = _job(oracle, w, h, bits, skw, akw)
    peak = (1 << bits) - 1
    bound = cc.bound(peak)
    assert abs(bound - (0.7496 if bits == 8 else 32.64)) < 0.01
    ref, oc = cc.restatement(oracle, ad, ckw), oracle.Compensate(osup, ad, **ckw)
    worst = 0.0
    for m in range(len(osf) - 1):
        want = oc.frame(osf[m], osf[m + 1], blobs[m])
        got = ref.field(fsf[m], fsf[m + 1], blobs[m])
        for p in range(3):
            assert got[p].dtype == F and got[p].shape == want[p].shape
            err = float(np.abs(got[p].astype(np.float64) - want[p].astype(np.float64)).max())
            worst = max(worst, err)
            assert err <= bound, "frame %d plane %d: %.4f > %.4f" % (m, p, err, bound)
    print("max |float - integer| = %.4f (bound %.4f), wsum %d..%d" % (worst, bound, ref.wsum_range[0], ref.wsum_range[1]))
    assert 2047 <= ref.wsum_range[0] and ref.wsum_range[1] <= 2049


@pytest.mark.parametrize("akw,cover", [(B84, 4), (B168, 4), (B80, 1)], ids=["8/4", "16/8", "8/0"])
def test_a_flat_clip_stays_flat(oracle, akw, cover):
    """one value per plane, vectors on the limits of their legal rectangles and in between: |out - c| <= one ulp of c per covering block"""
    import super_float_ref as sf
    osup, osf, fsf, ad, blobs, nref, _ = _job(oracle, 96, 64, 8, dict(pel=1), akw)
    crafted = vector_fields.limits(blobs[0], ad, 40)
    for values in [(0.25, -0.5, 1.0), (0.1, 0.1, -0.1), (1.0, 0.25, 0.1), (1.3, -0.2, 0.7)]:
        src = [np.full((64 >> (1 if p else 0), 96 >> (1 if p else 0)), values[p], F) for p in range(3)]
        sup, _ = sf.frame(src, pel=1)
        out = cc.restatement(oracle, ad, {}).field(sup, sup, crafted)
        for p in range(3):
            c = F(values[p])
            err = float(np.abs(out[p].astype(np.float64) - float(c)).max())
            assert err <= cover * float(np.spacing(np.abs(c))), (values[p], p, err)
            if cover == 1:
                assert np.array_equal(out[p].view(np.uint32), src[p].view(np.uint32))


@pytest.mark.parametrize("akw", [B84, B80], ids=["8/4", "8/0"])
def test_negative_and_overshooting_samples_come_through_unclamped(oracle, akw):
    """the integer-valued frames scaled and shifted: luma -0.2 .. 1.3, chroma centred on 0 and beyond +-0.5; the filter is linear up to rounding,
    so the result is the scaled and shifted integer-valued result to within float rounding -- and leaves 0 .. 1 where that does"""
    osup, osf, fsf, ad, blobs, nref, frames = _job(oracle, 96, 64, 8, dict(pel=2), akw)
    lo = [min(float(fr[p].min()) for fr in frames) for p in range(3)]
    hi = [max(float(fr[p].max()) for fr in frames) for p in range(3)]
    span = [1.5, 1.4, 1.4]
    a = [F(span[p] / (hi[p] - lo[p])) for p in range(3)]
    b = [F((-0.2 if p == 0 else -0.7) - lo[p] * float(a[p])) for p in range(3)]
    moved = [[fr[p] * a[p] + b[p] for p in range(3)] for fr in fsf]
    ref = cc.restatement(oracle, ad, dict(thsad=250))
    plain, got = ref.field(fsf[1], fsf[2], blobs[1]), ref.field(moved[1], moved[2], blobs[1])
    for p in range(3):
        want = plain[p].astype(np.float64) * float(a[p]) + float(b[p])
        assert float(np.abs(got[p] - want).max()) <= 1e-5
        assert got[p].min() < (0.0 if p == 0 else -0.5) and got[p].max() > (1.0 if p == 0 else 0.5)


def test_copies_are_bit_for_bit(oracle):
    """float samples that are not integers' images, with a payload in their low bits: the centre, an unusable field, the strips and blocks side by
    side are the very bits of the frame they come from"""
    import degrain_float_cases as fc
    import super_float_ref as sf
    w, h = 104, 70
    osup, osf, _, ad, blobs, nref, frames = _job(oracle, w, h, 16, dict(pel=1), B160)
    fl = fc.float_clip(frames, 16, seed=3)
    fsf = [sf.frame(f, pel=1)[0] for f in fl]
    bits = lambda planes: [np.ascontiguousarray(p).view(np.uint32) for p in planes]
    ref = cc.restatement(oracle, ad, dict(thsad=250))
    out = ref.job(1, fsf[1], [fsf[2], fsf[0]], [blobs[1], blobs[1]])
    assert all(np.array_equal(bits(out[1])[p], bits(fl[1])[p]) for p in range(3))                    # the centre
    dead = vector_fields.invalid(blobs[1], ad)
    for scb, want in ((0, fl[2]), (1, fl[1])):
        r = cc.restatement(oracle, ad, dict(scbehavior=scb))
        assert all(np.array_equal(bits(r.field(fsf[1], fsf[2], dead))[p], bits(want)[p]) for p in range(3))
        assert all(np.array_equal(bits(r.field(fsf[1], None, blobs[1]))[p], bits(fl[1])[p]) for p in range(3))
        strips = r.field(fsf[1], fsf[2], blobs[1])
        assert np.array_equal(bits(strips)[0][:, 96:], bits(want)[0][:, 96:]) and np.array_equal(bits(strips)[0][64:], bits(want)[0][64:])
    # blocks side by side: every output sample is some sample of the two super frames, bit for bit
    got = ref.field(fsf[1], fsf[2], blobs[1])
    pool = np.union1d(bits(fsf[1])[0].ravel(), bits(fsf[2])[0].ravel())
    assert np.isin(bits(got)[0], pool).all() and not np.array_equal(got[0], fl[1][0])
