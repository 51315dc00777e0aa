"""CPU: tests/blockfps_float_ref.py (the yardstick of the float BlockFPS) anchored to the oracle.  It is fed the oracle's integer super frames
converted to float32 (integer-valued samples; only their level-0 rows are read), the integer clip converted likewise, and blobs from
oracle.Analyse -- searched, or crafted by tests/vector_fields.py so that the masks are neither empty nor saturated.

Exact anchors.  Modes 0, 1 and 2 without overlap: b * t + fw * (256 - t) is an integer below 2^24 at 16 bits (65535 * 256), so every float
product, the sum and the multiplication by 1 / 256 are exact and the float value is the rational E whose floor the integer filter's ">> 8"
(no rounding term) gives; floor commutes with the median of mode 1 and 2 because the other two operands are integers.  So floor(restatement)
is the oracle's sample.  Modes 5 and 8 without overlap: the value is mO / 255, so rint(restatement * 255) is the oracle's sample >> (bits - 8),
which pins usable, the occlusion / SAD masks, the padding, O = F * B / 255 and the upsizer.  The fallbacks are copies or the same exact blend.

The bound elsewhere, on integer-valued samples 0..peak (blockfps_float_cases.bound).  Write D = 255 / 256.
    ">> 8" against "* K"        floor(E) against E: 0 <= E - floor(E) <= D.
    "(N + 255) >> 8" against "N / 255", 0 <= N <= 255 * 255 (an 8-bit mask mix of samples 0..255):
                                (N + 255) / 256 - N / 255 = (65025 - N) / 65280 lies in [0, D], and the floor takes off [0, D]: the two differ
                                by at most D either way.  (At 16 bits the same difference reaches peak / 256: the float path is compared with
                                the integer one on samples 0..255 only.)
    modes 0, 1, 2               one stage: D.
    modes 3, 6                  bb and ff are each within D of the integer mixes; the time stage is a convex combination of them (still D) and
                                one floor (D): 2 D.
    modes 4, 7                  avg: (x + 255) >> 8 of an integer x / 256 is within D; m is within 2 D as above; the last mix is a convex
                                combination (2 D) and one "(N + 255) >> 8" against "N / 255" (D): 3 D.
    overlap                     the integer filter's overlap sum of its own block values against the float sum of the same values:
                                0.625 + peak / 2048 + 5 roundings (tests/test_compensate_float_ref.py derives it: four ">> 6" of 1 / 32 each, one
                                rounding of a half, wsum = 2048 +- 1); a convex combination of block values moves by no more than they do, so the
                                stages above add.  The 8-bit accumulator does not wrap: 4 * 255 * 2048 / 64 < 65536.
    float rounding              every rounded operation is off by 2^-24 of a value of at most 256 * peak before the exact scaling, peak * 256 /
                                255 in output units: 0 operations in modes 0..2 (exact, above), 11 in modes 3 / 6 (two mixes of 4, the time
                                stage's 3), 18 in modes 4 / 7 (3 for avg and 4 for the last mix more).
    bound = stages * D + ops * peak * (256 / 255) * 2^-24 [+ 0.625 + peak / 2048 + 5 * peak * (2049 / 2048) * 2^-24]
It is not a measured tolerance: 0.9961 / 1.9924 / 2.9886 without overlap at 8 bits, 1.7458 / 2.7420 / 3.7383 with; modes 0..2 with overlap at 16
bits 33.64."""
import numpy as np
import pytest

import blockfps_float_cases as bc
import degrain_float_cases as fc
import degrain_n_cases as dc
import pipeline as pl
import vector_fields

F = np.float32
B80, B160, B84, B168, B42 = dict(blksize=8, overlap=0), dict(blksize=16, overlap=0), dict(blksize=8, overlap=4), dict(blksize=16, overlap=8), dict(blksize=4, overlap=2)
_jobs = {}


class Job:
    """a clip of five frames with the oracle's super frames (integer and integer-valued float32) and both vector clips of every frame"""

    def __init__(self, oracle, w, h, bits, skw, akw, fmt="420", n=bc.NFRAMES):
        self.frames = dc.clip(w, h, bits, n, fmt)
        self.n, self.gray = n, fmt == "gray"
        self.osup = oracle.Super(w, h, bits, **dict(dc.FORMATS[fmt], **skw))
        self.osf = [self.osup.frame(f) for f in self.frames]
        self.fsf = [[p.astype(F) for p in fr] for fr in self.osf]
        self.fclip = fc.integer_valued(self.frames)
        abw, afw = oracle.Analyse(self.osup, num_frames=n, isb=1, **akw), oracle.Analyse(self.osup, num_frames=n, isb=0, **akw)
        self.adb, self.adf = abw.ad, afw.ad
        rb, rf = bc.vector_jobs(n)
        self.bw = [abw.frame(self.osf[m], self.osf[rb[m]] if rb[m] is not None else None) for m in range(n)]
        self.fw = [afw.frame(self.osf[m], self.osf[rf[m]] if rf[m] is not None else None) for m in range(n)]

    def crafted(self, recipe, bkw):
        """both vector clips rewritten by a recipe of tests/vector_fields.py (the blobs of frames whose reference lies outside the clip stay)"""
        rb, rf = bc.vector_jobs(self.n)
        bw = [bc.crafted(recipe, b, self.adb, 100 + m, bkw) if rb[m] is not None else b for m, b in enumerate(self.bw)]
        fw = [bc.crafted(recipe, b, self.adf, 200 + m, bkw) if rf[m] is not None else b for m, b in enumerate(self.fw)]
        return bw, fw


def _job(oracle, w, h, bits, skw, akw, fmt="420"):
    key = (w, h, bits, tuple(sorted(skw.items())), tuple(sorted(akw.items())), fmt)
    if key not in _jobs:
        _jobs[key] = Job(oracle, w, h, bits, skw, akw, fmt)
    return _jobs[key]


def _pair(oracle, j, bkw, bw=None, fw=None):
    """(oracle.BlockFPS, the restatement, want(n) -> the oracle's frame, got(n) -> the restatement's) at 24 -> 60"""
    bw, fw = bw or j.bw, fw or j.fw
    ob = oracle.BlockFPS(j.osup, j.adb, j.adf, j.n, 24, 1, num=60, den=1, **bkw)
    ref = bc.restatement(oracle, j.adb, j.adf, bkw, gray=j.gray)
    want = lambda n: ob.frame(n, j.frames, j.osf, bw, fw)
    got = lambda n: bc.want_frame(ref, ob.map, n, j.fclip, j.fsf, bw, fw)
    return ob, ref, want, got


def test_the_24_to_60_map_has_a_copy_and_both_kinds_of_fallback(oracle):
    j = _job(oracle, 96, 64, 8, dict(pel=2), B80)
    ob = oracle.BlockFPS(j.osup, j.adb, j.adf, j.n, 24, 1, num=60, den=1)
    assert ob.num_frames == 11
    assert [ob.map(n) for n in range(11)] == [(0, 1, 0), (0, 1, 102), (0, 1, 205), (1, 2, 51), (1, 2, 154), (2, 3, 0), (2, 3, 102), (2, 3, 205), (3, 4, 51),
                                              (3, 4, 154), (4, 5, 0)]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("w,h,bits,skw,akw", [(96, 64, 8, dict(pel=1), B80), (104, 70, 16, dict(pel=2), B160), (104, 70, 8, dict(pel=4), B160), (96, 64, 16, dict(pel=2), B80)],
                         ids=["8bit-pel1-8/0", "16bit-pel2-16/0-strips", "8bit-pel4-16/0-strips", "16bit-pel2-8/0"])
def test_modes_0_1_2_without_overlap_floor_to_the_oracle(oracle, w, h, bits, skw, akw, mode):
    j = _job(oracle, w, h, bits, skw, akw)
    for bw, fw in ((j.bw, j.fw), j.crafted("limits", {})):
        ob, ref, want, got = _pair(oracle, j, dict(mode=mode), bw, fw)
        moved = 0
        for n in range(ob.num_frames):
            wn, gn = want(n), got(n)
            for p in range(3):
                assert gn[p].dtype == F
                assert pl.first_diff(np.floor(gn[p]).astype(wn[p].dtype), wn[p]) == "", "output %d %s plane %d" % (n, ob.map(n), p)
            moved += not np.array_equal(wn[0], j.frames[min(ob.map(n)[0], j.n - 1)][0])
        assert moved >= 6


@pytest.mark.parametrize("mode,ml", [(5, 100.0), (5, 40.0), (8, 40.0), (8, 100.0)])
@pytest.mark.parametrize("w,h,bits,skw,akw,recipe", [(128, 112, 8, dict(pel=2), B80, "occlusion"), (104, 70, 16, dict(pel=2), B160, "limits"), (128, 112, 10, dict(pel=1), B80, "occlusion")],
                         ids=["8bit-8/0", "16bit-16/0-strips", "10bit-8/0"])
def test_modes_5_and_8_times_255_are_the_oracles_mask(oracle, w, h, bits, skw, akw, recipe, mode, ml):
    j = _job(oracle, w, h, bits, skw, akw)
    bkw = dict(mode=mode, ml=ml)
    bw, fw = j.crafted(recipe, bkw)
    ob, ref, want, got = _pair(oracle, j, bkw, bw, fw)
    covW, covH = j.adb.nBlkX * j.adb.nBlkSizeX, j.adb.nBlkY * j.adb.nBlkSizeY
    seen = set()
    for n in (1, 2, 3, 4):
        wn, gn = want(n), got(n)
        for p in range(3):
            cw, ch = (covW, covH) if p == 0 else (covW // 2, covH // 2)
            m = np.rint(gn[p][:ch, :cw].astype(np.float64) * 255).astype(np.int64)
            assert np.array_equal(m, wn[p][:ch, :cw].astype(np.int64) >> (bits - 8)), "output %d plane %d" % (n, p)
            assert np.array_equal(m.astype(F) / F(255.0), gn[p][:ch, :cw])
            assert np.array_equal(np.floor(gn[p]).astype(np.int64)[ch:], wn[p].astype(np.int64)[ch:])      # the strip below: the blend
            seen |= set(np.unique(m).tolist())
    assert len(seen) > 20, sorted(seen)    # (O = F * B / 255 seldom reaches 255)


BOUND_GEOS = [("8/4", 128, 96, 8, dict(pel=2), B84, "occlusion"), ("8/0", 128, 112, 8, dict(pel=2), B80, "occlusion"), ("16/8-strips", 104, 70, 8, dict(pel=1), B168, "limits"),
              ("16/0-pel4-strips", 104, 70, 8, dict(pel=4), B160, "limits"), ("4/2", 96, 64, 8, dict(pel=2), B42, "occlusion"), ("16bit-8/4", 104, 70, 16, dict(pel=2), B84, "limits")]
# modes 0..2 without overlap are exact (above); the mask mixes are compared on samples 0..255
BOUND_CASES = [g + (mode,) for g in BOUND_GEOS for mode in (3, 4, 6, 7, 0, 1, 2) if (mode >= 3 or g[5]["overlap"]) and (mode < 3 or g[3] == 8)]


@pytest.mark.parametrize("tag,w,h,bits,skw,akw,recipe,mode", BOUND_CASES, ids=["%s-mode%d" % (c[0], c[-1]) for c in BOUND_CASES])
def test_the_other_modes_stay_within_the_derived_bound(oracle, tag, w, h, bits, skw, akw, recipe, mode):
    overlap = akw["overlap"] > 0
    peak = (1 << bits) - 1
    bound = bc.bound(mode, overlap, peak)
    j = _job(oracle, w, h, bits, skw, akw)
    bkw = dict(mode=mode, ml=bc.crafted_ml(recipe, mode))
    bw, fw = j.crafted(recipe, bkw)
    ob, ref, want, got = _pair(oracle, j, bkw, bw, fw)
    worst = 0.0
    for n in (1, 2, 3, 4):
        wn, gn = want(n), got(n)
        for p in range(3):
            assert gn[p].dtype == F and gn[p].shape == wn[p].shape
            err = float(np.abs(gn[p].astype(np.float64) - wn[p].astype(np.float64)).max())
            worst = max(worst, err)
            assert err <= bound, "mode %d output %d plane %d: %.4f > %.4f" % (mode, n, p, err, bound)
        if mode >= 3:
            lo, hi = bc.mask_shares(ref)
            assert lo >= bc.SHARE and hi >= bc.SHARE, (n, lo, hi)
    print("mode %d: max |float - integer| = %.4f (bound %.4f)" % (mode, worst, bound))


def test_the_bound_is_the_derived_one():
    want = {(0, False, 255): 0.9961, (3, False, 255): 1.9924, (4, False, 255): 2.9886, (0, True, 255): 1.7458, (6, True, 255): 2.7420, (7, True, 255): 3.7383,
            (2, True, 65535): 33.64}
    for (mode, ov, peak), b in want.items():
        assert abs(bc.bound(mode, ov, peak) - b) < 0.006, (mode, ov, peak, bc.bound(mode, ov, peak))
    with pytest.raises(AssertionError):
        bc.bound(3, False, 65535)


# operations between a flat input and the output, each off by at most one ulp of the value: the time stage is 3 (two products, a sum; the scaling
# is exact), a mix 4, the overlap sum of four covering blocks 4 products, 4 sums and a division
OPS = {0: 3, 1: 3, 2: 3, 3: 7, 6: 7, 4: 11, 7: 11}


@pytest.mark.parametrize("mode", sorted(OPS))
@pytest.mark.parametrize("akw", [B84, B160], ids=["8/4", "16/0"])
def test_a_flat_clip_stays_flat(oracle, akw, mode):
    """one value per plane, vectors on the limits of their legal rectangles: |out - c| <= one ulp of c per operation (modes 5 and 8 write the mask,
    not the clip)"""
    import super_float_ref as sf
    j = _job(oracle, 96, 64, 8, dict(pel=1), akw)
    bkw = dict(mode=mode, ml=bc.crafted_ml("limits", mode))
    bw, fw = j.crafted("limits", bkw)
    ref = bc.restatement(oracle, j.adb, j.adf, bkw)
    ops = OPS[mode] + (9 if akw["overlap"] else 0)
    for values in [(0.25, -0.5, 1.0), (0.1, 0.1, -0.1), (1.3, -0.2, 0.7)]:
        src = [np.full((64 >> (1 if p else 0), 96 >> (1 if p else 0)), values[p], F) for p in range(3)]
        sup, _ = sf.frame(src, pel=1)
        for t in (1, 102, 128, 255):
            out = ref.frame(t, src, src, sup, sup, fw[2], bw[1])
            assert ref.masks is not None or mode < 3
            for p in range(3):
                c = F(values[p])
                err = float(np.abs(out[p].astype(np.float64) - float(c)).max())
                assert err <= ops * float(np.spacing(np.abs(c))), (values[p], t, p, err)


@pytest.mark.parametrize("akw", [B84, B160], ids=["8/4", "16/0"])
def test_fallbacks_clip_end_blend_and_time_0_are_exact(oracle, akw):
    """float samples that are not integers' images: a scene change (one block too many above thscd1), an invalid blob and the clip's end give
    clip_left bit for bit at blend 0 and (l * fu + r * ft) * K at blend 1; time256 0 and 256 are copies whatever the vectors; one block fewer
    above thscd1 and the frame is interpolated"""
    import super_float_ref as sf
    j = _job(oracle, 96, 64, 16, dict(pel=2), akw)
    fl = fc.float_clip(j.frames, 16, seed=3)
    fsf = [sf.frame(f, pel=2)[0] for f in fl]
    _, s1, s2 = vector_fields.scaled_thresholds(j.adb, 400)
    over = vector_fields.scene_count(j.bw[1], j.adb, 77, s1, s2 + 1, 400)
    on = vector_fields.scene_count(j.bw[1], j.adb, 77, s1, s2, 400)
    dead = vector_fields.invalid(j.fw[2], j.adf)
    bits = lambda planes: [np.ascontiguousarray(p).view(np.uint32) for p in planes]
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))
    for blend in (0, 1):
        ref = bc.restatement(oracle, j.adb, j.adf, dict(mode=3, blend=blend))
        t = 102
        mixed = [(fl[1][p] * F(256 - t) + fl[2][p] * F(t)) * F(1 / 256) for p in range(3)]
        for args in ((fsf[1], fsf[2], j.fw[2], over), (fsf[1], fsf[2], dead, j.bw[1]), (None, None, None, None)):
            out = ref.frame(t, fl[1], fl[2], *args)
            assert same(out, mixed if blend else fl[1])
        assert not same(mixed, fl[1])
        assert ref.usable(t, fsf[1], fsf[2], j.fw[2], on) and not ref.usable(t, fsf[1], fsf[2], j.fw[2], over)
        assert not same(ref.frame(t, fl[1], fl[2], fsf[1], fsf[2], j.fw[2], on), mixed)
        assert same(ref.frame(0, fl[1], fl[2], fsf[1], fsf[2], j.fw[2], j.bw[1]), fl[1])
        assert same(ref.frame(256, fl[1], fl[2], fsf[1], fsf[2], j.fw[2], j.bw[1]), fl[2])
        # past the clip's end the package hands the last frame as both clip frames: 24 -> 60 has no such frame over five inputs, 24 -> 120 would
        assert same(ref.frame(128, fl[4], fl[4], None, None, None, None), fl[4] if not blend else [(fl[4][p] * F(128) + fl[4][p] * F(128)) * F(1 / 256) for p in range(3)])
