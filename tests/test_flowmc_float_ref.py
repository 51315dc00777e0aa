"""CPU: the float restatement of Flow / FlowBlur (tests/flowmc_float_ref.py) anchored to the integer one (tests/flowmc_ref.py) and to the Super
restatement (tests/super_float_ref.py), on every geometry of the GPU cases (tests/flowmc_float_cases.py) with the oracle's search.

Integer-valued float clips are 8-bit samples stored as float32.  At pel 1 their float super frame is the padded plane, integer-valued too, so the
float filters must give the integer filters' samples: exactly for Flow, which only moves samples, and after floor() for FlowBlur (below).  The
samples are kept inside 2 .. 254 so that neither filter's hole value -- 255, 1.0f, 0.5f -- is a sample.  At pel 2 and 4 the float super frame is
not integer-valued (no rounding), so Flow is held to the positions instead: the integer restatement run on a Finest frame of position labels
names, per output sample, where it read, and the float output must be super_float_ref's sample there, found through the sub-pel plane, row and
column of that position and not through the restatement's own interleaved plane."""
import numpy as np
import pytest

import degrain_float_cases as fc
import flowmc_float_cases as fx
import flowmc_float_ref as ff
import flowmc_ref
import super_float_ref as sf

F = np.float32


def _geometries(cases):
    """one case per (format, size, padding, blocks) of the list"""
    seen, out = set(), []
    for c in cases:
        key = (c.fmt, c.w, c.h, c.skw.get("hpad"), c.akw["blksize"], c.akw["overlap"])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


class World:
    """one case at 8 bits and pel `pel`: the integer clip inside 2 .. 254, its integer-valued float clip, the oracle's super and Finest frames,
    the float super frames of the Super restatement, the (edited) vectors"""

    def __init__(self, oracle, mv, c, pel):
        self.c = c = c._replace(bits=8, skw=dict(c.skw, pel=pel))
        q, _ = fx.clips(c)
        self.q = [[np.clip(p, 2, 254) for p in fr] for fr in q]
        self.floats = fc.integer_valued(self.q)
        self.vectors = fx.edited(c, fx.search_oracle(oracle, c, self.q))
        self.info = mv.Super(c.w, c.h, 32, sample_float=True, **fx.super_kwargs(c)).info
        self.osup = oracle.Super(c.w, c.h, 8, **fx.super_kwargs(c))
        self.gray = c.fmt == "gray"
        self.nplanes = 1 if self.gray else 3
        self._fin, self._sup = {}, {}

    def fin(self, k):
        if k not in self._fin:
            self._fin[k] = self.osup.finest(self.osup.frame(self.q[k]))
        return self._fin[k]

    def sup(self, k):
        if k not in self._sup:
            i = self.info
            self._sup[k] = sf.frame(self.floats[k], sub=fx.SUB[self.c.fmt], gray=self.gray, hpad=i.hpad, vpad=i.vpad, pel=i.pel, sharp=i.sharp)[0]
        return self._sup[k]


@pytest.mark.parametrize("mode", [0, 1], ids=["fetch", "shift"])
@pytest.mark.parametrize("c", fx.FLOW_CASES, ids=fx.case_id)
def test_flow_at_pel_1_is_the_integer_flow(oracle, mv, c, mode):
    w = World(oracle, mv, c, 1)
    fkw = dict(w.c.fkw, mode=mode)
    ad, blobs = w.vectors[0]
    i = w.info
    old = flowmc_ref.Flow(ad, fx.NF, w.nplanes, i.hpad, i.vpad, 8, **fkw)
    new = ff.Flow(ad, fx.NF, w.nplanes, i.hpad, i.vpad, **fkw)
    kinds = set()
    for n in range(fx.NF):
        want = old.frame(n, w.q, w.fin, blobs[n])
        got = new.frame(n, w.floats, w.sup, blobs[n])
        assert new.last_kind == old.last_kind
        kinds.add(old.last_kind)
        for p in range(w.nplanes):
            hole = want[p] == 255
            assert got[p].dtype == F and np.array_equal(got[p], np.where(hole, ff.HOLE[p], want[p].astype(F))), (n, p)
            if p == 0 and old.last_kind == "shift":
                assert np.array_equal(got[p] == F(1.0), hole)       # on luma the holes are 1.0 where the integer output has 255
            assert old.last_kind == "shift" or not hole.any()
    assert kinds == {"copy", "shift" if mode else "fetch"}


@pytest.mark.parametrize("mode", [0, 1], ids=["fetch", "shift"])
@pytest.mark.parametrize("pel", [2, 4])
@pytest.mark.parametrize("c", _geometries(fx.FLOW_CASES), ids=fx.case_id)
def test_flow_at_pel_2_and_4_gathers_at_the_integer_restatements_positions(oracle, mv, c, pel, mode):
    w = World(oracle, mv, c, pel)
    fkw = dict(w.c.fkw, mode=mode)
    ad, blobs = w.vectors[0]
    i = w.info
    old = flowmc_ref.Flow(ad, fx.NF, w.nplanes, i.hpad, i.vpad, ff.POSITION_BITS, **fkw)
    new = ff.Flow(ad, fx.NF, w.nplanes, i.hpad, i.vpad, **fkw)
    planes, _ = sf.geometry(c.w, c.h, fx.SUB[c.fmt], w.gray, i.hpad, i.vpad, pel)
    lp = {2: 1, 4: 2}[pel]

    def labels(k):  # a Finest frame whose samples are their own flat positions
        return [np.arange((ph + 2 * vp) * pel * (pw + 2 * hp) * pel, dtype=np.int64).reshape((ph + 2 * vp) * pel, (pw + 2 * hp) * pel)
                for pw, ph, hp, vp in planes]
    dummy = [[np.zeros(p.shape, np.int64) for p in fr] for fr in w.q]
    moved = 0
    for n in range(fx.NF):
        pos = old.frame(n, dummy, labels, blobs[n])
        got = new.frame(n, w.floats, w.sup, blobs[n])
        if old.last_kind == "copy":
            assert all(np.array_equal(ff.bits(a), ff.bits(b)) for a, b in zip(got, w.floats[n]))
            continue
        s = w.sup(old.ref(n))
        for p, (pw, ph, hp, vp) in enumerate(planes):
            rows, cols = ph + 2 * vp, (pw + 2 * hp) * pel
            hole = pos[p] == (1 << ff.POSITION_BITS) - 1
            Y, X = np.where(hole, 0, pos[p]) // cols, np.where(hole, 0, pos[p]) % cols
            k = (X & (pel - 1)) | ((Y & (pel - 1)) << lp)
            want = np.where(hole, ff.HOLE[p], s[p][k * rows + (Y >> lp), X >> lp])
            assert hole.any() <= bool(mode) and np.array_equal(got[p], want), (n, p)
        moved += not np.array_equal(got[0], w.floats[n][0])
    assert moved or w.c.fkw["time"] == 0.0


@pytest.mark.parametrize("c", fx.BLUR_CASES, ids=fx.case_id)
def test_flowblur_at_pel_1_floors_to_the_integer_flowblur(oracle, mv, c):
    """floor(float out) == integer out, exactly.  The samples are integers below 2^8 and a sample has fewer than 2^16 taps, so every partial
    sum is an integer below 2^24 and each float32 addition is exact: sum is the integer filter's sum S, and the divisor N = mF + mB + 1 is exact
    too.  The division is correctly rounded: out = fl(S / N).  The integer filter writes floor(S / N) =: z (S >= 0).  z is an integer below
    2^24, hence a float32, and rounding is monotonic, so out >= z.  If N divides S, out = z.  Otherwise S / N <= z + 1 - 1 / N, while the
    rounding error is at most half an ulp, |out - S / N| <= 2^-24 * S / N = 2^-24 * S * (1 / N) < 1 / N because S < 2^24: out < z + 1.
    The premises are asserted on each case: the largest divisor below 2^16, the largest sum below 2^24."""
    w = World(oracle, mv, c, 1)
    (abw, bbw), (afw, bfw) = w.vectors
    i = w.info
    old = flowmc_ref.FlowBlur(abw, afw, fx.NF, w.nplanes, i.hpad, i.vpad, 8, **w.c.fkw)
    new = ff.FlowBlur(abw, afw, fx.NF, w.nplanes, i.hpad, i.vpad, **w.c.fkw)
    probe, stats, kinds, fractions = {}, {}, set(), 0
    for n in range(fx.NF):
        want = old.frame(n, w.q, w.fin, bbw, bfw, probe=probe)
        got = new.frame(n, w.floats, w.sup, bbw, bfw, stats)
        assert new.last_kind == old.last_kind
        kinds.add(old.last_kind)
        for p in range(w.nplanes):
            assert got[p].dtype == F and np.array_equal(np.floor(got[p]).astype(want[p].dtype), want[p]), (n, p)
            fractions += int(np.count_nonzero(got[p] != np.floor(got[p])))
    assert kinds == {"copy", "blur"}
    assert probe["max_count"] < 1 << 16 and probe["max_sum"] < 1 << 24
    assert probe["max_count"] >= stats["max_taps"] + 1  # (the probe looks at every plane, the counters at luma: both count the same taps)
    if w.c.fkw["blur"] > 0:
        assert fractions > 0 and probe["max_count"] >= 2  # (there were taps, and float outputs that are no integers: the floor was needed)


def test_blur_sum_adds_in_order_and_divides_once():
    """a sample of 2^24 with the taps 1, 1 and -2^24: added one by one in float32 each 1 is lost (2^24 + 1 rounds back to 2^24) and the mean
    is 0, where an exact, a pairwise or a sorted sum gives 2 and the mean 0.5.  No taps: the sample's bits, a NaN payload, a negative zero
    and a signalling NaN included"""
    fin = np.array([[2.0 ** 24, 1.0, 1.0, -2.0 ** 24]], F)
    reads = [(np.array([[1]]), np.array([[1]]))] + [(np.array([[1]]), np.array([[k + 1]])) for k in (1, 2, 3)]
    out, count = ff.blur_sum(fin, reads, (1, 1))
    assert count[0, 0] == 3 and out.dtype == F and out[0, 0] == F(0.0)
    assert F(np.sum(fin.astype(np.float64)) / 4.0) == F(0.5)
    odd = np.array([[0x7FC01234, 0x80000000, 0x7F800001]], np.uint32).view(F)
    reads = [(np.array([[1, 1, 1]]), np.array([[1, 2, 3]])), (np.zeros((1, 3), np.int64), np.zeros((1, 3), np.int64))]
    out, count = ff.blur_sum(odd, reads, (1, 1))
    assert not count.any() and np.array_equal(ff.bits(out), ff.bits(odd))


def test_finest_interleaves_the_sub_pel_planes():
    """Finest[y * pel + sy][x * pel + sx] = sub-pel plane (sx | sy << log2 pel)[y][x], the padding included"""
    rng = np.random.default_rng(3)
    for pel in (1, 2, 4):
        w, h, hp, vp = 12, 10, 4, 2
        rows, cols = h + 2 * vp, w + 2 * hp
        s = rng.random((pel * pel * rows, cols)).astype(F)
        fin = ff.finest([s], w, h, gray=True, hpad=hp, vpad=vp, pel=pel)[0]
        assert fin.shape == (rows * pel, cols * pel)
        lp = {1: 0, 2: 1, 4: 2}[pel]
        for Y in range(0, rows * pel, 3):
            for X in range(0, cols * pel, 5):
                k = (X & (pel - 1)) | ((Y & (pel - 1)) << lp)
                assert fin[Y, X] == s[k * rows + (Y >> lp), X >> lp]
