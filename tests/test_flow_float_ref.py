"""CPU: the float restatement of FlowInter / FlowFPS (tests/flow_float_ref.py) anchored to the integer one (tests/flow_ref.py), on every case
of the GPU tests (tests/flow_float_cases.py) brought to 8 bits and pel 1 with the oracle's search.

Integer-valued float clips are 8-bit samples stored as float32.  At pel 1 their float super frame is the padded plane, integer-valued too, so
both restatements fetch the same numbers d <= peak = 255 and differ only in the arithmetic after the fetch.

Where mF = mB = 0 the float result, floored, IS the integer one.  mix(0, p, q) = (0 * p + 255 * q) / 255 = q exactly (255 * q < 2^16), and
time() forms r * t + l * (256 - t) < 2^16 exactly and multiplies by the exact 1 / 256: the float value is the rational (r * t + l * (256 - t)) /
256, whose floor is the integer filter's >> 8.  The integer stages are exact there as well: (255 * d + 255) >> 8 = d for d <= 255, and Simple's
formula at 128 is ((dF + dB) << 8) >> 9.

Elsewhere the difference is bounded by the reference's own rounding.  With v = S / 255 the exact mix, a stage (S + 255) >> 8 =
floor(v - v / 256 + 255 / 256) lies in (v - v / 256 - 1 / 256, v - v / 256 + 255 / 256], i.e. within (-(peak + 1) / 256, 255 / 256] of v; the
time stage averages two such errors with weights (256 - t) / 256 and t / 256 and its >> 8 adds (-1, 0]:
    Simple, Extra    integer - exact in (-(peak + 1) / 256 - 1, 255 / 256]
    Regular          the inner stage (mF * I + 255) >> 8 with I = 255 * w stands for mF * w and lies in (-mF * w / 256 - 1 / 256, 255 / 256 -
                     mF * w / 256] of it, mF * w <= 255 * peak; the outer ">> 8" divides that by 256 once more and adds its own
                     (-a / 256 - 1 / 256, 255 / 256 - a / 256]:  integer - exact in (-(peak / 256 + 255 * peak / 65536 + 257 / 65536) - 1,
                     255 / 256 + 255 / 65536]
    Simple at 128    the reference's ((dF + dB) * 256 + (dB - dF) * (mF - mB)) >> 9 has / 512 where the general formula has / 510:
                     |dB - dF| * |mF - mB| * (1 / 510 - 1 / 512) <= peak / 512, and its >> 9 adds (-1, 0]:  within peak / 512 + 1
Float rounding comes on top: at most ten operations, each off by at most half an ulp of a value below 2^16 (2^-9), every one of them divided
by at least 255 afterwards: below 10 * 2^-9 / 255 < 2^-12 = SLACK."""
import numpy as np
import pytest

import degrain_float_cases as fc
import flow_float_cases as fx
import flow_float_ref as fl
import flow_ref
import super_float_ref as sf

F = np.float32
PEAK = 255
SLACK = 2.0 ** -12
STAGE = (-(PEAK + 1) / 256.0 - 1.0, 255.0 / 256.0)
BOUNDS = {"simple": STAGE, "extra": STAGE, "extra128": STAGE,
          "regular": (-(PEAK / 256.0 + 255.0 * PEAK / 65536.0 + 257.0 / 65536.0) - 1.0, 255.0 / 256.0 + 255.0 / 65536.0),
          "simple128": (-(PEAK / 512.0 + 1.0), PEAK / 512.0 + 1.0)}
BOUNDS["regular128"] = BOUNDS["regular"]


def test_the_bounds_are_the_derived_ones():
    r = lambda b: (round(b[0], 4), round(b[1], 4))
    assert r(BOUNDS["simple"]) == (-2.0, 0.9961) and r(BOUNDS["regular"]) == (-2.9922, 1.0) and r(BOUNDS["simple128"]) == (-1.498, 1.498)


class World:
    """one case at 8 bits and pel 1: the integer clip, its integer-valued float clip, the oracle's super and Finest frames, the float super
    frames of the Super restatement, the (edited) vectors"""

    def __init__(self, oracle, mv, c):
        self.c = c = c._replace(bits=8, skw=dict(c.skw, pel=1))
        self.q, _ = fx.clips(c)
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


_seen = {}


@pytest.mark.parametrize("c", fx.CASES, ids=fx.case_id)
def test_integer_valued_clips_floor_to_the_integer_filter_or_stay_within_the_bound(oracle, mv, c):
    w = World(oracle, mv, c)
    (abw, bbw), (afw, bfw) = w.vectors
    i = w.info
    old = flow_ref.Flow(abw, afw, fx.NF, w.nplanes, i.hpad, i.vpad, **w.c.fkw)
    new = fl.Flow(abw, afw, fx.NF, w.nplanes, i.hpad, i.vpad, **w.c.fkw)
    assert new.num_frames == old.num_frames
    worst = {}
    for n in range(old.num_frames):
        probe = {}
        want = old.frame(n, w.q, w.fin, bbw, bfw)
        got = new.frame(n, w.floats, w.sup, bbw, bfw, probe)
        kind = old.last_kind
        assert new.last_kind == kind and new.map(n) == old.map(n)
        _seen.setdefault(c.kind, set()).add(kind)
        for p in range(w.nplanes):
            assert got[p].dtype == F and got[p].shape == want[p].shape
            if kind in ("copy", "left"):
                assert np.array_equal(got[p], want[p].astype(F)), (n, p)
                continue
            if kind == "blend":   # (l * (256 - t) + r * t) / 256 exactly: the floor is Blend's >> 8
                assert np.array_equal(np.floor(got[p]).astype(want[p].dtype), want[p]), (n, p)
                continue
            MF, MB = probe["MF"][p], probe["MB"][p]
            clear = (MF == 0) & (MB == 0)
            assert np.array_equal(np.floor(got[p])[clear].astype(want[p].dtype), want[p][clear]), (n, p, kind)
            d = want[p].astype(np.float64) - got[p].astype(np.float64)
            lo, hi = BOUNDS[kind]
            assert d.min() > lo - SLACK and d.max() <= hi + SLACK, (n, p, kind, float(d.min()), float(d.max()))
            wk = worst.setdefault(kind, [0.0, 0.0, 0, 0])
            wk[0], wk[1], wk[2], wk[3] = min(wk[0], float(d.min())), max(wk[1], float(d.max())), wk[2] + int(clear.sum()), wk[3] + int((~clear).sum())
    print("%s: integer - float per kind (min, max, clear samples, masked samples): %s" % (fx.case_id(c), worst))


def test_every_formula_was_anchored():
    """(runs after the cases above) FlowInter has no Simple path"""
    if len(_seen.get("inter", ())) and len(_seen.get("fps", ())):
        strip = lambda ks: {k.replace("128", "") for k in ks}
        assert strip(_seen["inter"]) >= {"regular", "extra", "blend", "left"}
        assert strip(_seen["fps"]) >= {"simple", "regular", "extra", "copy", "blend", "left"} and "simple128" in _seen["fps"]


def test_copies_and_the_left_frame_keep_their_bits(oracle, mv):
    """clip frames of quiet NaNs with payloads, a negative zero, infinities and a denormal: FlowFPS at time256 0, and a blend 0 fallback, return
    the bits"""
    odd = np.array([0x7FC00000, 0x7FC01234, 0xFFC00001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x7F7FFFFF], np.uint32)
    for cases, name in ((fx.FPS_CRAFTED, "70x54-scene-60-mask1-blend0"), (fx.INTER_CRAFTED, "70x54-scene-blend0")):
        c = [x for x in cases if x.name == name][0]
        q, floats = fx.clips(c)
        weird = [[odd[(np.arange(p.size) + n) % odd.size].reshape(p.shape).view(F) for p in fr] for n, fr in enumerate(floats)]
        info = mv.Super(c.w, c.h, 32, sample_float=True, **fx.super_kwargs(c)).info
        e = fx.Expected(c, weird, fx.edited(c, fx.search_oracle(oracle, c, q)), info, supers=lambda k: sf.frame(floats[k], sub=fx.SUB[c.fmt], gray=False,
                        hpad=info.hpad, vpad=info.vpad, pel=info.pel, sharp=info.sharp)[0])
        hit = 0
        for n, kind in enumerate(e.kinds):
            if kind in ("copy", "left"):
                nl = e.ref.map(n)[0]
                assert all(np.array_equal(fl.bits(a), fl.bits(b)) for a, b in zip(e.frames[n], weird[min(nl, fx.NF - 1)])), (name, n)
                hit += 1
        assert hit >= 2


def test_simple_has_one_formula_at_128():
    """at time256 128 the float Simple is the general formula, not the reference's special one: they differ where the masks differ"""
    dF, dB = np.array([10.0, 200.0], F), np.array([250.0, 20.0], F)
    mF, mB = np.array([255, 0]), np.array([0, 255])
    got = fl.simple(128, dF, dB, mF, mB)
    assert np.array_equal(got, np.array([250.0, 200.0], F))                       # (dF + dB) / 2 + (dB - dF) * (mF - mB) / 510
    special = ((dF.astype(np.int64) + dB.astype(np.int64)) * 256 + (dB - dF).astype(np.int64) * (mF - mB)) >> 9
    assert list(special) == [249, 199]                                            # ... / 512 in the reference
