"""CPU: tests/super_float_ref.py (the yardstick of the float Super) anchored to the oracle's Super, which the reference pins.

On a float clip whose samples are the integers of an 8-bit or of a 16-bit clip every intermediate of the float rule is an integer below 2^24
(sharp 1: at most 18 * 65535; sharp 2: |m0| <= (2 + 5 * 8) * 65535 < 2^22), so float32 holds it exactly, a multiplication by a power of two
is exact, and the integer rule's (v + r) >> k is floor(v / 2^k + 0.5): clip(floor(x + 0.5), 0, peak) of the restatement's level-0 plane and of
its H and V planes must equal the oracle's planes sample for sample, and for sharp 0 the HV plane too.  The HV plane of sharp 1 and 2 and the
averages of pel 4 are not anchored: the integer path rounds in between."""
import numpy as np
import pytest

import pipeline as pl
import sample_range as sr
import super_float_ref as sf
import synth

W, H = 72, 40


def _clip(gen, bits):
    if gen == "texture":
        return synth.survey_clip(W, H, bits, 1)[0]
    return sr.make(gen, W, H, bits, 2)[1]


@pytest.mark.parametrize("sharp", [0, 1, 2])
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("gen", ["rails", "checker", "texture"])
def test_integer_valued_clips_round_to_the_oracles_planes(oracle, gen, bits, sharp):
    frame = _clip(gen, bits)
    peak = (1 << bits) - 1
    osup = oracle.Super(W, H, bits, pel=2, sharp=sharp)
    want = osup.frame(frame)
    got, defined = sf.frame([p.astype(np.float32) for p in frame], pel=2, sharp=sharp)
    checked = 0
    for p, lv, k, y0, x0, h, w in osup.defined_regions():
        if lv or (k == 3 and sharp):
            continue
        g = got[p][y0:y0 + h, x0:x0 + w]
        assert defined[p][y0:y0 + h, x0:x0 + w].all()
        r = np.clip(np.floor(g.astype(np.float64) + 0.5), 0, peak).astype(want[p].dtype)
        assert pl.first_diff(r, want[p][y0:y0 + h, x0:x0 + w]) == "", (p, k)
        checked += 1
    assert checked == 3 * (4 if sharp == 0 else 3)
    if sharp and gen != "texture":  # the clamp matters here: the float planes overshoot the range on these clips
        assert float(got[0].min()) < 0 or float(got[0].max()) > peak


def test_geometry_is_the_integer_creates_at_one_level(oracle):
    for sub, gray, hpad, vpad, pel in [((1, 1), False, 16, 16, 2), ((1, 1), False, 8, 4, 4), ((1, 0), False, 5, 3, 1), ((0, 0), False, 0, 0, 2), ((1, 1), True, 16, 16, 4),
                                       ((1, 1), False, 3, 5, 1)]:
        osup = oracle.Super(70, 54, 8, subsampling=sub, gray=gray, hpad=hpad, vpad=vpad, pel=pel, levels=1)
        _, shapes = sf.geometry(70, 54, sub, gray, hpad, vpad, pel)
        assert [tuple(osup.plane_shape(p)) for p in range(osup.nplanes)] == shapes


def test_pel_4_planes_are_averages_and_the_shifted_ones_end_in_zero():
    rng = np.random.default_rng(3)
    src = rng.random((9, 11)).astype(np.float32)
    p = sf.subpel_planes(src, 2, 1, 4, 1)
    assert sorted(p) == list(range(16))
    assert np.array_equal(p[1], (p[0] + p[2]) * np.float32(0.5))
    assert np.array_equal(p[3][:, :-1], (p[0][:, 1:] + p[2][:, :-1]) * np.float32(0.5)) and not p[3][:, -1].any()
    assert np.array_equal(p[12][:-1], (p[0][1:] + p[8][:-1]) * np.float32(0.5)) and not p[12][-1].any()
    assert np.array_equal(p[5], (p[4] + p[6]) * np.float32(0.5))
    assert np.array_equal(p[15][:, :-1], (p[12][:, 1:] + p[14][:, :-1]) * np.float32(0.5))


def test_a_flat_plane_stays_flat_and_chroma_may_be_negative():
    for c in (0.25, -0.5, 1.0, 0.1, 1.3):
        for sharp in (0, 1, 2):
            for k, a in sf.subpel_planes(np.full((12, 14), c, np.float32), 4, 4, 2, sharp).items():
                assert np.abs(a - np.float32(c)).max() <= 2 * np.spacing(np.float32(abs(c))), (c, sharp, k)
