"""CPU: the cases of tests/test_gpu_flowmc_float.py test what they claim (tests/flowmc_float_cases.py states the conditions).  Each case is run
through the restatement (tests/flowmc_float_ref.py) on the oracle's search of the integer clip -- the float clip's quantised copy, which
degrain_float_cases.float_clip asserts -- and held to its conditions: a FlowBlur case that took no taps, a shift case without a hole or without
a contested destination, or a batch without a copied frame beside the compensated ones could not tell a wrong kernel from a right one."""
import numpy as np
import pytest

import flowmc_float_cases as fx
import flowmc_float_ref as ff

_expected = {}


def expected(oracle, mv, c):
    if fx.case_id(c) not in _expected:
        q, floats = fx.clips(c)
        info = mv.Super(c.w, c.h, 32, sample_float=True, **fx.super_kwargs(c)).info
        _expected[fx.case_id(c)] = (fx.Expected(c, floats, fx.edited(c, fx.search_oracle(oracle, c, q)), info), floats)
    return _expected[fx.case_id(c)]


@pytest.mark.parametrize("c", fx.CASES, ids=fx.case_id)
def test_a_case_meets_its_conditions(oracle, mv, c):
    e, floats = expected(oracle, mv, c)
    print("%s: %s %s" % (fx.case_id(c), e.kinds, e.stats))
    fx.check_conditions(c, e)
    same = [all(np.array_equal(ff.bits(a), ff.bits(b)) for a, b in zip(frame, floats[n])) for n, frame in enumerate(e.frames)]
    assert all(s for s, kind in zip(same, e.kinds) if kind == "copy")
    if c.fkw.get("time") != 0.0 and c.fkw.get("blur") != 0.0:  # (compensated frames are not copies of the clip frame)
        assert sum(not s for s in same) >= len(same) - e.kinds.count("copy") - 1, same


def test_the_searched_shift_cases_have_holes_and_contested_destinations_between_them(oracle, mv):
    hole = collide = 0
    for c in fx.FLOW_SEARCHED:
        if c.fkw.get("mode"):
            s = expected(oracle, mv, c)[0].stats
            hole, collide = hole + s.get("hole", 0), collide + s.get("collide", 0)
    assert hole >= 1 and collide >= 1, (hole, collide)


def test_the_cases_cover_what_they_should():
    both = lambda cases, key: {key(c) for c in cases}
    for cases in (fx.FLOW_CASES, fx.BLUR_CASES):
        assert both(cases, lambda c: c.fmt) >= {"420", "444", "gray"}
        assert both(cases, lambda c: c.bits) == {8, 16}
        assert both(cases, lambda c: c.skw["pel"]) == {1, 2, 4}
        assert both(cases, lambda c: (c.w, c.h)) == {(96, 64), (70, 54), (36, 36), (35, 30)}
        assert both(cases, lambda c: c.recipes[-1].name if c.recipes else None) >= {None, "limits", "invalid", "scene_count"}
    blocks = {(c.akw["blksize"], c.akw["overlap"]) for c in fx.CASES}
    assert blocks == {(16, 8), (8, 4), (4, 2), (16, 0)}
    assert {c.fkw["time"] for c in fx.FLOW_CASES} == {100.0, 50.0, 0.0}
    assert {(c.akw["isb"], c.akw.get("delta", 1)) for c in fx.FLOW_CASES} >= {(1, 1), (0, 1), (1, 2), (0, 2)}
    assert sum(c.akw.get("delta", 1) <= 0 for c in fx.FLOW_CASES) == 1
    assert {c.fkw["blur"] for c in fx.BLUR_CASES} == {50.0, 200.0, 0.0} and {c.fkw.get("prec", 1) for c in fx.BLUR_CASES} == {1, 4}
    # segments of 4, 2 and 1 float samples: the widest that divides the plane width
    seg = lambda w: 4 if w % 4 == 0 else 2 if w % 2 == 0 else 1
    assert [seg(96), seg(48), seg(70), seg(35), seg(36)] == [4, 4, 2, 1, 4]
