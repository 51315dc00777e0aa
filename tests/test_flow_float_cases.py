"""CPU: the cases of tests/test_gpu_flow_float.py test what they claim (tests/flow_float_cases.py states the conditions).  Each case is run
through the restatement (tests/flow_float_ref.py) on the oracle's search of the integer clip and held to its conditions: a batch without a
fallback beside the interpolated jobs, an occlusion field that masks almost nothing, masked samples whose two fetches are equal, or an Extra
job whose clamp never binds could not tell a wrong kernel from a right one."""
import numpy as np
import pytest

import flow_float_cases as fx
import flow_float_ref as fl

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
    print("%s: %s %s %s" % (fx.case_id(c), e.kinds, e.times, e.stats))
    fx.check_conditions(c, e)
    assert len(e.frames) == (fx.NF if c.kind == "inter" else {60: 11, 48: 9}[c.fkw["num"]])
    last = fx.NF - 1
    for n, (frame, kind) in enumerate(zip(e.frames, e.kinds)):
        nl, nr, t = e.ref.map(n)
        assert all(p.dtype == np.float32 for p in frame)
        if kind in ("copy", "left"):   # bit for bit the clip frame
            src = floats[min(nr, last)] if kind == "copy" and t == 256 else floats[min(nl, last)]
            assert all(np.array_equal(fl.bits(a), fl.bits(b)) for a, b in zip(frame, src)), (n, kind)
        assert (kind == "copy") == (c.kind == "fps" and t in (0, 256))


def test_the_cases_cover_what_they_should(oracle, mv):
    kinds = {k: set() for k in ("inter", "fps")}
    left = fallthrough = False
    for c in fx.CASES:
        e, _ = expected(oracle, mv, c)
        kinds[c.kind] |= set(e.kinds)
        left = left or (c.fkw.get("blend") == 0 and "left" in e.kinds)
        fallthrough = fallthrough or (c.kind == "fps" and c.fkw["mask"] == 2 and any(k.startswith("simple") for k in e.kinds))
    strip = lambda ks: {k.replace("128", "") for k in ks}
    assert strip(kinds["inter"]) >= {"regular", "extra", "blend", "left"} and "simple" not in strip(kinds["inter"])  # (FlowInter has no Simple path)
    assert strip(kinds["fps"]) >= {"simple", "regular", "extra", "copy", "blend", "left"}
    assert {"regular128", "extra128"} <= kinds["inter"] and {"simple128", "regular128", "extra128"} <= kinds["fps"]
    assert left and fallthrough
    both = lambda cases, key: {key(c) for c in cases}
    for cases in (fx.INTER_CASES, fx.FPS_CASES):
        assert both(cases, lambda c: c.fmt) >= {"420", "444", "gray"}
        assert both(cases, lambda c: c.bits) == {8, 16}
        assert both(cases, lambda c: c.skw["pel"]) == {1, 2, 4}
        assert both(cases, lambda c: (c.w, c.h)) == {(96, 64), (70, 54), (36, 36), (35, 30)}
        assert both(cases, lambda c: c.recipes[-1].name if c.recipes else None) >= {None, "limits", "occlusion", "invalid", "scene_count"}
        assert both(cases, lambda c: c.akw.get("delta", 1)) == {1, 2}
        assert both(cases, lambda c: c.fkw.get("blend", 1)) == {0, 1}
    assert {c.fkw["time"] for c in fx.INTER_CASES} == {0.0, 37.5, 50.0, 100.0}
    assert {(c.fkw["num"], c.fkw["mask"]) for c in fx.FPS_CASES} >= {(n, m) for n in (48, 60) for m in (0, 1, 2)}
    # segments of 4, 2 and 1 float samples: the widest that divides the plane width
    seg = lambda w: 4 if w % 4 == 0 else 2 if w % 2 == 0 else 1
    assert [seg(96), seg(48), seg(70), seg(35), seg(36)] == [4, 4, 2, 1, 4]
