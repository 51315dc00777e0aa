"""CPU: the RecalculateN cases of tests/test_gpu_multi_recalculate.py and tests/test_vs_multi_shell.py test what they claim.  Through the oracle
alone, over every valid (frame, field) of each case: at least a fiftieth of the blocks are searched again at the cases' thsad, and at least a
fiftieth keep the vector interpolated from the old field.  A RecalculateN that never searched, or one that always did, could not pass them."""
import pytest

import multi_oracle as mu


@pytest.mark.parametrize("case", mu.recalc_cases(), ids=mu.recalc_id)
def test_some_blocks_are_searched_again_and_some_are_not(oracle, case):
    again, kept = mu.recalc_multi(case).recalc_shares(**mu.recalc_kwargs(case))
    assert again >= mu.SHARE and kept >= mu.SHARE, "%.3f of the blocks searched again, %.3f kept" % (again, kept)


def test_the_cases_cover_what_they_should():
    cases = mu.recalc_cases()
    plain = {(fmt, bits, geo[0], radius) for fmt, bits, geo, radius, extra in cases if not extra}
    assert plain == {(fmt, bits, geo[0], radius) for fmt, bits in (("420", 8), ("420", 16), ("444", 8)) for geo in mu.RECALC_GEOS for radius in (1, 2, 3, 7)}
    assert any(extra.get("divide") == 1 for *_, extra in cases) and any(extra.get("smooth") == 0 for *_, extra in cases)
