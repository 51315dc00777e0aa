"""CPU: the DegrainN and CompensateN cases of tests/test_vs_multi_shell.py test what they claim, shown through the oracle alone.

DegrainN beyond radius 6: on the middle frame at least half of the (block, reference) pairs beyond distance 6 carry a weight and at least a fiftieth carry
none (degrain_n_cases.far_shares_ok, the condition of tests/test_degrain_n_cases.py).  Up to radius 6 the references change the frame.
CompensateN: beyond distance 1 at least half of the (block, field) pairs are compensated and at least a fiftieth fall back on the source
(multi_cases.far_shares, the condition of tests/test_multi_cases.py); the scene-change cases have fields of both kinds; the map from an output to its field
puts the outputs in temporal order."""
import numpy as np
import pytest

import degrain_n_cases as dc
import multi_cases as mc
import pipeline as pl
import vs_multi_cases as vc


@pytest.mark.parametrize("case", vc.DEGRAIN_CASES, ids=vc.degrain_id)
def test_degrain_cases_use_their_references(oracle, case):
    m, radius, dkw, ad, blobs = vc.degrain_inputs(case)
    n = m.n // 2
    if case[7] == "oracle":
        out = vc.degrain_expected(oracle, case, frames=(n,))[n]
        assert np.count_nonzero(out[0] != m.frames[n][0]) > out[0].size // 4
        return
    ref = vc.degrain_ref(oracle, case)
    ref.weigh([m.ref(n, r) for r in range(2 * radius)], blobs[n][:2 * radius])
    if radius > 6:
        ok, what = dc.far_shares_ok(ref)
        assert ok, what
    else:
        assert np.count_nonzero(ref.plan[0][1]) > ref.plan[0][1].size // 2


@pytest.mark.parametrize("case", [c for c in vc.COMPENSATE_CASES if not c[6] and not c[7]], ids=vc.compensate_id)
def test_compensate_cases_compensate_most_far_blocks_and_not_all(oracle, case):
    m, tr = vc.compensate_multi(case), vc.compensate_tr(case)
    n = m.radius + 1
    sads = [pl.blob_vectors(m.blobs[n][r], m.ads[r])[2] for r in range(2 * tr)]
    used, unused = mc.far_shares(sads, m.ads[0], case[5]["thsad"], tr)
    assert used >= mc.USED and unused >= mc.UNUSED, "beyond distance 1: %.3f of the pairs below thsad, %.3f not" % (used, unused)


@pytest.mark.parametrize("case", [c for c in vc.COMPENSATE_CASES if "thscd1" in c[5]], ids=vc.compensate_id)
def test_scene_change_cases_have_fields_of_both_kinds(oracle, case):
    m, tr = vc.compensate_multi(case), vc.compensate_tr(case)
    sc = vc.scene_changes(m, range(2 * tr), case[5]["thscd1"], case[5]["thscd2"])
    cut = sum(sc.values())
    assert cut >= 4 and len(sc) - cut >= 4, "%d of %d valid (frame, field) pairs are scene changes" % (cut, len(sc))
    # ... and at a scene change the output is the reference frame (scbehavior 0) or the source (1), which differ
    want = vc.compensate_expected(oracle, case)
    no = 2 * tr + 1
    seen = 0
    for (n, f), is_cut in sc.items():
        if not is_cut:
            continue
        k = [k for k in range(no) if vc.compensate_map(tr, k)[1] == f][0]
        other = m.frames[n] if case[5]["scbehavior"] else m.frames[m.nref(n, f)]
        assert all(np.array_equal(a, b) for a, b in zip(want[n * no + k], other))
        seen += 1
    assert seen == cut


@pytest.mark.parametrize("tr", [1, 2, 7])
def test_the_map_is_in_temporal_order(tr):
    seen = []
    for k in range(2 * tr + 1):
        off, field = vc.compensate_map(tr, k)
        assert off == k - tr
        if field >= 0:
            isb, d = mc.field_of(field)
            assert d == abs(off) and bool(isb) == (off > 0)
            seen.append(field)
    assert sorted(seen) == list(range(2 * tr))
