"""GPU parity of mv.DepanStabilise on float clips (depan_warp_kernel<float, SUB, DS_SOURCES> of mvx_depan_warp.hip) against the sequential paint
of the CPU restatement tests/depan_float_ref.py, through the Python package: every sample of every plane as uint32, all jobs of a case in ONE
mvx_depan_stabilise_frames call, guard rows and row tails untouched.  The crafted cases are depan_stab_cases' -- prev only, next only, both
and neither, mixed in one batch, each subpixel, the mirror bits, blur, 4:2:2 / 4:4:4 / Gray, NaN and out-of-range transforms -- on float32
noise in [-0.25, 1.25); whole clips take their plans from the library's host arithmetic (method 0 and 1).  A current frame that is negative
everywhere is never overpainted where it covers the sample: the float path carries a painted flag where the integer path reads `v < 0`."""
import numpy as np
import pytest

import depan_cases as dc
import depan_float_cases as fc
import depan_float_ref as fr
import depan_stab_cases as sc
import depan_stab_ref as sr

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = fc.once(sc.CASES)


def _run(mv, case, frames=None):
    import torch
    src, want, who, stats = fc.stab_expected(case, "noise", frames)
    f = dc.FORMATS[case["fmt"]]
    dev = [[mv.plane_to_device(p) for p in fr_] for fr_ in src]
    g = mv.DepanStabilise(case["w"], case["h"], 32, f["subsampling"], f.get("gray", False), src_pitch=[d.stride(0) for d in dev[0]], subpixel=case["sub"],
                          mirror=case["mirror"], blur=case["blur"], prev=1, next=1, num_frames=3, sample_float=True)
    assert g.dtype == np.float32 and g.info.bits == 32 and list(g.info.border) == [0, 0, 0]
    plans = [fc.stab_plan(mv, *j) for j in case["jobs"]]
    n = len(plans)
    full, out = dc.guarded(g, n)
    arr, _ = g.jobs(plans, [dev[0]] * n, [dev[j[2][0]] if j[2] else None for j in case["jobs"]], [dev[j[1][0]] if j[1] else None for j in case["jobs"]], out=out)
    g.launch(arr)
    torch.cuda.synchronize()
    fc.check(full, want)
    return want, who, stats


@pytest.mark.parametrize("case", CASES, ids=sc.ids(CASES))
def test_crafted_plans(mv, case):
    _, _, stats = _run(mv, case)
    assert not sc.missing(case, stats), stats


@pytest.mark.parametrize("name", ["combos_s0_8", "combos_s1_8", "combos_s2_8", "mirror15_s2"])
def test_a_negative_current_frame_is_never_overpainted(mv, name):
    """the current frame in [-3, -2), the fill sources in [1, 2): a sample is negative exactly where the restatement took it from the current
    frame (tests/test_depan_float_ref.py holds that set to the integer restatement's coverage), and the batch mixes jobs with both fill
    sources, one and none"""
    case = next(c for c in sc.CASES if c["name"] == name)
    rng = np.random.default_rng(7)
    frames = [[(rng.random(s, dtype=f32) + f32(o)).astype(f32) for s in dc.planes_shape(case)] for o in (-3, 1, 1)]
    want, who, stats = _run(mv, case, frames)
    assert stats["from_cur"] and stats["from_next"] and stats["from_prev"]
    for k, (cur, nxt, prev) in enumerate(case["jobs"]):
        if nxt is None and prev is None:
            continue                                                     # the current frame is the first pass: its border value is not negative
        for p in range(len(want[k])):
            assert np.array_equal(want[k][p] < 0, who[k][p] == fr.CUR), (k, p)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("sub", [0, 2])
def test_a_whole_clip(mv, method, sub):
    """12 frames of 70 x 38 through run(frames, motions) with prev = next = 2 and one bad frame: the plans are the library's host arithmetic
    (held to the restatement's by tests/test_depan_stab_host.py), painted frame by frame by the float restatement"""
    import torch
    w, h, n = 70, 38, 12
    rng = np.random.default_rng(21)
    frames = [[(rng.random(s, dtype=f32) * f32(1.5) - f32(0.25)).astype(f32) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))] for _ in range(n)]
    motions = sc.track(n, 22, bad=(5,))
    dev = [mv.frame_to_device(f) for f in frames]
    kw = dict(method=method, cutoff=0.5, mirror=15, blur=2, subpixel=sub)
    g = mv.DepanStabilise(w, h, 32, src_pitch=[t.stride(0) for t in dev[0]], num_frames=n, prev=2, next=2, sample_float=True, **kw)
    e = sr.Stabilise(w, h, n, prev=2, next=2, **kw)
    stats, want = {}, []
    for k in range(n):
        p = e.plan(k, motions)
        assert sr.plan_words(p) == list(np.frombuffer(bytes(g.plan(k, motions[g.window(k)[0]:g.window(k)[1] + 1])), np.uint32))
        want.append(fr.paint(frames[k], p["tr"], (frames[p["prev"]["frame"]], p["prev"]["tr"]), (frames[p["next"]["frame"]], p["next"]["tr"]), sub, mirror=15, blur=2, stats=stats))
    assert stats["from_cur"] and stats["from_next"] and stats["from_prev"] and stats["passes"] == 9 * n
    full, out = dc.guarded(g, n)
    g.run(dev, motions, out=out)
    torch.cuda.synchronize()
    fc.check(full, want)


def test_no_frames_is_a_no_op(mv):
    import torch
    g = mv.DepanStabilise(206, 118, 32, num_frames=4, prev=1, next=1, sample_float=True)
    full, out = dc.guarded(g, 1)
    g.launch((mv.DepanStabiliseJob * 0)())
    assert g.run([], []) == []
    torch.cuda.synchronize()
    assert all(bool((t == 0xA5).all()) for t in full[0])
