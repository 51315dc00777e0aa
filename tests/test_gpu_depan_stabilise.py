"""GPU parity of mv.DepanStabilise (mvx_depan_warp.hip) against the sequential painting of the CPU restatement tests/depan_stab_ref.py, through the
Python package.  Bit-exact on every sample of every plane; all jobs of a case in ONE mvx_depan_stabilise_frames call.  Every destination plane
sits in a buffer with a guard row before and after it, filled with 0xA5: nothing but the samples may change.

The crafted cases (tests/depan_stab_cases.py) name the counters of the restatement they must reach -- samples from each of the three sources,
the mirror and blur branches of the first pass, undefined positions -- and tests/test_depan_stab_ref.py proves the same cases on the CPU with
the kernel's text compiled for the host.  Nothing here provokes a fault: NaN and out-of-range transforms are defined behaviour (the pass's
border value, mvtools_amd.h)."""
import numpy as np
import pytest

import depan_cases as dc
import depan_stab_cases as sc
import depan_stab_ref as sr

pytestmark = pytest.mark.gpu
f32 = np.float32


def _plan(mv, cur, nxt, prev):
    p = mv.DepanStabilisePlan()
    p.tr[:] = [float(v) for v in cur]
    for name, s in (("next", nxt), ("prev", prev)):
        if s is not None:
            d = getattr(p, name)
            d.used, d.frame = 1, s[0]
            d.tr[:] = [float(v) for v in s[1]]
    return p


def _run(mv, case):
    import torch
    src, want, stats = sc.expected(case)
    f = dc.FORMATS[case["fmt"]]
    dev = [[mv.plane_to_device(p) for p in fr] for fr in src]
    g = mv.DepanStabilise(case["w"], case["h"], case["bits"], f["subsampling"], f.get("gray", False), src_pitch=[d.stride(0) for d in dev[0]], subpixel=case["sub"],
                          mirror=case["mirror"], blur=case["blur"], prev=1, next=1, num_frames=3)
    plans = [_plan(mv, *j) for j in case["jobs"]]
    n = len(plans)
    full, out = dc.guarded(g, n)
    arr, _ = g.jobs(plans, [dev[0]] * n, [dev[j[2][0]] if j[2] else None for j in case["jobs"]], [dev[j[1][0]] if j[1] else None for j in case["jobs"]], out=out)
    g.launch(arr)
    torch.cuda.synchronize()
    dc.check(full, want, g.dtype)
    return stats


@pytest.mark.parametrize("case", sc.CASES, ids=sc.ids(sc.CASES))
def test_crafted_plans(mv, case):
    stats = _run(mv, case)
    assert not sc.missing(case, stats), stats


@pytest.mark.parametrize("case", sc.FULL_CASES, ids=sc.ids(sc.FULL_CASES))
def test_full_size(mv, case):
    """1920 x 1080 4:2:0 8-bit with both fill sources, the shape tools/depan_stabilise_bench.py measures; rotation forms walk 1920 columns"""
    stats = _run(mv, case)
    assert not sc.missing(case, stats), stats


def _clip(w, h, n, seed):
    rng = np.random.default_rng(seed)
    return [[rng.integers(0, 256, s).astype(np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))] for _ in range(n)]


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("size", [(70, 38), (206, 118)], ids=["70x38", "206x118"])
def test_a_whole_clip(mv, size, method):
    """12 frames through run(frames, motions) with prev = next = 2 and one bad frame, against the restatement's plans painted frame by frame;
    and prev = next = 0 equals DepanCompensate.run given the plans' transforms"""
    import torch
    w, h = size
    n = 12
    frames = _clip(w, h, n, 21)
    motions = sc.track(n, 22, bad=(5,))
    dev = [mv.frame_to_device(f) for f in frames]
    pitch = [t.stride(0) for t in dev[0]]
    kw = dict(method=method, cutoff=0.5, mirror=15, blur=2, subpixel=2)
    g = mv.DepanStabilise(w, h, src_pitch=pitch, num_frames=n, prev=2, next=2, **kw)
    e = sr.Stabilise(w, h, n, prev=2, next=2, **kw)
    stats, want = {}, []
    for k in range(n):
        p = e.plan(k, motions)
        want.append(e.paint(frames[k], p["tr"], (frames[p["prev"]["frame"]], p["prev"]["tr"]), (frames[p["next"]["frame"]], p["next"]["tr"]), stats))
    assert stats["from_cur"] and stats["from_next"] and stats["from_prev"] and stats["passes"] == 9 * n
    full, out = dc.guarded(g, n)
    as_dicts = [dict(dx=m[0], dy=m[1], zoom=m[2], rot=m[3]) for m in motions]      # what DepanAnalyse.run and DepanEstimate.run return
    g.run(dev, as_dicts, out=out)
    torch.cuda.synchronize()
    dc.check(full, want, np.uint8)

    g0 = mv.DepanStabilise(w, h, src_pitch=pitch, num_frames=n, **kw)
    plans = [g0.plan(k, motions[g0.window(k)[0]:g0.window(k)[1] + 1]) for k in range(n)]
    assert not any(p.prev.used or p.next.used for p in plans)
    a = g0.run(dev, motions)
    b = mv.DepanCompensate(w, h, src_pitch=pitch, offset=1.0, subpixel=2, mirror=15, blur=2).run(dev, [np.array(p.tr, dtype=f32) for p in plans])
    torch.cuda.synchronize()
    for k in range(n):
        for p in range(3):
            width = w >> (1 if p else 0)
            assert torch.equal(a[k][p][:, :width], b[k][p][:, :width]), (k, p)


def test_radius_zero_takes_the_border_value_and_the_fill_sources(mv):
    """method 1 with fps < 4 * cutoff: the transform of every frame is NaN (MVDepan.cpp:3155), so the current frame's pass paints nothing
    (DepanCompensate's divergence 5) and, without fill sources, every sample is the border value"""
    import torch
    w, h, n = 70, 38, 4
    frames = _clip(w, h, n, 23)
    motions = sc.track(n, 24)
    dev = [mv.frame_to_device(f) for f in frames]
    pitch = [t.stride(0) for t in dev[0]]
    for fill in (0, 1):
        g = mv.DepanStabilise(w, h, src_pitch=pitch, num_frames=n, method=1, cutoff=7.0, prev=fill, next=fill)
        e = sr.Stabilise(w, h, n, method=1, cutoff=7.0, prev=fill, next=fill)
        assert g.info.radius == 0
        want, stats = [], {}
        for k in range(n):
            p = e.plan(k, motions)
            assert np.isnan(p["tr"]).all()
            src = lambda s: None if s is None else (frames[s["frame"]], s["tr"])
            want.append(e.paint(frames[k], p["tr"], src(p["prev"]), src(p["next"]), stats))
        full, out = dc.guarded(g, n)
        g.run(dev, motions, out=out)
        torch.cuda.synchronize()
        dc.check(full, want, np.uint8)
        assert stats["undef"] > 0
        if not fill:
            assert all(np.all(fr[0] == 0) and np.all(fr[1] == 128) and np.all(fr[2] == 128) for fr in want)


def test_no_frames_is_a_no_op(mv):
    import torch
    g = mv.DepanStabilise(206, 118, num_frames=4, prev=1, next=1)
    full, out = dc.guarded(g, 1)
    g.launch((mv.DepanStabiliseJob * 0)())
    assert g.run([], []) == []
    torch.cuda.synchronize()
    assert all(bool((t == 0xA5).all()) for t in full[0])
