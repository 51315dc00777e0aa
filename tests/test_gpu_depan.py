"""GPU parity of mv.DepanCompensate (mvx_depan_warp.hip) and mv.DepanAnalyse (mvx_depan.hip) against the CPU restatement tests/depan_ref.py, through the Python
package.  Bit-exact on every sample of every plane; all frames of a case in ONE mvx_depan_compensate_frames call.  Every destination plane
is allocated with a guard row before and after it and filled with 0xA5: nothing but the samples may change.

The parity cases (tests/depan_cases.py) are in domain -- the restatement's strict mode raises nothing, which tests/test_depan_ref.py checks on
the CPU too -- and each names the counters it must reach.  The library-rule cases are out of domain on purpose and compared with the
restatement's library mode (mvtools_amd.h, divergences 2 and 5): defined behaviour, nothing here provokes a fault."""
import numpy as np
import pytest

import depan_cases as dc
import depan_ref as dr
import pipeline as pl
import vector_fields as vf

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 206, 118


def _run(mv, case):
    import torch
    src, want, stats = dc.expected(case)
    f = dc.FORMATS[case["fmt"]]
    dev = [mv.plane_to_device(p) for p in src]
    g = mv.DepanCompensate(case["w"], case["h"], case["bits"], f["subsampling"], f.get("gray", False), src_pitch=[d.stride(0) for d in dev], offset=1.0,
                           subpixel=case["sub"], mirror=case["mirror"], blur=case["blur"])
    full, out = dc.guarded(g, len(case["trs"]))
    g.run([dev] * len(case["trs"]), case["trs"], out=out)
    torch.cuda.synchronize()
    dc.check(full, want, g.dtype)
    return stats


@pytest.mark.parametrize("case", dc.CASES, ids=dc.ids(dc.CASES))
def test_compensate_parity(mv, case):
    stats = _run(mv, case)
    assert not dc.missing(case, stats), stats
    assert not stats.get("ood") and not stats.get("undef")


@pytest.mark.parametrize("case", dc.LIBRARY_CASES, ids=dc.ids(dc.LIBRARY_CASES))
def test_compensate_library_rule(mv, case):
    """mirrored shifts of at least the width, bilinear translation with inttr0 >= row_size - 2, positions beyond the int range and NaN:
    the border value where the reference's index leaves its row, and no byte outside the samples"""
    stats = _run(mv, case)
    assert not dc.missing(case, stats), stats


@pytest.mark.parametrize("case", dc.FULL_CASES, ids=dc.ids(dc.FULL_CASES))
def test_compensate_parity_full_size(mv, case):
    """1920 x 1080 4:2:0 8-bit, the shape tools/depan_bench.py measures; the chain of the rotation form runs over 1920 columns"""
    stats = _run(mv, case)
    assert not dc.missing(case, stats), stats


def test_the_rotation_chain_is_not_the_direct_product(mv):
    """at 206 columns the last positions hold more than 200 accumulated roundings: the restatement's chain differs from x0 + k * dxx in this
    case, so the parity above cannot pass with the direct product"""
    case = next(c for c in dc.CASES if c["name"] == "rot_s1_8")
    _, _, stats = dc.expected(case)
    assert stats["chain_differs"] > 1000
    src, want, _ = dc.expected(case)
    chain = dr._chain

    def direct(pl_, t):
        hs, rs = np.arange(pl_.H, dtype=f32), np.arange(pl_.W, dtype=f32)
        return (t[0] + t[2] * hs)[:, None] + rs[None, :] * t[1], (t[3] + t[5] * hs)[:, None] + rs[None, :] * t[4]
    dr._chain = direct
    try:
        other = dc.expected(case)[1]
    finally:
        dr._chain = chain
    assert any(not np.array_equal(a, b) for fa, fb in zip(want, other) for a, b in zip(fa, fb)), "the direct product gives the same samples: the case proves nothing"


def test_no_frames_is_a_no_op(mv):
    import torch
    g = mv.DepanCompensate(W, H, offset=1.0)
    full, out = dc.guarded(g, 1)
    g.launch((mv.DepanCompensateJob * 0)())
    torch.cuda.synchronize()
    assert all(bool((t == 0xA5).all()) for t in full[0])
    assert mv.DepanAnalyse(mv.Analyse(mv.Super(W, H, 8), isb=0, delta=1).ad, W, H).run([]) == []


# ------------------------------------------------------------------------------------------------ DepanAnalyse through the gather kernel

def _gpu_vectors(mv, isb, nf=4, motion=(3, -1), blk=8, ov=4):
    frames = pl.moving_clip(W, H, 8, nf, seed=11, noise=2, motion=motion)
    sup = mv.Super(W, H, 8)
    devf = [mv.frame_to_device(f) for f in frames]
    sfs = sup.build(devf)
    an = mv.Analyse(sup, num_frames=nf, blksize=blk, overlap=ov, isb=isb, delta=1)
    jobs = []
    for n in range(nf):
        k = n + 1 if isb else n - 1
        jobs.append((sfs[n], sfs[k] if 0 <= k < nf else None))
    return frames, devf, an, an.run(jobs)


def _same(got, want):
    for k in ("dx", "dy", "zoom", "rot", "error"):
        assert f32(got[k]).tobytes() == f32(want[k]).tobytes(), (k, got, want)
    assert got["iter"] == want["iter"]


@pytest.mark.parametrize("isb", [0, 1])
@pytest.mark.parametrize("masked", [False, True])
def test_analyse_gather_equals_the_restatement(mv, isb, masked):
    """GPU Analyse blobs, a crafted blob uploaded again, an invalid one and a NULL blob in one batch: usable and unusable frames mixed"""
    import torch
    _, _, an, blobs = _gpu_vectors(mv, isb)
    ad = an.ad
    _, s1, s2 = vf.scaled_thresholds(ad, 400)
    host = [b.cpu().numpy() for b in blobs]
    crafted = vf.scene_count(host[1], ad, 3, s1, s2 + 1, 400)             # one block too many above thscd1
    edge = vf.scene_count(host[1], ad, 3, s1, s2, 400)                    # exactly thscd2
    host += [crafted, edge, vf.invalid(host[2], ad), None]
    dev = list(blobs) + [torch.from_numpy(b).cuda() for b in host[4:7]] + [None]
    n = len(dev)
    mask = np.random.default_rng(8).integers(0, 256, (H, W)).astype(np.uint8)
    mask[:, 100:] = 255
    dmask = mv.plane_to_device(mask)
    top = [k & 1 for k in range(n)]
    g = mv.DepanAnalyse(ad, W, H, mask=(8,) if masked else None, fields=1)
    got = g.run(dev, [dmask] * n if masked else None, top)
    assert got == g.run_host(host, [mask] * n if masked else None, top)
    ref = dr.Analyse(ad, W, H, s1, s2, fields=True, has_mask=masked)
    stats = {}
    for k in range(n):
        _same(got[k], ref.frame(host[k], mask if masked else None, bool(top[k]), stats))
    assert stats["unusable"] == 4 and bool(stats.get("inverse")) == bool(isb)   # no reference frame, the scene change, the invalid and the NULL blob
    assert got[5]["dx"] != 0.0 and got[4]["dx"] == 0.0
    if masked:
        assert stats.get("r_border", 0) == 0


def test_end_to_end_on_a_planted_pan(mv):
    """Super -> Analyse (delta 1, both directions) -> DepanAnalyse -> transform -> DepanCompensate at offset +1 and -1, equal to the
    restatement run on the same blobs"""
    import torch
    nf = 4
    frames, devf, an_f, blobs_f = _gpu_vectors(mv, 0, nf)
    _, _, an_b, blobs_b = _gpu_vectors(mv, 1, nf)
    _, s1, s2 = vf.scaled_thresholds(an_f.ad, 400)
    for an, blobs, isb in ((an_f, blobs_f, 0), (an_b, blobs_b, 1)):
        per_frame = [blobs[max(0, n - 1)] if isb else blobs[n] for n in range(nf)]        # :287
        motions = mv.DepanAnalyse(an.ad, W, H, num_frames=nf).run(per_frame)
        ref = dr.Analyse(an.ad, W, H, s1, s2)
        for n in range(nf):
            _same(motions[n], ref.frame(per_frame[n].cpu().numpy()))
        for offset in (1.0, -1.0):
            g = mv.DepanCompensate(W, H, src_pitch=[t.stride(0) for t in devf[0]], offset=offset, subpixel=2, mirror=15, num_frames=nf)
            src, trs, want = [], [], []
            for n in range(nf):
                m = g.map(n)
                assert m == dr.frame_map(offset, n, nf)
                if m is None:
                    continue
                ms = [(motions[k]["dx"], motions[k]["dy"], motions[k]["zoom"], motions[k]["rot"]) for k in range(m[1] + 1, m[2] + 1)]
                t, info = g.transform(ms)
                t_ref, info_ref = dr.motion_to_transform(ms, offset, W, H)
                assert t.tobytes() == t_ref.tobytes() and info.tobytes() == info_ref.tobytes()
                src.append(devf[m[0]])
                trs.append(t)
                want.append(dr.compensate_frame(frames[m[0]], t_ref, 2, 8, (1, 1), False, 15, 0, "strict"))
            assert len(src) == nf - 1
            full, out = dc.guarded(g, len(src))
            g.run(src, trs, out=out)
            torch.cuda.synchronize()
            dc.check(full, want, np.uint8)
        # the planted pan of (3, -1) per frame comes back from real vectors; backward vectors give the inverse motion
        assert abs(abs(motions[2]["dx"]) - 3) < 0.5 and abs(abs(motions[2]["dy"]) - 1) < 0.5
