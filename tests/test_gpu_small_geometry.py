"""GPU parity on the geometries nobody ran: tiny clips with no padding or a padding below the chroma ratio, byte for byte against the
oracle.  mv.Super at 8 and 16 bits with padding 0, 1 and (2, 0); mv.Analyse with every level's record compared (the coarsest level is where
a block's legal rectangle is empty and the clipped predictors lie left of and above the level: tests/small_geometry_cases.py), through every
kernel family that can take the geometry; mv.Recalculate and mv.Degrain on those vectors.

The first case of test_search is the search that once ended in an illegal memory access (8-bit 36x36 Gray, no padding, pel 2, blocks 8/4):
an unsigned 32-bit offset that wrapped for the clipped predictor (-1, -1) of the coarsest level.  tests/test_search_addressing.py finds
that on the CPU and shows the biased offsets clean; csrc/mvx_analyse_addr.h has the rule."""
import ctypes as C

import numpy as np
import pytest

import pipeline as pl
import small_geometry_cases as sg
from test_gpu_parity import dbg  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

NF = 5


def _np_super(mv, sup, frame):
    return [mv.plane_to_numpy(frame[p], sup.info.plane_width[p], sup.dtype) for p in range(sup.nplanes)]


def _launch(mv):
    info = (C.c_int * 5)()
    mv.lib().mvx_debug_last_launch(info)
    return list(info)


def _shadow_bad(mv, gsup, osup, fr):
    """the shadow data behind the planes of a built super frame, inside the defined regions: the luma copy shifted left by one sample (clips of
    more than 8 bits) and the UV-interleaved plane -- what the lean and the speculative kernels actually load"""
    import torch
    bad = []
    if not gsup.shadow:
        return bad
    i = gsup.info

    def area(p):
        t = fr[p]
        raw = torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage(), t.storage_offset(), (gsup.shadow_stride[p] * gsup.slots[p],))
        return raw.cpu().numpy()

    def rows(a, off, h, pitch):
        return a[off:off + h * pitch].reshape(h, pitch).view(gsup.dtype)
    a0 = area(0)
    plane = rows(a0, 0, i.plane_height[0], gsup.pitch[0])
    if gsup.slots[0] > 1:
        copy = rows(a0, gsup.shadow_stride[0], i.plane_height[0], gsup.pitch[0])
        for (p, lv, k, y0, x0, h, w) in osup.defined_regions():
            if p == 0 and not np.array_equal(copy[y0:y0 + h, x0:x0 + w - 1], plane[y0:y0 + h, x0 + 1:x0 + w]):
                xs = np.nonzero(copy[y0:y0 + h, x0:x0 + w - 1] != plane[y0:y0 + h, x0 + 1:x0 + w])[1]
                bad.append(("luma copy", lv, k, int(xs.min()), int(xs.max()), w))
    if gsup.nplanes == 3 and gsup.slots[1] > 1:
        a1 = area(1)
        u = rows(a1, 0, i.plane_height[1], gsup.pitch[1])
        v = rows(area(2), 0, i.plane_height[2], gsup.pitch[2])
        uv = rows(a1, gsup.shadow_stride[1], i.plane_height[1], 2 * gsup.pitch[1])
        for (p, lv, k, y0, x0, h, w) in osup.defined_regions():
            if p == 1 and not (np.array_equal(uv[y0:y0 + h, 2 * x0:2 * (x0 + w):2], u[y0:y0 + h, x0:x0 + w]) and np.array_equal(uv[y0:y0 + h, 2 * x0 + 1:2 * (x0 + w):2], v[y0:y0 + h, x0:x0 + w])):
                bad.append(("uv plane", lv, k, w))
    return bad


SUPER_CLIPS = [(36, 36, "gray"), (36, 36, "420"), (35, 30, "444"), (70, 54, "gray"), (70, 54, "420"), (72, 40, "420"), (16, 16, "420")]


@pytest.mark.parametrize("bits", (8, 16))
@pytest.mark.parametrize("w,h,fmt", SUPER_CLIPS)
def test_super(oracle, mv, w, h, fmt, bits):
    """every padding below the chroma ratio x pel 1 / 2 / 4, with the shadow planes and (16 bits) without; the 8-bit rows kernels at hpad = 0.
    The shadow data is compared too: at 16 bits, sharp 2 and no padding the fused build once wrote column XB - 1 of the shifted copy of the H and HV
    planes with the interior filter where the plane has the edge rule (widths of 4 modulo 8: 36)"""
    g0 = sg.geometry(w, h, fmt, bits, 2, (0, 0), (8, 4))
    frames = sg.clip(g0, 2)
    dev = [mv.frame_to_device(f) for f in frames]
    for pad in sg.PADS:
        for pel in (1, 2, 4):
            for shadow in ((True, False) if bits == 16 else (True,)):
                kw = dict(subsampling=sg.SUB[fmt], gray=fmt == "gray", pel=pel, hpad=pad[0], vpad=pad[1])
                osup, gsup = oracle.Super(w, h, bits, **kw), mv.Super(w, h, bits, shadow=shadow, **kw)
                assert (gsup.info.super_width, gsup.info.super_height, gsup.info.levels) == (osup.s.superWidth, osup.s.superHeight, osup.s.levels)
                out = gsup.build(dev)
                for f in range(2):
                    bad = pl.defined_equal(osup, osup.frame(frames[f]), _np_super(mv, gsup, out[f]))
                    assert not bad, "pad %s pel %d shadow %s frame %d (plane, level, pelplane, count, y, x, oracle, gpu): %s" % (pad, pel, shadow, f, bad[:4])
                    bad = _shadow_bad(mv, gsup, osup, out[f])
                    assert not bad, "pad %s pel %d frame %d: shadow data differs from its plane (what, level, pelplane, ...): %s" % (pad, pel, f, bad[:4])


def _searched(oracle, mv, g):
    """the clip's super frames on both sides, and per variant the oracle's blobs of all NF frames"""
    frames = sg.clip(g, NF)
    osup, _ = sg.make(oracle, g, NF)
    gsup, _ = sg.make(mv, g, NF)
    osf = [osup.frame(f) for f in frames]
    gsrc = [mv.frame_to_device(f) for f in frames]
    gsf = gsup.build(gsrc)
    return frames, osup, gsup, osf, gsrc, gsf


def _ref(v, n):
    r = n + (v["delta"] if v["isb"] else -v["delta"])
    return r if 0 <= r < NF else None


def _search_case(oracle, mv, dbg, g, routes=None):
    frames, osup, gsup, osf, gsrc, gsf = _searched(oracle, mv, g)
    ran = []
    for v in sg.VARIANTS:
        if g["fmt"] == "gray" and "chroma" in v:
            continue
        _, oan = sg.make(oracle, g, NF, **v)
        _, gan = sg.make(mv, g, NF, **v)
        want = [oan.frame(osf[n], osf[_ref(v, n)] if _ref(v, n) is not None else None) for n in range(NF)]
        jobs = [(gsf[n], gsf[_ref(v, n)] if _ref(v, n) is not None else None) for n in range(NF)]
        route = gan.levels()[0][23]
        for rid, opts, kind in sg.routes(g, route):
            if routes is not None and rid not in routes:
                continue
            for k in ("general", "cpw1"):
                dbg(k, opts.get(k, 0))
            dbg("spec", opts.get("spec", 1))
            dbg("team", opts.get("team", -1))
            got = gan.run(jobs)
            info = _launch(mv)
            if rid in ("general", "cpw1"):
                assert info[0] == 0 and info[4] == 0, (rid, info)
            else:
                assert info[0] >= 1 and (kind is None or info[4] == kind), (rid, info)  # never silently the general kernel
            for n in range(NF):
                b = got[n].cpu().numpy()
                assert np.array_equal(b, want[n]), "%s %s route %s frame %d: blob differs from the oracle's at byte %d of %d" % (
                    g["name"], v, rid, n, int(np.nonzero(b != want[n])[0][0]), len(b))
            ran.append(rid)
    return ran


def test_search_that_faulted(oracle, mv, dbg):
    """8-bit 36x36 Gray, no padding, pel 2, blocks 8/4, isb = 1, 5 frames -- as the library launches it by default, nothing else"""
    assert "spec1" in _search_case(oracle, mv, dbg, sg.FAULTING, routes=("spec1",))


@pytest.mark.parametrize("g", sg.GPU_SEARCHES, ids=[g["name"] for g in sg.GPU_SEARCHES])
def test_search(oracle, mv, dbg, g):
    """every level's record of every blob, isb 0 / 1, delta 1 / 2 (references outside the clip at both ends), chroma and global on and off,
    through the general kernels (four chains and one per workgroup), the lean kernel, the speculative kernel in its four forms and as teams"""
    ran = _search_case(oracle, mv, dbg, g)
    assert "general" in ran and "cpw1" in ran
    # the lean and the speculative kernels take every 4:2:0 / Gray geometry here but the pel-4 ones (searched at pelsearch 4: mvx_fast_eligible),
    # which -- like 4:4:4 -- are the general kernels' alone; mvx_analyse_debug_level says so, and the expectation is written down here, not read there
    _, gan = sg.make(mv, g, NF)
    lean = g["fmt"] != "444" and g["akw"].get("pelsearch", g["skw"]["pel"]) != 4
    assert gan.levels()[0][23] == (2 if lean else 0 if g["fmt"] == "444" else 1)
    if lean:
        assert {"spec0", "spec1", "spec2", "spec3", "spec5", "team2", "team4"} <= set(ran), ran


CONSUMERS = [sg.FAULTING, sg.geometry(36, 36, "420", 16, 2, (0, 0), (8, 4)), sg.geometry(36, 36, "420", 16, 2, (0, 0), (8, 4), shadow=False),
             sg.geometry(70, 54, "420", 8, 2, (0, 0), (8, 4)), sg.geometry(70, 54, "420", 16, 2, (1, 1), (8, 4))]


@pytest.mark.parametrize("g", CONSUMERS, ids=[g["name"] for g in CONSUMERS])
def test_recalculate_and_degrain(oracle, mv, g):
    """the consumers on an unpadded frame's vectors: mv.Recalculate (blocks 4/2 on the searched field) and mv.Degrain1 -- at 16 bits its blocks
    at odd sample positions come from the shifted luma copy -- for a frame inside the clip and for frame 0, whose forward reference is missing"""
    import torch
    frames, osup, gsup, osf, gsrc, gsf = _searched(oracle, mv, g)
    gray = g["fmt"] == "gray"
    for target in (2, 0):
        ob, gb, oref, gref = [], [], [], []
        for isb in (1, 0):
            _, oan = sg.make(oracle, g, NF, isb=isb)
            _, gan = sg.make(mv, g, NF, isb=isb)
            r = target + (1 if isb else -1)
            r = r if 0 <= r < NF else None
            oref.append(osf[r] if r is not None else None)
            gref.append(gsf[r] if r is not None else None)
            ob.append(oan.frame(osf[target], oref[-1]))
            gb.append(gan.run([(gsf[target], gref[-1])])[0])
            assert np.array_equal(gb[-1].cpu().numpy(), ob[-1])
            rkw = dict(blksize=4, overlap=2, thsad=60)
            orc = oracle.Recalculate(osup, oan.ad, **rkw)
            grc = mv.Recalculate(gsup, gan.ad, **rkw)
            assert np.array_equal(grc.run([(gsf[target], gref[-1], gb[-1])])[0].cpu().numpy(), orc.frame(osf[target], oref[-1], ob[-1])), (target, isb)
        want = oracle.Degrain(1, osup, oan.ad).frame(frames[target], oref, ob)
        got = mv.Degrain(1, gsup, gan.ad, [p.stride(0) for p in gsrc[0]]).run([(gsrc[target], gref, gb)])[0]
        torch.cuda.synchronize()
        for p in range(1 if gray else 3):
            assert not pl.first_diff(mv.plane_to_numpy(got[p], want[p].shape[1], want[p].dtype), want[p]), (target, p)
