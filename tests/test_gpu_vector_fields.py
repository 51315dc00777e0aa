"""GPU parity of every filter that consumes motion vectors on crafted vector fields (tests/vector_fields.py): vectors on the limits of their
legal rectangles, SADs on the thresholds and above 2^32, scene-change counts on thscd2, occlusions that span several blocks, invalid blobs.

The vectors come from the GPU's Analyse, are edited on the host and uploaded again; the oracle (Degrain, Compensate, BlockFPS, Recalculate)
or the restatement (tests/flow_ref.py, tests/flowmc_ref.py) gets the same edited bytes.  Bit-exact, every sample of every plane.
tests/test_vector_fields.py checks on the CPU that each field listed here is what its recipe claims."""
import itertools

import numpy as np
import pytest

import pipeline as pl
import test_gpu_flow as gflow
import test_gpu_flowmc as gflowmc
import vector_fields as vf
from test_gpu_parity import _pipeline

pytestmark = pytest.mark.gpu

ids = lambda cases: ["%d-%s" % (i, c[-1]) for i, c in enumerate(cases)]


def _upload(mv, edit, gblob, ad, index):
    """the edited bytes (numpy, for the CPU side) and their device copy"""
    import torch
    e = edit(gblob.cpu().numpy(), ad, index)
    return e, torch.from_numpy(e).to(gblob.device)


def _check(consumer, recipe, what, plane, got, want):
    d = pl.first_diff(got, want)
    if d:
        pytest.fail("%s on %r, %s plane %d: %s" % (consumer, recipe, what, plane, d))


def _numbered(edit):
    """edit(blob, ad) for the flow runners, which edit the backward clip's blobs and then the forward clip's: the i-th call gets index i"""
    count = itertools.count()
    return lambda blob, ad: edit(blob, ad, next(count))


def _named(consumer, recipe, fn):
    try:
        return fn()
    except AssertionError as e:
        pytest.fail("%s on %r: %s" % (consumer, recipe, e))


# ------------------------------------------------------------------ Degrain

def _degrain(oracle, mv, w, h, bits, radius, skw, akw, dkw, recipe):
    import torch
    frames, osup, gsup, osf, gsrc, gsf = _pipeline(oracle, mv, w, h, bits, radius, skw, akw, seed=23)
    target = radius
    edit = vf.case_editor("degrain", recipe, dkw)
    oblobs, gblobs, refs_o, refs_g = [], [], [], []
    for d in range(1, radius + 1):
        for isb in (1, 0):
            gan = mv.Analyse(gsup, isb=isb, delta=d, **akw)
            nref = target + (d if isb else -d)
            e, g = _upload(mv, edit, gan.run([(gsf[target], gsf[nref])])[0], gan.ad, len(gblobs))
            oblobs.append(e)
            gblobs.append(g)
            refs_o.append(osf[nref])
            refs_g.append(gsf[nref])
    odg = oracle.Degrain(radius, osup, gan.ad, **dkw)
    gdg = mv.Degrain(radius, gsup, gan.ad, [p.stride(0) for p in gsrc[0]], **dkw)
    want = odg.frame(frames[target], refs_o, oblobs)
    got = gdg.run([(gsrc[target], refs_g, gblobs)])[0]
    torch.cuda.synchronize()
    for p in range(3):
        _check("Degrain%d" % radius, recipe, "%dx%d %d bit" % (w, h, bits), p, mv.plane_to_numpy(got[p], want[p].shape[1], want[p].dtype), want[p])
    return frames[target], want


@pytest.mark.parametrize("w,h,bits,radius,skw,akw,dkw,recipe", vf.DEGRAIN_CASES, ids=ids(vf.DEGRAIN_CASES))
def test_degrain_on_crafted_fields(oracle, mv, w, h, bits, radius, skw, akw, dkw, recipe):
    src, want = _degrain(oracle, mv, w, h, bits, radius, skw, akw, dkw, recipe)
    if recipe.name == "invalid" and recipe.kw.get("only") is None or recipe.name == "scene_count" and recipe.kw.get("over") and recipe.kw.get("only") is None:
        assert all(np.array_equal(a, b) for a, b in zip(src, want)), "no reference is usable: the source frame"
    else:
        assert not np.array_equal(src[0], want[0]), "the field does not reach the output"


def test_degrain3_full_size_on_limits(oracle, mv):
    """4K 16-bit blk 16/8, one output frame: the launch shape of the benchmark"""
    _degrain(oracle, mv, *vf.FULL_DEGRAIN)


# ------------------------------------------------------------------ Compensate

@pytest.mark.parametrize("w,h,bits,skw,akw,ckw,shift,recipe", vf.COMPENSATE_CASES, ids=ids(vf.COMPENSATE_CASES))
def test_compensate_on_crafted_fields(oracle, mv, w, h, bits, skw, akw, ckw, shift, recipe):
    import torch
    frames, osup, gsup, osf, gsrc, gsf = _pipeline(oracle, mv, w, h, bits, 1, skw, akw, nframes=2, seed=25)
    fields = dict(fields=1) if shift is not None else {}
    gan = mv.Analyse(gsup, isb=1, **dict(akw, **fields))
    gb = gan.run([(gsf[0], gsf[1])], **(dict(field_shift=shift) if fields else {}))[0]
    edit = vf.case_editor("compensate", recipe, ckw)
    e, g = _upload(mv, edit, gb, gan.ad, 0)
    oc = oracle.Compensate(osup, gan.ad, **ckw)
    gc = mv.Compensate(gsup, gan.ad, **dict(ckw, **fields))
    want = oc.frame(osf[0], osf[1], e, field_shift=shift or 0)
    got = gc.run([(gsf[0], gsf[1], g, shift) if fields else (gsf[0], gsf[1], g)])[0]
    torch.cuda.synchronize()
    for p in range(3):
        _check("Compensate", recipe, "%dx%d %d bit shift %s" % (w, h, bits, shift), p, mv.plane_to_numpy(got[p], want[p].shape[1], want[p].dtype), want[p])
    if fields:
        assert not all(np.array_equal(a, b) for a, b in zip(want, oc.frame(osf[0], osf[1], e))), "the field shift does not reach the output"


# ------------------------------------------------------------------ BlockFPS

@pytest.mark.parametrize("w,h,bits,akw,bkw,recipe", vf.BLOCKFPS_CASES, ids=ids(vf.BLOCKFPS_CASES))
def test_blockfps_on_crafted_fields(oracle, mv, w, h, bits, akw, bkw, recipe):
    import torch
    akw = dict(akw)
    delta = akw.pop("delta", 1)
    nf = 3 + delta
    frames, osup, gsup, osf, gsrc, gsf = _pipeline(oracle, mv, w, h, bits, 1, {}, akw, nframes=nf, seed=43)
    gabw = mv.Analyse(gsup, num_frames=nf, isb=1, delta=delta, **akw)
    gafw = mv.Analyse(gsup, num_frames=nf, isb=0, delta=delta, **akw)
    gbbw = gabw.run([(gsf[n], gsf[n + delta] if n + delta < nf else None) for n in range(nf)])
    gbfw = gafw.run([(gsf[n], gsf[n - delta] if n - delta >= 0 else None) for n in range(nf)])
    edit = vf.case_editor("blockfps", recipe, bkw)
    bw = [_upload(mv, edit, b, gabw.ad, i) for i, b in enumerate(gbbw)]
    fw = [_upload(mv, edit, b, gafw.ad, nf + i) for i, b in enumerate(gbfw)]
    ob = oracle.BlockFPS(osup, gabw.ad, gafw.ad, nf, 24, 1, **bkw)
    gb = mv.BlockFPS(gsup, gabw.ad, gafw.ad, nf, [p.stride(0) for p in gsrc[0]], 24, 1, **bkw)
    assert gb.num_frames == ob.num_frames
    ns = list(range(gb.num_frames))
    for n in ns:
        assert gb.map(n) == ob.map(n)
    out = gb.run(ns, gsrc, gsf, [g for _, g in bw], [g for _, g in fw])
    torch.cuda.synchronize()
    for n in ns:
        want = ob.frame(n, frames, osf, [e for e, _ in bw], [e for e, _ in fw])
        for p in range(3):
            _check("BlockFPS mode %s" % bkw.get("mode"), recipe, "output %d %s" % (n, gb.map(n)), p, mv.plane_to_numpy(out[n][p], want[p].shape[1], want[p].dtype), want[p])


# ------------------------------------------------------------------ Recalculate

@pytest.mark.parametrize("bits,pel_old,pel_new,akw,rkw,recipe", vf.RECALC_CASES, ids=ids(vf.RECALC_CASES))
def test_recalculate_on_crafted_old_vectors(oracle, mv, bits, pel_old, pel_new, akw, rkw, recipe):
    import torch
    w, h, nf = 192, 128, 2
    frames, osup_old, gsup_old, osf_old, gsrc, gsf_old = _pipeline(oracle, mv, w, h, bits, 1, dict(pel=pel_old), {}, nframes=nf, seed=55)
    if pel_new == pel_old:
        osup, gsup, osf, gsf = osup_old, gsup_old, osf_old, gsf_old
    else:
        osup, gsup = oracle.Super(w, h, bits, pel=pel_new), mv.Super(w, h, bits, pel=pel_new)
        osf, gsf = [osup.frame(f) for f in frames], gsup.build(gsrc)
    gan = mv.Analyse(gsup_old, num_frames=nf, isb=1, **akw)
    gold = gan.run([(gsf_old[n], gsf_old[n + 1] if n + 1 < nf else None) for n in range(nf)])
    orc = oracle.Recalculate(osup, gan.ad, **rkw)
    grc = mv.Recalculate(gsup, gan.ad, **rkw)
    assert grc.blob_size == orc.blob_size
    edit = vf.case_editor("recalculate", recipe, rkw, orc)
    old = [_upload(mv, edit, b, gan.ad, i) for i, b in enumerate(gold)]
    got = grc.run([(gsf[n], gsf[n + 1] if n + 1 < nf else None, old[n][1]) for n in range(nf)])
    torch.cuda.synchronize()
    for n in range(nf):
        want = orc.frame(osf[n], osf[n + 1] if n + 1 < nf else None, old[n][0])
        g = got[n].cpu().numpy()
        if not np.array_equal(g, want):
            msg = ["Recalculate on %r, frame %d: %d bytes differ" % (recipe, n, int(np.count_nonzero(g != want)))]
            (gx, gy, gs), (wx, wy, ws) = pl.blob_vectors(g, grc.ad), pl.blob_vectors(want, orc.ad)
            d = (gx != wx) | (gy != wy) | (gs != ws)
            if d.any():
                y, x = [int(v[0]) for v in np.nonzero(d)]
                msg.append("level 0: %d of %d blocks differ, first (by=%d, bx=%d) got (%d, %d, %d) want (%d, %d, %d)" % (
                    int(d.sum()), d.size, y, x, gx[y, x], gy[y, x], gs[y, x], wx[y, x], wy[y, x], ws[y, x]))
            pytest.fail("; ".join(msg))


# ------------------------------------------------------------------ FlowInter, FlowFPS

def _flow_editor(recipe, fkw):
    return _numbered(vf.case_editor("flowinter", recipe, fkw))


@pytest.mark.parametrize("fmt,w,h,bits,skw,akw,fkw,recipe", vf.FLOWINTER_CASES, ids=ids(vf.FLOWINTER_CASES))
def test_flowinter_flowfps_on_crafted_fields(oracle, mv, fmt, w, h, bits, skw, akw, fkw, recipe):
    kinds = _named("FlowFPS" if fkw.get("fps") else "FlowInter", recipe,
                   lambda: gflow._run(mv, oracle, fmt, w, h, bits, skw, akw, fkw, nf=4, seed=97, edit=_flow_editor(recipe, fkw)))
    kinds = set(kinds.split(",")) - {"copy"}
    if recipe.name == "scene_count" and recipe.kw.get("over"):
        assert kinds == {"blend"}, kinds
    else:
        assert kinds & {"extra", "regular", "simple", "extra128", "regular128", "simple128"}, kinds


def test_flowfps_full_size_on_limits(oracle, mv):
    """1080p 8-bit, FlowFPS 2x mask=2, the output between frames 1 and 2 (all four blobs usable: Extra)"""
    fmt, w, h, bits, skw, akw, fkw, recipe = vf.FULL_FLOWFPS
    kinds = _named("FlowFPS", recipe, lambda: gflow._run(mv, oracle, fmt, w, h, bits, skw, akw, fkw, nf=4, seed=99, outs=[3], edit=_flow_editor(recipe, fkw)))
    assert kinds == "extra128"


# ------------------------------------------------------------------ Flow, FlowBlur

@pytest.mark.parametrize("fmt,w,h,bits,skw,akw,fkw,recipe", vf.FLOW_CASES, ids=ids(vf.FLOW_CASES))
def test_flow_on_crafted_fields(oracle, mv, fmt, w, h, bits, skw, akw, fkw, recipe):
    edit = _numbered(vf.case_editor("flow", recipe, fkw))
    kinds = _named("Flow", recipe, lambda: gflowmc._run_flow(mv, oracle, fmt, w, h, bits, skw, akw, fkw, nf=4, seed=107, edit=edit)).split(",")
    if recipe.name == "scene_count" and recipe.kw.get("over"):
        assert kinds == ["copy"], kinds
    elif fkw.get("mode"):
        assert "shift" in kinds and "collide" in kinds and "hole" in kinds, kinds
    else:
        assert "fetch" in kinds, kinds


@pytest.mark.parametrize("fmt,w,h,bits,skw,akw,fkw,recipe", vf.BLUR_CASES, ids=ids(vf.BLUR_CASES))
def test_flowblur_on_crafted_fields(oracle, mv, fmt, w, h, bits, skw, akw, fkw, recipe):
    edit = _numbered(vf.case_editor("flowblur", recipe, fkw))
    kinds = _named("FlowBlur", recipe, lambda: gflowmc._run_blur(mv, oracle, fmt, w, h, bits, skw, akw, fkw, nf=4, seed=109, edit=edit)).split(",")
    assert "blur" in kinds and "taps" in kinds and "trunc" in kinds, kinds
