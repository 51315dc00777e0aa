"""The cases of tests/sample_range.py reach what they claim -- shown through the oracle alone, on the CPU.

A GPU case that never clamps, never saturates a limit or never brings the penalty product past 2^31 proves nothing about those
paths however bit-exact it is; these are the conditions (not measurements) that make tests/test_gpu_sample_range.py worth its time."""
import functools
import os
import subprocess

import numpy as np
import pytest

import pipeline as pl
import sample_range as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ generators
@pytest.mark.parametrize("bits", sr.DEPTHS)
def test_generators_reach_both_rails(bits):
    pm = (1 << bits) - 1
    for sub in ((1, 1), (0, 0), (1, 0)):
        fr = sr.rails(136, 72, bits, 2, sub=sub)
        for p in range(3):
            assert fr[0][p].shape == (72 >> (sub[1] if p else 0), 136 >> (sub[0] if p else 0)) and fr[0][p].dtype == (np.uint8 if bits == 8 else np.uint16)
            v = fr[0][p]
            assert (v == 0).mean() >= 0.1 and (v == pm).mean() >= 0.1, (bits, sub, p, (v == 0).mean(), (v == pm).mean())
            between = v[(v > 0) & (v < pm)]
            assert between.size >= 0.2 * v.size and len(np.unique(between)) >= 16, "real texture between the rails"  # (8-bit chroma at gain 8: at most 31 levels)
    ck = sr.checker(136, 72, bits, 3)
    for f in range(3):
        for p in range(3):
            assert set(np.unique(ck[f][p]).tolist()) == {0, pm}
    assert np.array_equal(ck[1][0][1:, 2:], ck[0][0][:-1, :-2]) and np.array_equal(ck[2][1][1:, 2:], ck[1][1][:-1, :-2])  # moves by (2, 1)
    assert (ck[0][0][:3, :3] == ck[0][0][0, 0]).all() and (ck[0][0][:3, 3:6] == pm - ck[0][0][0, 0]).all() and (ck[0][0][3:6, :3] == pm - ck[0][0][0, 0]).all()
    lo, hi = pm // 8, pm - pm // 16
    st = sr.step(128, 96, bits, 3, lo, hi)
    amp = (1 << bits) // 32
    for p in range(3):
        assert st[0][p].min() >= lo and st[0][p].max() <= lo + amp and st[2][p].max() <= lo + amp
        assert st[1][p].max() <= hi and st[1][p].min() >= hi - amp
        assert len(np.unique(st[0][p])) > min(amp, 8)
    assert not np.array_equal(st[0][0], st[2][0])
    full = sr.step(64, 32, bits, 2, 0, pm)  # levels AT the ends: the noise is pulled inwards, nothing wraps
    assert full[0][0].max() <= amp and pm - amp <= full[1][0].min() and full[1][0].max() <= pm


# ----------------------------------------------------------------------------------------------------------------- Super
def _subpel_values(osup, frame):
    out = []
    for (p, lv, k, y0, x0, h, w) in osup.defined_regions():
        if lv == 0 and k > 0:
            out.append(frame[p][y0:y0 + h, x0:x0 + w].ravel())
    return np.concatenate(out)


@pytest.mark.parametrize("gen,w,h,bits,sub,kw", sr.super_overshoot_cases())
def test_super_cases_overshoot(oracle, gen, w, h, bits, sub, kw):
    """the same samples through a 16-bit Super: values above pm inside the defined sub-pel planes = what the real depth's clamp must
    cut; the real-depth Super holds pm and 0 there"""
    pm = (1 << bits) - 1
    frames = sr.make(gen, w, h, bits, 2, sub=sub)
    wide = oracle.Super(w, h, 16, subsampling=sub, **kw)
    real = oracle.Super(w, h, bits, subsampling=sub, **kw)
    for f in frames:
        over = _subpel_values(wide, wide.frame(sr.widen([f])[0]))
        assert int((over > pm).sum()) > 0, "no sample above pm: the clamp at pm is never exercised"
        v = _subpel_values(real, real.frame(f))
        assert v.max() == pm and v.min() == 0
        assert int((v == pm).sum()) >= int((over > pm).sum())


@pytest.mark.parametrize("bits", [10, 12, 14])
def test_super_checker_overshoot_counts(oracle, bits):
    """the overshoot does not depend on the depth (the taps scale), and bilinear (sharp 0) never overshoots"""
    pm = (1 << bits) - 1
    f = sr.checker(136, 72, bits, 1)[0]
    counts = {}
    for pel in (2, 4):
        for sharp in (0, 1, 2):
            wide = oracle.Super(136, 72, 16, pel=pel, sharp=sharp)
            counts[(pel, sharp)] = int((_subpel_values(wide, wide.frame(sr.widen([f])[0])) > pm).sum())
    f10 = sr.checker(136, 72, 10, 1)[0]
    for (pel, sharp), n in counts.items():
        wide = oracle.Super(136, 72, 16, pel=pel, sharp=sharp)
        assert n == int((_subpel_values(wide, wide.frame(sr.widen([f10])[0])) > 1023).sum()), (pel, sharp)
        assert (n == 0) == (sharp == 0), (pel, sharp, n)
    assert counts[(4, 2)] > 4 * counts[(2, 2)] > 0


# --------------------------------------------------------------------------------------------------------------- Analyse
def _penalty_products(case):
    name, bits, sub, lo, hi, akw = case
    frames = sr.step(sr.STEP_W, sr.STEP_H, bits, 2, lo, hi, sub=sub)
    pnew = akw.get("pnew", 50)  # truemotion's default (MVAnalyse.c:359)
    sad = sr.zero_vector_luma_sad(frames, akw["blksize"], akw["overlap"])
    return frames, pnew, sad


@pytest.mark.parametrize("case", sr.PENALTY_CASES, ids=lambda c: c[0])
def test_penalty_cases_pass_2_31(oracle, case):
    frames, pnew, sad = _penalty_products(case)
    assert sad.shape[0] >= 3 and sad.shape[1] >= 3
    assert sad.max() < 1 << 27, "the sum's bound: a block SAD stays below 2^27"
    assert (pnew * sad >= 1 << 31).mean() >= 0.5, "pnew * SAD below 2^31 on most blocks: a 32-bit product would not wrap"
    # the oracle's own level-0 SADs (luma + chroma, whatever vector it ends on) are of that size too: no candidate is much better than the zero vector
    name, bits, sub, lo, hi, akw = case
    osup = oracle.Super(sr.STEP_W, sr.STEP_H, bits, subsampling=sub)
    oan = oracle.Analyse(osup, isb=1, **akw)
    osf = [osup.frame(f) for f in frames]
    x, y, s = pl.blob_vectors(oan.frame(osf[0], osf[1]), oan.ad, 0)
    assert s.shape == sad.shape and (pnew * s >= 1 << 31).mean() >= 0.5 and (s >= sad * 15 // 16).all()


def test_penalty_444_case_passes_2_31_in_chroma_only():
    name, bits, sub, lo, hi, akw = sr.PENALTY_444_CASE
    frames, pnew, sad = _penalty_products(sr.PENALTY_444_CASE)
    csad = sum(sr.zero_vector_luma_sad([[f[p]] for f in frames], akw["blksize"], akw["overlap"]) for p in (1, 2))
    assert (pnew * sad < 1 << 31).all() and (pnew * csad >= 1 << 31).all() and csad.max() < 1 << 27


@pytest.mark.parametrize("case", sr.CONTROL_CASES, ids=lambda c: c[0])
def test_control_cases(case):
    name, bits, sub, lo, hi, akw = case
    frames, pnew, sad = _penalty_products(case)
    if bits == 16:  # the largest block SAD there is: just below 2^27 (the sum's bound)
        assert (1 << 26) - (1 << 22) < sad.min() and sad.max() < 1 << 27
    else:           # cannot pass 2^31, chroma included
        csad = sum(sr.zero_vector_luma_sad([[f[p]] for f in frames], akw["blksize"] // 2, akw["overlap"] // 2) for p in (1, 2))
        assert (pnew * sad).max() < 1 << 31 and (pnew * csad).max() < 1 << 31
        assert 256 * (16 * 16 * ((1 << bits) - 1)) < 1 << 31


@pytest.mark.parametrize("name,bits,akw", sr.RAILS_ANALYSE_CASES, ids=lambda c: c if isinstance(c, str) else None)
def test_rails_search_still_finds_the_motion(oracle, name, bits, akw):
    frames = sr.rails(sr.RAILS_W, sr.RAILS_H, bits, 2, noise=3)
    osup = oracle.Super(sr.RAILS_W, sr.RAILS_H, bits)
    oan = oracle.Analyse(osup, isb=1, **akw)
    osf = [osup.frame(f) for f in frames]
    x, y, s = pl.blob_vectors(oan.frame(osf[0], osf[1]), oan.ad, 0)
    assert x.shape[0] >= 3 and x.shape[1] >= 3
    hit = (np.abs(x) == 6) & (np.abs(y) == 2)  # (3, -1) px per frame at pel 2
    assert hit.mean() > 0.5, hit.mean()
    if "badsad" in akw:  # the rescue runs: some block's SAD is above badsad after the normal search (scaled as MVAnalyse.c:436)
        assert (s > akw["badsad"] * (akw["blksize"] ** 2) // 64 * (1 << (bits - 8))).any()


# ------------------------------------------------------------------------------------------------- Degrain and Compensate
def _consumer_clip(gen, w, h, bits, nframes):
    if gen == "step":
        lo, hi = sr.STEP_SPAN[bits]
        return sr.step(w, h, bits, nframes, lo, hi)
    return sr.make(gen, w, h, bits, nframes)


def _oracle_degrain(oracle, gen, w, h, bits, radius, akw, dkw):
    frames = _consumer_clip(gen, w, h, bits, 2 * radius + 1)
    osup = oracle.Super(w, h, bits)
    osf = [osup.frame(f) for f in frames]
    blobs, refs = [], []
    for d in range(1, radius + 1):
        for isb in (1, 0):
            oan = oracle.Analyse(osup, isb=isb, delta=d, **akw)
            nref = radius + (d if isb else -d)
            blobs.append(oan.frame(osf[radius], osf[nref]))
            refs.append(osf[nref])
    return frames[radius], oracle.Degrain(radius, osup, oan.ad, **dkw).frame(frames[radius], refs, blobs)


@pytest.mark.parametrize("gen,w,h,bits,radius,akw,dkw", [c for c in sr.DEGRAIN_CASES if c[0] == "rails"])
def test_degrain_rails_cases_reach_both_ends(oracle, gen, w, h, bits, radius, akw, dkw):
    pm = (1 << bits) - 1
    src, out = _oracle_degrain(oracle, gen, w, h, bits, radius, akw, dkw)
    for p in range(3):
        assert out[p].min() == 0 and out[p].max() == pm, (p, out[p].min(), out[p].max())
    if dkw:
        _, free = _oracle_degrain(oracle, gen, w, h, bits, radius, akw, {})
        for p in range(3):
            lim = dkw["limit"] if p == 0 else dkw["limitc"]
            s, o, u = src[p].astype(np.int64), out[p].astype(np.int64), free[p].astype(np.int64)
            assert ((u < s - lim) & (o == s - lim)).any() and ((u > s + lim) & (o == s + lim)).any(), "no sample held at a limit (plane %d)" % p
            # the bounds themselves leave the range, and there the filter did change the sample: s - limit < 0 and s + limit > pm must not wrap
            assert ((s - lim < 0) & (u != s)).any() and ((s + lim > pm) & (u != s)).any(), "no limit bound outside [0, pm] (plane %d)" % p


@pytest.mark.parametrize("gen,w,h,bits,radius,akw,dkw", [c for c in sr.DEGRAIN_CASES if c[0] == "checker"])
def test_degrain_checker_cases_blend_and_hold_the_limits(oracle, gen, w, h, bits, radius, akw, dkw):
    """the references stay in the blend (the output differs from the source in every plane), and with limits a sample of 0 ends on
    0 + limit and a sample of pm on pm - limit"""
    pm = (1 << bits) - 1
    src, out = _oracle_degrain(oracle, gen, w, h, bits, radius, akw, dkw)
    for p in range(3):
        s, o = src[p].astype(np.int64), out[p].astype(np.int64)
        assert (o != s).mean() > 0.02, "plane %d: the references were not used" % p
        if "limit" in dkw:
            lim = dkw["limit"] if p == 0 else dkw["limitc"]
            assert ((s == 0) & (o == lim)).any() and ((s == pm) & (o == pm - lim)).any() and (np.abs(o - s) <= lim).all()
        else:
            assert (np.abs(o - s) > _limit_of(bits)).any()


def _limit_of(bits):
    return max(1, ((1 << bits) - 1) // 100)


@pytest.mark.parametrize("gen,w,h,bits,akw,ckw", [c for c in sr.COMPENSATE_CASES if c[0] == "rails" and not c[5]])
def test_compensate_rails_cases_reach_both_ends(oracle, gen, w, h, bits, akw, ckw):
    pm = (1 << bits) - 1
    frames = _consumer_clip(gen, w, h, bits, 2)
    osup = oracle.Super(w, h, bits)
    osf = [osup.frame(f) for f in frames]
    oan = oracle.Analyse(osup, isb=1, **akw)
    ob = oan.frame(osf[0], osf[1])
    out = oracle.Compensate(osup, oan.ad, **ckw).frame(osf[0], osf[1], ob)
    for p in range(3):
        assert out[p].min() == 0 and out[p].max() == pm
    tiny = oracle.Compensate(osup, oan.ad, thsad=1).frame(osf[0], osf[1], ob)
    assert not all(np.array_equal(a, b) for a, b in zip(out, tiny)), "thsad=1 must send blocks to the fallback"


# -------------------------------------------------------------------------------------------------------------- BlockFPS
def test_blockfps_occlusion_mask_is_mixed(oracle):
    """mode 5 writes the occlusion mask itself (MVBlockFPS.c:117-227): neither all 0 nor all 255 on the rails case of the GPU list, with that
    case's own parameters; its vector blobs are usable (an unusable pair is blended instead and no mask is made: the step cases)"""
    import ctypes as C
    gen, w, h, bits, akw, bkw = [c for c in sr.BLOCKFPS_CASES if c[5].get("mode") == 5][0]
    nf = 6
    frames = _consumer_clip(gen, w, h, bits, nf)
    osup = oracle.Super(w, h, bits)
    osf = [osup.frame(f) for f in frames]
    oabw, oafw = oracle.Analyse(osup, num_frames=nf, isb=1, **akw), oracle.Analyse(osup, num_frames=nf, isb=0, **akw)
    obbw = [oabw.frame(osf[n], osf[n + 1] if n + 1 < nf else None) for n in range(nf)]
    obfw = [oafw.frame(osf[n], osf[n - 1] if n >= 1 else None) for n in range(nf)]
    t1, t2 = C.c_int64(400), C.c_int(130)  # the defaults (MVBlockFPS.c:905-906), as the GPU case leaves them
    oracle.lib().mvo_scale_thscd(C.byref(t1), C.byref(t2), C.byref(oabw.d.ad))
    for b in obbw[:-1] + obfw[1:]:
        assert oracle.lib().mvo_blob_is_usable(C.byref(oabw.d.ad), C.c_void_p(b.ctypes.data), t1.value, t2.value)
    ob = oracle.BlockFPS(osup, oabw.ad, oafw.ad, nf, 24, 1, **bkw)
    masks = [ob.frame(n, frames, osf, obbw, obfw)[0] >> (bits - 8) for n in range(ob.num_frames) if ob.map(n)[2] not in (0, 256)]
    m = np.concatenate([x.ravel() for x in masks])
    assert (m > 0).any() and (m < 255).any() and len(np.unique(m)) > 2, np.unique(m)[:8]


# ---------------------------------------------------------------------------------------- FlowInter / FlowFPS, Flow, FlowBlur
# The runners below do on the CPU what those of tests/test_gpu_flow.py and tests/test_gpu_flowmc.py do on the GPU: the oracle's Super and
# Analyse (which the GPU's are pinned to, byte for byte) feed the restatements, the crafted fields are built through the same
# vector_fields.case_editor with the same blob indices.  What they report is therefore what the GPU case compares.
FORMATS = {"420": dict(subsampling=(1, 1)), "444": dict(subsampling=(0, 0)), "422": dict(subsampling=(1, 0)), "gray": dict(gray=True)}


def _flow_pipeline(oracle, gen, fmt, w, h, bits, skw, akw, isbs):
    """(frames, super, Finest frames by number, [analysis data, blobs per input frame] per direction); the cases that share it follow one another"""
    return _flow_pipeline_of(gen, fmt, w, h, bits, tuple(sorted(skw.items())), tuple(sorted(akw.items())), isbs)


@functools.lru_cache(maxsize=8)
def _flow_pipeline_of(gen, fmt, w, h, bits, skw, akw, isbs):
    import mvoracle as oracle
    nf = sr.FLOW_NF
    frames = sr.flow_clip(gen, fmt, w, h, bits)
    osup = oracle.Super(w, h, bits, **dict(FORMATS[fmt], **dict(skw)))
    osf = [osup.frame(f) for f in frames]
    fin = [osup.finest(f) for f in osf]
    akw = dict(akw)
    delta = akw.pop("delta", 1)
    vecs = []
    for isb in isbs:
        an = oracle.Analyse(osup, num_frames=nf, isb=isb, delta=delta, **akw)
        refs = [n + delta if isb else n - delta for n in range(nf)]
        vecs.append((an.ad, [an.frame(osf[n], osf[r] if 0 <= r < nf else None) for n, r in enumerate(refs)]))
    return frames, osup, fin, vecs


def _edited(consumer, recipe, fkw, vecs):
    """the blobs after the case's editor, numbered as the GPU runners number them: the backward clip's first, then the forward clip's"""
    if recipe is None:
        return [b for _, b in vecs]
    import vector_fields as vf
    edit, out, i = vf.case_editor(consumer, recipe, fkw), [], 0
    for ad, blobs in vecs:
        out.append([edit(b, ad, i + k) for k, b in enumerate(blobs)])
        i += len(blobs)
    return out


def _cpu_flowinter(oracle, case, probe=None, **override):
    import flow_ref
    gen, fmt, w, h, bits, skw, akw, fkw, recipe, _ = case
    fkw = dict(fkw, **override)
    frames, osup, fin, vecs = _flow_pipeline(oracle, gen, fmt, w, h, bits, skw, akw, (1, 0))
    bbw, bfw = _edited("flowinter", recipe, fkw, vecs)
    fkw = dict(fkw)
    fps = (24, 1) if fkw.pop("fps", None) else None
    ref = flow_ref.Flow(vecs[0][0], vecs[1][0], sr.FLOW_NF, osup.nplanes, osup.s.hpad, osup.s.vpad, fps=fps, **fkw)
    kinds, outs = set(), []
    for n in range(ref.num_frames):
        outs.append(ref.frame(n, frames, fin, bbw, bfw, probe))
        kinds.add(ref.last_kind)
    return ",".join(sorted(kinds)), frames, outs


def _cpu_flow(oracle, case, bits_of_the_hole=None):
    import flowmc_ref
    gen, fmt, w, h, bits, skw, akw, fkw, recipe, _ = case
    akw = dict(akw)
    isb = akw.pop("isb")
    frames, osup, fin, vecs = _flow_pipeline(oracle, gen, fmt, w, h, bits, skw, akw, (isb,))
    blobs, = _edited("flow", recipe, fkw, vecs)
    ref = flowmc_ref.Flow(vecs[0][0], sr.FLOW_NF, osup.nplanes, osup.s.hpad, osup.s.vpad, bits_of_the_hole or bits, **fkw)
    kinds, stats, outs = set(), {}, []
    for n in range(sr.FLOW_NF):
        outs.append(ref.frame(n, frames, lambda k: fin[k], blobs[n], 0, stats))
        kinds.add(ref.last_kind)
    return ",".join(sorted(kinds | {k for k, v in stats.items() if v > 0})), stats, outs


def _cpu_blur(oracle, case):
    import flowmc_ref
    gen, fmt, w, h, bits, skw, akw, fkw, recipe, _ = case
    frames, osup, fin, vecs = _flow_pipeline(oracle, gen, fmt, w, h, bits, skw, akw, (1, 0))
    bbw, bfw = _edited("flowblur", recipe, fkw, vecs)
    ref = flowmc_ref.FlowBlur(vecs[0][0], vecs[1][0], sr.FLOW_NF, osup.nplanes, osup.s.hpad, osup.s.vpad, bits, **fkw)
    kinds, stats, probe = set(), {}, {}
    for n in range(sr.FLOW_NF):
        ref.frame(n, frames, lambda k: fin[k], bbw, bfw, stats, probe)
        kinds.add(ref.last_kind)
    return ",".join(sorted(kinds | {k for k, v in stats.items() if v > 0})), stats, probe


def _cases(cases, cond=lambda c: True):
    return [pytest.param(c, id=sr.flow_case_id(c)) for c in cases if cond(c)]


def test_flow_range_lists_are_well_formed():
    """new recipe seeds start at 2000 and lie 20 apart (a case edits 2 * FLOW_NF blobs with seed + index); the geometry is the issue's"""
    import vector_fields as vf
    cases = sr.FLOWINTER_RANGE_CASES + sr.FLOW_RANGE_CASES + sr.BLUR_RANGE_CASES
    seeds = sorted(c[8].seed for c in cases if c[8] is not None)
    assert seeds[0] >= 2000 and all(b - a >= 20 for a, b in zip(seeds, seeds[1:])) and 2 * sr.FLOW_NF <= 20
    old = [k[-1].seed for lst in (vf.DEGRAIN_CASES, vf.COMPENSATE_CASES, vf.BLOCKFPS_CASES, vf.RECALC_CASES, vf.FLOWINTER_CASES, vf.FLOW_CASES, vf.BLUR_CASES,
                                  [vf.FULL_DEGRAIN, vf.FULL_FLOWFPS]) for k in lst]
    assert max(old) + 20 <= seeds[0]
    for c in cases:
        assert c[4] in (10, 12, 14, 16) and c[5] == {} and c[6]["blksize"] == 8 and c[6]["overlap"] == 4 and (c[8] is None or isinstance(c[8], vf.Recipe))
        assert c[8] is None or "thscd1" not in c[7], "the crafted fields are usable at the default thresholds"
    assert len(set(sr.flow_case_id(c) for c in cases)) == len(cases)


def test_flow_range_cases_cover_every_formula_below_16_bits():
    """together, at 10, 12 and 14 bits alone, the cases reach each formula and fallback of FlowInter / FlowFPS, Flow's fetch and shift with
    colliding sources and holes, and FlowBlur's taps with truncating divisions (tests/test_gpu_flow.py and tests/test_gpu_flowmc.py hold the
    same sets over their 8 and 16-bit cases)"""
    seen = lambda cases: set(k for c in cases if c[4] in (10, 12, 14) for k in c[-1].split(","))
    assert seen(sr.FLOWINTER_RANGE_CASES) == {"simple", "simple128", "regular", "regular128", "extra", "extra128", "blend", "left", "copy"}
    assert seen(sr.FLOW_RANGE_CASES) == {"copy", "fetch", "shift", "collide", "hole"}
    assert seen(sr.BLUR_RANGE_CASES) == {"copy", "blur", "taps", "trunc", "notaps"}   # (notaps: the prec=3 case only)
    for bits in (10, 12, 14):   # every depth on its own reaches the hole value and a formula of each family
        assert {"hole", "fetch"} <= set(k for c in sr.FLOW_RANGE_CASES if c[4] == bits for k in c[-1].split(","))
        assert {"simple", "regular", "extra"} <= set(k for c in sr.FLOWINTER_RANGE_CASES if c[4] == bits for k in c[-1].split(","))


@pytest.mark.parametrize("case", _cases(sr.FLOWINTER_RANGE_CASES, lambda c: c[0] != "step" or c[8] is not None))
def test_flowinter_range_cases_reach_their_kinds(oracle, case):
    """the pinned kinds, from the restatement; searched vectors (T): a twentieth at least of the fetched dF and of the fetched dB are 0 and
    a twentieth are pm; crafted occlusion fields: both masks reach 255, and on the checker most fetched samples are 0 or pm"""
    gen, bits, recipe = case[0], case[4], case[8]
    pm = (1 << bits) - 1
    probe = {}
    kinds, _, _ = _cpu_flowinter(oracle, case, probe)
    assert kinds == case[-1]
    dF, dB = (np.concatenate([a.ravel() for a in probe[k]]) for k in ("dF", "dB"))
    MF, MB = (np.concatenate([a.ravel() for a in probe[k]]) for k in ("MF", "MB"))
    if recipe is None:
        for d in (dF, dB):
            assert (d == 0).mean() >= 0.05 and (d == pm).mean() >= 0.05, ((d == 0).mean(), (d == pm).mean())
        if case[7].get("ml") == 20.0:
            assert MF.max() == 255 and MB.max() == 255, "ml 20 is there to let the search's own vectors saturate the masks"
    else:
        assert MF.max() == 255 and MB.max() == 255 and (MF == 255).mean() > 0.02 and (MB == 255).mean() > 0.02
        assert ((MF > 0) & (MF < 255)).any() and (MF == 0).any()
        if gen == "checker":
            assert ((dF == 0) | (dF == pm)).mean() > 0.5 and ((dB == 0) | (dB == pm)).mean() > 0.5   # (the sub-pel planes hold values between)
        for d in (dF, dB):   # a mask of 255 on a sample of 0 and on a sample of pm, both ways round
            for m in (MF, MB):
                assert ((m == 255) & (d == 0)).any() and ((m == 255) & (d >= pm - (pm + 1) // 32)).any()


def test_searched_vectors_on_rails_need_the_thresholds_raised(oracle):
    """the trap: at the default thscd1 / thscd2 the search's vectors on rails are scene changes, every job is Blend (or FlowFPS's copy) and a
    GPU case would compare the fallback alone"""
    for case in (sr.FLOWINTER_RANGE_CASES[0], [c for c in sr.FLOWINTER_RANGE_CASES if c[0] == "rails" and c[4] == 16 and "time" in c[7]][0]):
        assert case[8] is None and case[7]["thscd1"] == 16320 and case[7]["thscd2"] == 255
        kinds, _, _ = _cpu_flowinter(oracle, case, thscd1=400, thscd2=130)
        assert set(kinds.split(",")) <= {"blend", "copy"} and "blend" in kinds, kinds
        assert set(case[-1].split(",")) & {"extra", "extra128", "simple", "regular"}


OCC16 = [c for c in sr.FLOWINTER_RANGE_CASES if c[4] == 16 and c[8] is not None and c[7] == dict(fps=1, num=48, mask=1)]
BOUND = 65535 * 255 * 255 + 255   # MF * (dB * (255 - MB) + MB * dF0) + 255 at MF = 255 and samples of 65535: 0.992 * 2^32


@pytest.mark.parametrize("case", _cases(OCC16))
def test_regular_product_reaches_its_bound_at_16_bits(oracle, case):
    """MaskFun.cpp:374-414 forms MF * (dB * (255 - MB) + MB * dF0) + 255 in 64 bits, the kernel in 32 unsigned: a tenth of the products
    at least lie at or above 2^31 (where a signed 32-bit product would wrap) and the largest IS the bound, 4 261 413 630 < 2^32"""
    probe = {}
    kinds, _, _ = _cpu_flowinter(oracle, case, probe)
    assert kinds == "copy,regular128"
    inner = np.concatenate([a.ravel() for a in probe["inner"]])
    assert inner.dtype == np.int64 and inner.min() >= 255
    assert (inner >= 1 << 31).mean() >= 0.1, (inner >= 1 << 31).mean()
    assert int(inner.max()) == BOUND == 4261413630 and BOUND < 1 << 32


def test_regular_product_control_at_14_bits(oracle):
    """the same field on the same clip at 14 bits: the largest product is 16383 * 255 * 255 + 255, below 2^31 -- only 16 bits reach the bound"""
    assert len(OCC16) == 3 and sorted(c[0] for c in OCC16) == ["checker", "rails", "step"]
    case = [c for c in OCC16 if c[0] == "rails"][0]
    probe = {}
    _cpu_flowinter(oracle, case[:4] + (14,) + case[5:], probe)
    assert max(int(a.max()) for a in probe["inner"]) == 16383 * 255 * 255 + 255 < 1 << 31


@pytest.mark.parametrize("case", _cases(sr.FLOWINTER_RANGE_CASES, lambda c: c[0] == "step" and c[8] is None))
def test_the_cut_is_blended_or_left(oracle, case):
    """between a frame near 0 and a frame near pm every job falls back: Blend (FlowFPS: and the copies), or the left frame with blend=0"""
    pm = (1 << case[4]) - 1
    kinds, frames, outs = _cpu_flowinter(oracle, case)
    assert kinds == case[-1] and set(kinds.split(",")) - {"copy"} == ({"blend"} if case[7].get("blend", 1) else {"left"})
    for n, fr in enumerate(frames):
        for p in fr:
            assert (p.mean() > 15 * pm / 16) if n & 1 else (p.mean() < pm / 16), (n, p.mean())
    if case[7].get("blend", 1):   # a blend of the two levels: an output frame far from both
        assert any(pm / 8 < o[0].mean() < 7 * pm / 8 for o in outs)


@pytest.mark.parametrize("case", _cases(sr.FLOW_RANGE_CASES))
def test_flow_range_cases_reach_their_kinds(oracle, case):
    """the pinned kinds; shift at time 100 on the crafted fields below 16 bits: a tenth at least of the destinations are holes and a tenth
    are not, sources collide, and the same run with the hole value of 16 bits gives other planes (so a kernel that painted 65535, or took
    the depth from the two-byte container, fails the GPU case); fetch: the output holds 0 and pm"""
    bits, fkw, recipe = case[4], case[7], case[8]
    pm = (1 << bits) - 1
    kinds, stats, outs = _cpu_flow(oracle, case)
    assert kinds == case[-1]
    if fkw.get("mode"):
        total = (sr.FLOW_NF - 1) * sum(p.size for p in outs[0])   # all frames but one have a reference (the last with isb=1, the first with isb=0)
        assert stats["hole"] > 0 and stats["collide"] > 0
        if recipe is not None and fkw["time"] == 100.0:
            assert 0.1 * total <= stats["hole"] <= 0.9 * total, (stats, total)
        if bits < 16:
            _, _, wide = _cpu_flow(oracle, case, bits_of_the_hole=16)
            assert any(not np.array_equal(a, b) for o, v in zip(outs, wide) for a, b in zip(o, v))
            assert all(int(p.max()) <= pm for o in outs for p in o) and any(int(p.max()) == 65535 for v in wide for p in v)
    else:
        assert min(int(p.min()) for o in outs for p in o) == 0 and max(int(p.max()) for o in outs for p in o) == pm


@pytest.mark.parametrize("case", _cases(sr.BLUR_RANGE_CASES))
def test_blur_range_cases_reach_their_kinds(oracle, case):
    """the pinned kinds, taps and truncating divisions; at 16 bits the largest sum of a sample and its taps is above 2^24 (hundreds of taps
    of 65535: no float32 accumulator holds it exactly)"""
    kinds, stats, probe = _cpu_blur(oracle, case)
    assert kinds == case[-1] and stats["taps"] > 0 and stats["trunc"] > 0
    if case[4] == 16 and case[7].get("prec", 1) == 1:
        assert probe["max_sum"] > 1 << 24 and probe["max_count"] > 256, probe
    assert probe["max_sum"] <= probe["max_count"] * ((1 << case[4]) - 1) < 1 << 31


# ------------------------------------------------------------------------------------------- the oracle under sanitizers
def test_oracle_has_no_undefined_behaviour_at_the_ends_of_the_range(tmp_path):
    """tests/sample_range_oracle_main.c: step and checker clips at 16 and 10 bits through Super -> Analyse (blksize 32 and 16, pnew 50 and
    256) -> Degrain1 -> Compensate of the oracle's C functions, as a stand-alone program built with AddressSanitizer and
    UndefinedBehaviourSanitizer (any report aborts).  The parity target has no overflow of its own at these inputs."""
    exe = str(tmp_path / "sample_range_oracle_main")
    odir = os.path.join(ROOT, "oracle")
    srcs = [os.path.join(odir, f) for f in ("mvo_super.c", "mvo_analyse.c", "mvo_degrain.c", "mvo_blockfps.c")]
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-ffp-contract=off", "-fno-strict-aliasing", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + odir, os.path.join(ROOT, "tests", "sample_range_oracle_main.c")] + srcs + ["-o", exe, "-lm"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-3000:]
    # same arithmetic as the Python generators: the program prints a checksum of each clip it made
    sums = dict(line.split()[1:3] for line in r.stdout.splitlines() if line.startswith("clip "))
    for bits in (16, 10):
        pm = (1 << bits) - 1
        st = sr.step(256, 160, bits, 3, 0, pm - pm // 4)
        ck = sr.checker(256, 160, bits, 3)
        for name, fr in (("step%d" % bits, st), ("checker%d" % bits, ck)):
            want = sum(int(p.astype(np.int64).sum()) * (7 * f + p_i + 1) for f, planes in enumerate(fr) for p_i, p in enumerate(planes))
            assert int(sums[name]) == want, name
