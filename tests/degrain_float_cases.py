"""What the float Super / DegrainN tests share (test infrastructure): float clips with their quantised integer copies (the search runs on the
copy, the filter on the float clip), and the float restatement set up from a filter's resolved thresholds."""
import numpy as np

import degrain_float_ref
import degrain_n_cases as dc
import vector_fields

F = np.float32


def float_clip(int_frames, bits, seed=0, overshoot=False):
    """float32 frames whose quantised copy round(x * peak) (chroma: round((x + 0.5) * peak)) is int_frames: luma in [0, 1], chroma in [-0.5, 0.5],
    with noise below half a step of the integer clip so that the float samples are not the integers' images.  overshoot: luma stretched to
    -0.2 .. 1.3 (its quantised copy is then not int_frames: for Super only)"""
    rng = np.random.default_rng(seed)
    peak = float((1 << bits) - 1)
    out = []
    for fr in int_frames:
        planes = []
        for p, a in enumerate(fr):
            x = (a.astype(np.float64) + rng.uniform(-0.3, 0.3, a.shape)) / peak - (0.5 if p else 0.0)
            if overshoot and p == 0:
                x = (x - x.min()) / (x.max() - x.min()) * 1.5 - 0.2
            planes.append(x.astype(F))
        out.append(planes)
    if not overshoot:
        for fr, ifr in zip(out, int_frames):
            for p, a in enumerate(fr):
                assert np.array_equal(np.rint((a.astype(np.float64) + (0.5 if p else 0.0)) * peak).astype(ifr[p].dtype), ifr[p])
    return out


def integer_valued(int_frames):
    """the float clip whose samples are the integers themselves"""
    return [[p.astype(F) for p in fr] for fr in int_frames]


def restatement(oracle, radius, ad, th_luma, th_chroma, dkw, gray=False):
    """tests/degrain_float_ref.py for a filter whose scaled thresholds per distance are th_luma / th_chroma; dkw: the filter's other arguments"""
    _, s1, s2 = vector_fields.scaled_thresholds(ad, 400, dkw.get("thscd1", 400), dkw.get("thscd2", 130))
    return degrain_float_ref.DegrainFloat(oracle, radius, ad, th_luma, th_chroma, s1, s2, plane=dkw.get("plane", 4), limit=dkw.get("limit"),
                                          limitc=dkw.get("limitc"), gray=gray)


def oracle_job(oracle, frames, w, h, bits, radius, target, akw, skw=None, sub=(1, 1), gray=False):
    """the oracle's search around `target`: -> (oracle super, its frames, analysis data, frame numbers of the 2 * radius references or None, blobs)"""
    osup = oracle.Super(w, h, bits, subsampling=sub, gray=gray, **(skw or {}))
    sfr = [osup.frame(f) for f in frames]
    nrefs, blobs, ad = [], [], None
    for r, isb, d, nref in dc.neighbours(target, radius, len(frames)):
        an = oracle.Analyse(osup, isb=isb, delta=d, **akw)
        blobs.append(an.frame(sfr[target], sfr[nref] if nref is not None else None))
        nrefs.append(nref)
        ad = an.ad
    return osup, sfr, ad, nrefs, blobs
