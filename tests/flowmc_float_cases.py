"""What the float Flow / FlowBlur tests share (test infrastructure): the cases of tests/test_gpu_flowmc_float.py, how a case's clips, vectors
and expected frames are made, and the conditions every case has to meet (tests/test_flowmc_float_cases.py enforces them on the CPU).

A case runs every frame of a five-frame clip as one batch of jobs.  The integer clip is the (1, 0)-per-frame moving texture of
tests/degrain_n_cases.py; the float clip is degrain_float_cases.float_clip of it, so the search -- the oracle's on the CPU, the library's on the
GPU, the same blobs -- is the integer clip's.  Crafted cases rewrite level 0 of every blob with the recipes of tests/vector_fields.py, one
after the other, before the filter sees them.

Sizes: 96x64 (tests/multi_cases.py; segments of 4 float samples in every plane), 70x54 (segments of 2 in luma, of 1 in the 35-sample chroma
rows), 36x36 Gray without padding, and 35x30 4:4:4 (an odd width: one-sample segments in every plane).  Nothing larger is needed: edge-cut cells,
one-sample segments and occlusions that span workgroups all occur at these.

The conditions:
  blur      every FlowBlur case with blur > 0 has at least TAPS_SHARE of its luma samples with mF + mB >= 1 and at least one with mF + mB >= 8
  shift     every shift case on a crafted field has at least one hole and at least one destination that two sources claim; the searched
            shift cases have both between them
  copies    every batch has at least one job that copies (a clip end, a scene change, an invalid blob) beside at least one that does not
"""
import collections

import numpy as np

import degrain_float_cases as fc
import degrain_n_cases as dc
import flowmc_float_ref as ff
import super_float_ref as sf
import vector_fields
from vector_fields import Recipe as R

NF = 5
TAPS_SHARE = 0.1
SUB = {"420": (1, 1), "422": (1, 0), "444": (0, 0), "gray": (1, 1)}
P0 = dict(hpad=0, vpad=0)
B168, B84, B42, B160 = dict(blksize=16, overlap=8), dict(blksize=8, overlap=4), dict(blksize=4, overlap=2), dict(blksize=16, overlap=0)

Case = collections.namedtuple("Case", "kind name fmt w h bits skw akw fkw recipes")


def _f(name, fmt, w, h, bits, skw, akw, fkw, *recipes):
    return Case("flow", name, fmt, w, h, bits, skw, akw, fkw, recipes)


def _b(name, fmt, w, h, bits, skw, akw, fkw, *recipes):
    return Case("blur", name, fmt, w, h, bits, skw, akw, fkw, recipes)


BW, FW = dict(isb=1), dict(isb=0)
FETCH100, SHIFT100 = dict(time=100.0), dict(time=100.0, mode=1)
FLOW_SEARCHED = [
    _f("420-8bit-pel2-8/4-bw", "420", 96, 64, 8, dict(pel=2), dict(B84, **BW), FETCH100),
    _f("420-16bit-pel2-8/4-fw-shift", "420", 96, 64, 16, dict(pel=2), dict(B84, **FW), SHIFT100),
    _f("444-8bit-pel4-16/8-bw-d2-time50", "444", 96, 64, 8, dict(pel=4), dict(B168, isb=1, delta=2), dict(time=50.0)),
    _f("444-16bit-pel4-16/8-fw-d2-time50-shift", "444", 96, 64, 16, dict(pel=4), dict(B168, isb=0, delta=2), dict(time=50.0, mode=1)),
    _f("gray-16bit-pel1-16/0-bw-shift", "gray", 96, 64, 16, dict(pel=1), dict(B160, **BW), SHIFT100),
    _f("gray-8bit-pel1-16/0-fw", "gray", 96, 64, 8, dict(pel=1), dict(B160, **FW), FETCH100),
    _f("70x54-8bit-pel2-4/2-fw", "420", 70, 54, 8, dict(pel=2), dict(B42, **FW), FETCH100),
    _f("70x54-16bit-pel2-4/2-bw-shift", "420", 70, 54, 16, dict(pel=2), dict(B42, **BW), SHIFT100),
    _f("420-8bit-pel2-8/4-bw-time0", "420", 96, 64, 8, dict(pel=2), dict(B84, **BW), dict(time=0.0)),
    _f("420-8bit-pel2-8/4-fw-time0-shift", "420", 96, 64, 8, dict(pel=2), dict(B84, **FW), dict(time=0.0, mode=1)),
    # vectors with an absolute reference (frame 2): no clip end copies, so frame 3's blob is made invalid
    _f("420-8bit-pel2-8/4-absolute", "420", 96, 64, 8, dict(pel=2), dict(B84, isb=0, delta=-2), FETCH100, R("invalid", 7, only=(3,))),
    _f("36x36-gray-pad0-8/4-bw", "gray", 36, 36, 8, dict(pel=2, **P0), dict(B84, **BW), FETCH100),
    _f("36x36-gray-pad0-8/4-fw-d2-shift", "gray", 36, 36, 16, dict(pel=2, **P0), dict(B84, isb=0, delta=2), SHIFT100),
    _f("35x30-444-pel1-8/4-bw", "444", 35, 30, 8, dict(pel=1), dict(B84, **BW), FETCH100),
    _f("35x30-444-pel2-8/4-fw-shift", "444", 35, 30, 16, dict(pel=2), dict(B84, **FW), SHIFT100),
]
FLOW_CRAFTED = [
    _f("70x54-limits", "420", 70, 54, 8, dict(pel=2), dict(B84, **BW), FETCH100, R("limits", 2001)),
    _f("70x54-limits-shift", "420", 70, 54, 16, dict(pel=2), dict(B84, **FW), SHIFT100, R("limits", 2011)),
    _f("96x64-pel4-16/8-limits-time50-shift", "420", 96, 64, 16, dict(pel=4), dict(B168, **BW), dict(time=50.0, mode=1), R("limits", 2021)),
    _f("36x36-gray-pad0-limits-shift", "gray", 36, 36, 8, dict(pel=2, **P0), dict(B84, **BW), SHIFT100, R("limits", 2031)),
    _f("35x30-444-limits-shift", "444", 35, 30, 8, dict(pel=1), dict(B84, **FW), SHIFT100, R("limits", 2041)),
    _f("70x54-invalid", "420", 70, 54, 8, dict(pel=2), dict(B84, **BW), FETCH100, R("limits", 2051), R("invalid", 2052, only=(1,))),
    _f("70x54-invalid-shift", "420", 70, 54, 8, dict(pel=2), dict(B84, **BW), SHIFT100, R("limits", 2061), R("invalid", 2062, only=(2,))),
    # every blob exactly on thscd2 (usable), frame 1's one block over it (a scene change)
    _f("70x54-scene", "420", 70, 54, 16, dict(pel=2), dict(B84, **FW), FETCH100, R("limits", 2071), R("scene_count", 2072, over=1, only=(1,))),
    _f("70x54-scene-shift", "420", 70, 54, 8, dict(pel=2), dict(B84, **FW), SHIFT100, R("limits", 2081), R("scene_count", 2082, over=1, only=(2,))),
]
BLUR_SEARCHED = [
    _b("420-8bit-pel4-8/4-blur200", "420", 96, 64, 8, dict(pel=4), B84, dict(blur=200.0)),
    _b("420-16bit-pel2-16/8-d2-blur200", "420", 96, 64, 16, dict(pel=2), dict(B168, delta=2), dict(blur=200.0)),
    _b("444-8bit-pel4-16/0-blur200", "444", 96, 64, 8, dict(pel=4), B160, dict(blur=200.0)),
    _b("420-8bit-pel2-8/4-blur0", "420", 96, 64, 8, dict(pel=2), B84, dict(blur=0.0)),
    _b("gray-16bit-pel4-4/2-blur200", "gray", 96, 64, 16, dict(pel=4), B42, dict(blur=200.0)),
]
BLUR_CRAFTED = [
    _b("70x54-limits-blur50", "420", 70, 54, 8, dict(pel=2), B84, dict(blur=50.0), R("limits", 2101)),
    _b("70x54-4/2-limits-blur200-prec4", "420", 70, 54, 16, dict(pel=2), B42, dict(blur=200.0, prec=4), R("limits", 2111)),
    _b("36x36-gray-pad0-limits-blur50", "gray", 36, 36, 8, dict(pel=1, **P0), B160, dict(blur=50.0), R("limits", 2121)),
    _b("35x30-444-limits-blur200", "444", 35, 30, 16, dict(pel=1), B84, dict(blur=200.0), R("limits", 2131)),
    _b("96x64-pel4-limits-blur50-prec4", "420", 96, 64, 8, dict(pel=4), B168, dict(blur=50.0, prec=4), R("limits", 2141)),
    _b("70x54-invalid", "420", 70, 54, 8, dict(pel=2), B84, dict(blur=50.0), R("limits", 2151), R("invalid", 2152, only=(1,))),  # mvbw at 1: frame 2 copies
    _b("70x54-scene", "420", 70, 54, 16, dict(pel=2), B84, dict(blur=200.0), R("limits", 2161), R("scene_count", 2162, over=1, only=(NF + 2,))),  # mvfw at 2: frame 1
]
FLOW_CASES, BLUR_CASES = FLOW_SEARCHED + FLOW_CRAFTED, BLUR_SEARCHED + BLUR_CRAFTED
CASES = FLOW_CASES + BLUR_CASES


def case_id(c):
    return "%s-%s" % (c.kind, c.name)


def super_kwargs(c):
    return dict(dc.FORMATS[c.fmt], **c.skw)


def clips(c):
    """(the integer clip, the float clip whose quantised copy it is)"""
    q = dc.clip(c.w, c.h, c.bits, NF, c.fmt)
    return q, fc.float_clip(q, c.bits, seed=9)


def fields(c):
    """the vector clips a case searches: [(isb, delta)] -- Flow one, FlowBlur mvbw and mvfw"""
    if c.kind == "flow":
        return [(c.akw["isb"], c.akw.get("delta", 1))]
    return [(1, c.akw.get("delta", 1)), (0, c.akw.get("delta", 1))]


def analyse_kwargs(c):
    return {k: v for k, v in c.akw.items() if k not in ("isb", "delta")}


def reference(isb, delta, n):
    """the frame that frame n is searched against, None outside the clip (MVAnalyse.c; an absolute reference for delta <= 0)"""
    r = (n + delta if isb else n - delta) if delta > 0 else -delta
    return r if 0 <= r < NF else None


def search_oracle(oracle, c, q):
    """-> per vector clip (analysis data, [blob of every frame]) from the oracle's search on the integer clip"""
    osup = oracle.Super(c.w, c.h, c.bits, **super_kwargs(c))
    osf = [osup.frame(f) for f in q]
    out = []
    for isb, delta in fields(c):
        an = oracle.Analyse(osup, num_frames=NF, isb=isb, delta=delta, **analyse_kwargs(c))
        blobs = []
        for n in range(NF):
            r = reference(isb, delta, n)
            blobs.append(an.frame(osf[n], osf[r] if r is not None else None))
        out.append((an.ad, blobs))
    return out


def edited(c, searched):
    """the recipes of a case applied to every blob, one after the other; blob i of vector clip k has the index k * NF + i"""
    out = []
    for k, (ad, blobs) in enumerate(searched):
        new = []
        for i, b in enumerate(blobs):
            b = np.array(b, dtype=np.uint8, copy=True)
            for r in c.recipes:
                b = vector_fields.case_editor("flow" if c.kind == "flow" else "flowblur", r, c.fkw)(b, ad, k * NF + i)
            new.append(b)
        out.append((ad, new))
    return out


class Expected:
    """the restatement's frames of a case: frames[n] (float32 planes), kinds[n] ("copy" / "fetch" / "shift" / "blur") and the counters"""

    def __init__(self, c, floats, vectors, info, supers=None):
        """floats: the float clip; vectors: edited(); info: the float super clip's mvx_super_info (padding, pel, sharp); supers: callable
        k -> float super frame k on the host (default: the Super restatement's)"""
        gray = c.fmt == "gray"
        skw = dict(sub=SUB[c.fmt], gray=gray, hpad=info.hpad, vpad=info.vpad, pel=info.pel, sharp=info.sharp)
        cache = {}

        def sup(k):
            if k not in cache:
                cache[k] = supers(k) if supers else sf.frame(floats[k], **skw)[0]
            return cache[k]
        nplanes = 1 if gray else 3
        self.stats, self.frames, self.kinds = {}, [], []
        fkw = dict(c.fkw)
        if c.kind == "flow":
            ad, blobs = vectors[0]
            ref = ff.Flow(ad, NF, nplanes, info.hpad, info.vpad, **fkw)
            for n in range(NF):
                self.frames.append(ref.frame(n, floats, sup, blobs[n], 0, self.stats))
                self.kinds.append(ref.last_kind)
        else:
            (abw, bbw), (afw, bfw) = vectors
            ref = ff.FlowBlur(abw, afw, NF, nplanes, info.hpad, info.vpad, **fkw)
            for n in range(NF):
                self.frames.append(ref.frame(n, floats, sup, bbw, bfw, self.stats))
                self.kinds.append(ref.last_kind)


def check_conditions(c, e):
    """the conditions of the module's docstring that one case can be held to"""
    assert "copy" in e.kinds and len(set(e.kinds)) == 2, "%s: the batch needs a job that copies beside the usable ones: %s" % (c.name, e.kinds)
    s = e.stats
    if c.kind == "blur" and c.fkw.get("blur", 50.0) > 0:
        assert s["taps1"] >= TAPS_SHARE * s["luma"], "%s: %d of %d luma samples have taps" % (c.name, s["taps1"], s["luma"])
        assert s["taps8"] >= 1, "%s: no sample with mF + mB >= 8 (the most: %d)" % (c.name, s["max_taps"])
    if c.kind == "flow" and c.fkw.get("mode") and c.recipes and c.recipes[0].name == "limits":
        assert s.get("hole", 0) >= 1 and s.get("collide", 0) >= 1, "%s: holes %d, claimed twice %d" % (c.name, s.get("hole", 0), s.get("collide", 0))
