"""What the float FlowInter / FlowFPS tests share (test infrastructure): the cases of tests/test_gpu_flow_float.py, how a case's clips, vectors
and expected frames are made, and the conditions the cases have to meet (tests/test_flow_float_cases.py enforces them on the CPU).

A case runs every output frame of a five-frame clip as one batch of jobs: FlowInter five, FlowFPS eleven (24 -> 60) or nine (24 -> 48, every
other frame at time256 128).  The clips are those of tests/flowmc_float_cases.py: the integer clip is the moving texture, the float clip is
float_clip of it, and the vectors are the oracle's search of the integer clip ON THE HOST in every test, the GPU tests included (mvbw and mvfw
of one delta).  Crafted cases rewrite level 0 of every blob with the recipes of tests/vector_fields.py, one after the other.

Sizes: 96x64 (segments of 4 float samples in every plane), 70x54 (segments of 2 in luma, of 1 in the 35-sample chroma rows; a padded small-field
column and row), 36x36 Gray without padding (fetches on the frame's edge) and 35x30 4:4:4 (an odd width).

The conditions:
  every case     the batch has a job that copies or blends (FlowFPS at time256 0, a clip end, a scene change, an invalid blob) beside an
                 interpolated one
  all together   Regular and Extra occur in FlowInter; Simple, Regular and Extra in FlowFPS (FlowInter has no Simple path: MVFlowInter.c calls
                 FlowInter and FlowInterExtra only, and fl_state follows it); some job has time256 128; some FlowFPS mask 2 job falls through
                 to Simple; some job of a blend 0 filter copies the left frame
  occlusion      every case on a crafted `occlusion` field has at least TAPS_SHARE of the luma samples of its interpolated jobs under
                 mF + mB >= 1 and at least one sample with dF != dB under a non-zero mask; if it has Extra jobs, at least one sample where
                 the clamp changes the extra fetch under its mask and one where it does not
"""
import collections

import numpy as np

import flow_float_ref as fl
import flowmc_float_cases as mc
import super_float_ref as sf
import vector_fields
from vector_fields import Recipe as R

NF = mc.NF
TAPS_SHARE = mc.TAPS_SHARE
SUB, P0 = mc.SUB, mc.P0
B168, B84, B42, B160 = mc.B168, mc.B84, mc.B42, mc.B160
FALLBACKS = ("copy", "blend", "left")

Case = collections.namedtuple("Case", "kind name fmt w h bits skw akw fkw recipes")


def _i(name, fmt, w, h, bits, skw, akw, fkw, *recipes):
    return Case("inter", name, fmt, w, h, bits, skw, akw, fkw, recipes)


def _p(name, fmt, w, h, bits, skw, akw, fkw, *recipes):
    return Case("fps", name, fmt, w, h, bits, skw, akw, dict(fkw, fps=(24, 1), den=1), recipes)


D2 = dict(delta=2)
INTER_SEARCHED = [
    _i("420-8bit-pel2-8/4-time50", "420", 96, 64, 8, dict(pel=2), B84, dict(time=50.0)),
    _i("444-16bit-pel4-16/8-d2-time37.5-blend0", "444", 96, 64, 16, dict(pel=4), dict(B168, **D2), dict(time=37.5, blend=0)),
    _i("gray-16bit-pel1-16/0-time100", "gray", 96, 64, 16, dict(pel=1), B160, dict(time=100.0)),
    _i("70x54-8bit-pel2-4/2-time0", "420", 70, 54, 8, dict(pel=2), B42, dict(time=0.0)),
    _i("36x36-gray-pad0-8/4-time37.5", "gray", 36, 36, 8, dict(pel=2, **P0), B84, dict(time=37.5)),
    _i("35x30-444-pel1-8/4-time50", "444", 35, 30, 16, dict(pel=1), B84, dict(time=50.0)),
]
INTER_CRAFTED = [
    _i("96x64-occlusion-time50", "420", 96, 64, 8, dict(pel=2), B84, dict(time=50.0), R("occlusion", 3001)),
    _i("70x54-4/2-occlusion-time37.5-ml200", "420", 70, 54, 16, dict(pel=2), B42, dict(time=37.5, ml=200.0), R("occlusion", 3011)),
    _i("36x36-gray-pad0-4/2-occlusion-time50-ml250", "gray", 36, 36, 8, dict(pel=1, **P0), B42, dict(time=50.0, ml=250.0), R("occlusion", 3021)),
    _i("70x54-limits-time50", "420", 70, 54, 8, dict(pel=2), B84, dict(time=50.0), R("limits", 3031)),
    _i("35x30-444-limits-pel2-time100", "444", 35, 30, 8, dict(pel=2), B84, dict(time=100.0), R("limits", 3041)),
    # mvfw at 2 invalid: frame 1 blends, frame 2 loses its extra vectors (Regular)
    _i("70x54-invalid", "420", 70, 54, 8, dict(pel=2), B84, dict(time=37.5), R("limits", 3051), R("invalid", 3052, only=(NF + 2,))),
    # every blob exactly on thscd2 (usable), mvbw at 1 one block over it (a scene change): frame 1 copies the left frame
    _i("70x54-scene-blend0", "420", 70, 54, 16, dict(pel=2), B84, dict(time=50.0, blend=0), R("limits", 3061), R("scene_count", 3062, over=1, only=(1,))),
]
FPS_SEARCHED = [
    _p("420-8bit-pel2-8/4-60-mask2", "420", 96, 64, 8, dict(pel=2), B84, dict(num=60, mask=2)),
    _p("420-16bit-pel2-8/4-48-mask1", "420", 96, 64, 16, dict(pel=2), B84, dict(num=48, mask=1)),
    _p("444-8bit-pel4-16/8-60-mask0", "444", 96, 64, 8, dict(pel=4), B168, dict(num=60, mask=0)),
    _p("gray-16bit-pel1-16/0-d2-48-mask2-blend0", "gray", 96, 64, 16, dict(pel=1), dict(B160, **D2), dict(num=48, mask=2, blend=0)),
    _p("70x54-16bit-pel2-4/2-60-mask2", "420", 70, 54, 16, dict(pel=2), B42, dict(num=60, mask=2)),
    _p("70x54-8bit-pel2-8/4-d2-60-mask1", "420", 70, 54, 8, dict(pel=2), dict(B84, **D2), dict(num=60, mask=1)),
    _p("36x36-gray-pad0-8/4-60-mask0", "gray", 36, 36, 16, dict(pel=2, **P0), B84, dict(num=60, mask=0)),
    _p("35x30-444-pel2-8/4-48-mask2", "444", 35, 30, 8, dict(pel=2), B84, dict(num=48, mask=2)),
]
FPS_CRAFTED = [
    _p("96x64-occlusion-48-mask2", "420", 96, 64, 8, dict(pel=2), B84, dict(num=48, mask=2), R("occlusion", 3101)),
    _p("70x54-4/2-occlusion-48-mask1-ml80", "420", 70, 54, 16, dict(pel=2), B42, dict(num=48, mask=1, ml=80.0), R("occlusion", 3111)),
    _p("35x30-444-4/2-occlusion-48-mask0", "444", 35, 30, 8, dict(pel=1), B42, dict(num=48, mask=0), R("occlusion", 3121)),
    _p("70x54-limits-60-mask2", "420", 70, 54, 8, dict(pel=2), B84, dict(num=60, mask=2), R("limits", 3131)),
    # mvfw at 1 invalid: the jobs between frames 0 and 1 blend, those between 1 and 2 lose their extra vectors (mask 2 falls through to Simple)
    _p("70x54-invalid-60-mask2", "420", 70, 54, 16, dict(pel=2), B84, dict(num=60, mask=2), R("limits", 3141), R("invalid", 3142, only=(NF + 1,))),
    _p("70x54-scene-60-mask1-blend0", "420", 70, 54, 8, dict(pel=2), B84, dict(num=60, mask=1, blend=0), R("limits", 3151),
       R("scene_count", 3152, over=1, only=(2,))),
]
INTER_CASES, FPS_CASES = INTER_SEARCHED + INTER_CRAFTED, FPS_SEARCHED + FPS_CRAFTED
CASES = INTER_CASES + FPS_CASES


def case_id(c):
    return "%s-%s" % (c.kind, c.name)


super_kwargs, clips = mc.super_kwargs, mc.clips


def fields(c):
    """the vector clips a case searches: mvbw and mvfw"""
    return [(1, c.akw.get("delta", 1)), (0, c.akw.get("delta", 1))]


def search_oracle(oracle, c, q):
    """-> per vector clip (analysis data, [blob of every frame]) from the oracle's search on the integer clip, as flowmc_float_cases does"""
    osup = oracle.Super(c.w, c.h, c.bits, **super_kwargs(c))
    osf = [osup.frame(f) for f in q]
    out = []
    for isb, delta in fields(c):
        an = oracle.Analyse(osup, num_frames=NF, isb=isb, delta=delta, **mc.analyse_kwargs(c))
        refs = [mc.reference(isb, delta, n) for n in range(NF)]
        out.append((an.ad, [an.frame(osf[n], osf[r] if r is not None else None) for n, r in enumerate(refs)]))
    return out


def edited(c, searched):
    """the recipes of a case applied to every blob, one after the other; blob i of vector clip k has the index k * NF + i"""
    out = []
    for k, (ad, blobs) in enumerate(searched):
        new = []
        for i, b in enumerate(blobs):
            b = np.array(b, dtype=np.uint8, copy=True)
            for r in c.recipes:
                b = vector_fields.case_editor("flowinter", r, c.fkw)(b, ad, k * NF + i)
            new.append(b)
        out.append((ad, new))
    return out


def package_kwargs(c):
    """the keyword arguments of mv.FlowInter / mv.FlowFPS for a case"""
    kw = {k: v for k, v in c.fkw.items() if k != "fps"}
    if c.kind == "fps":
        kw.update(fps_num=c.fkw["fps"][0], fps_den=c.fkw["fps"][1])
    return kw


class Expected:
    """the restatement's frames of a case: frames[n] (float32 planes), kinds[n] (flow_ref.Flow.last_kind) and the counters of the conditions"""

    def __init__(self, c, floats, vectors, info, supers=None):
        """floats: the float clip; vectors: edited(); info: the float super clip's mvx_super_info; supers: callable k -> float super frame k on
        the host (default: the Super restatement's)"""
        gray = c.fmt == "gray"
        skw = dict(sub=SUB[c.fmt], gray=gray, hpad=info.hpad, vpad=info.vpad, pel=info.pel, sharp=info.sharp)
        cache = {}

        def sup(k):
            if k not in cache:
                cache[k] = supers(k) if supers else sf.frame(floats[k], **skw)[0]
            return cache[k]
        nplanes = 1 if gray else 3
        (abw, bbw), (afw, bfw) = vectors
        self.ref = ref = fl.Flow(abw, afw, NF, nplanes, info.hpad, info.vpad, **c.fkw)
        self.num_frames = ref.num_frames
        self.frames, self.kinds, self.times, probe = [], [], [], {}
        for n in range(ref.num_frames):
            self.frames.append(ref.frame(n, floats, sup, bbw, bfw, probe))
            self.kinds.append(ref.last_kind)
            self.times.append(ref.map(n)[2])
        s = self.stats = dict(luma=0, masked=0, differ=0, bind=0, free=0)
        for i in range(len(probe.get("kind", []))):
            MF, MB, dF, dB = (probe[k][i] for k in ("MF", "MB", "dF", "dB"))
            if i % nplanes == 0:
                s["luma"] += MF.size
                s["masked"] += int(np.count_nonzero(MF + MB >= 1))
            s["differ"] += int(np.count_nonzero((dF != dB) & (MF + MB >= 1)))
        for dFF, dBB, i in zip(probe.get("dFF", []), probe.get("dBB", []), [i for i, k in enumerate(probe.get("kind", [])) if k == "extra"]):
            MF, MB, dF, dB = (probe[k][i] for k in ("MF", "MB", "dF", "dB"))
            lo, hi = np.minimum(dF, dB), np.maximum(dF, dB)
            cutBB, cutFF = (dBB < lo) | (dBB > hi), (dFF < lo) | (dFF > hi)
            s["bind"] += int(np.count_nonzero((cutBB & (MF > 0)) | (cutFF & (MB > 0))))
            s["free"] += int(np.count_nonzero((~cutBB & (MF > 0)) | (~cutFF & (MB > 0))))


def check_conditions(c, e):
    """the conditions of the module's docstring that one case can be held to"""
    kinds = set(e.kinds)
    assert kinds & set(FALLBACKS) and kinds - set(FALLBACKS), "%s: the batch needs a copying or blending job beside an interpolated one: %s" % (c.name, e.kinds)
    s = e.stats
    if c.recipes and c.recipes[0].name == "occlusion":
        assert s["masked"] >= TAPS_SHARE * s["luma"], "%s: %d of %d luma samples under a mask" % (c.name, s["masked"], s["luma"])
        assert s["differ"] >= 1, "%s: no sample with dF != dB under a mask" % c.name
        if any(k.startswith("extra") for k in e.kinds):
            assert s["bind"] >= 1 and s["free"] >= 1, "%s: the clamp binds at %d masked samples and not at %d" % (c.name, s["bind"], s["free"])
