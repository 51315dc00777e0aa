"""The cases of tests/test_vs_multi_shell.py and what the CPU oracle expects of them (test infrastructure).  tests/test_vs_multi_cases.py shows on the CPU
that the cases test what they claim.  Nothing here touches the library, the Python package or the shell."""
import degrain_n_cases as dc
import degrain_out16_ref as o16
import multi_cases as mc
import multi_oracle as mu
import mvoracle as mo
import pipeline as pl
import vector_fields

# the mini host's Gray clip has no subsampling: chroma ratios 1 / 1 in the analysis data
FORMATS = dict(dc.FORMATS, gray=dict(gray=True, subsampling=(0, 0)))
B84, B168 = dict(blksize=8, overlap=4), dict(blksize=16, overlap=8)

# ---- AnalyseN / MultiField: fmt, bits, super kwargs, analyse kwargs, radius (96x64, 2 * radius + 3 frames)
ANALYSE_CASES = [
    ("420", 8, dict(pel=2), B84, 1),
    ("420", 8, dict(pel=2), dict(B84, search=3), 3),
    ("420", 8, dict(pel=1), dict(blksize=16, overlap=0), 7),
    ("420", 8, dict(pel=2), dict(B168, divide=1), 2),
    ("420", 16, dict(pel=2), B84, 3),
    ("444", 8, dict(pel=2), B84, 2),
    ("gray", 8, dict(pel=1), B168, 2),
]
# every field at radius 1 and 3, the first and the last at radius 7, one of a divided clip, of 16 bits, of 4:4:4
FIELD_CASES = [(ANALYSE_CASES[0], f) for f in range(2)] + [(ANALYSE_CASES[1], f) for f in range(6)] + [(ANALYSE_CASES[2], 0), (ANALYSE_CASES[2], 13),
               (ANALYSE_CASES[3], 3), (ANALYSE_CASES[4], 4), (ANALYSE_CASES[5], 1)]


def analyse_id(c):
    fmt, bits, skw, akw, radius = c
    return "%s-%dbit-r%d-%s" % (fmt, bits, radius, ",".join("%s=%s" % kv for d in (skw, akw) for kv in sorted(d.items())))


def analyse_multi(c):
    fmt, bits, skw, akw, radius = c
    return mu.multi(fmt, bits, skw, akw, radius, fmt_kw=FORMATS[fmt])


# ---- RecalculateN: a subset of the C ABI's cases (tests/multi_oracle.py), both geometries, the three formats, radius 1 .. 7, divide and smooth=0
RECALC_CASES = [c for c in mu.recalc_cases() if c[4] or (c[0], c[1], c[2][0], c[3]) in
                {("420", 8, "16-8to8-4", 1), ("420", 16, "8-4to8-0", 3), ("444", 8, "16-8to8-4", 7), ("420", 8, "8-4to8-0", 2)}]

# ---- DegrainN: fmt, w, h, bits, super kwargs, analyse kwargs, the clip's radius, how it is checked, DegrainN's arguments, RecalculateN's (or None)
# The clips are tests/degrain_n_cases.py's (2 * radius + 1 frames of its (1, 0) motion), geometries A and B and its thresholds; every frame is produced and the
# middle one, the first and the last are compared
A, B = dc.A, dc.B
FALL = dict(thsad=1600, thsad2=400)   # degrain_n_cases' fall-off
DEGRAIN_CASES = [
    A + (1, "oracle", {}, None),
    A + (2, "oracle", dict(thsad=300, thsadc=200, limit=20), None),
    B + (3, "oracle", {}, None),
    A + (7, "ref", dict(FALL), None),
    A + (12, "ref", dict(FALL), None),
    B + (7, "ref", dict(thsad=1600, thsad2=400, thsadc=1000, thsadc2=250, plane=0), None),
    A + (3, "oracle", dict(radius=2), None),                 # a radius below the clip's: the first four fields
    A + (8, "ref", dict(radius=7, **FALL), None),
    A + (3, "out16", dict(out16=1), None),
    A + (7, "out16", dict(out16=1, **FALL), None),
    ("444", 128, 96, 8, {}, B84, 9, "ref", {}, None),
    ("gray", 128, 96, 8, {}, B84, 12, "ref", {}, None),
    ("444", 128, 96, 8, {}, B84, 2, "oracle", {}, None),
    ("gray", 128, 96, 8, {}, B84, 3, "out16", dict(out16=1), None),
    A + (3, "oracle", {}, dict(blksize=8, overlap=0, thsad=mu.RECALC_THSAD)),   # behind RecalculateN
]


def degrain_id(c):
    fmt, w, h, bits, skw, akw, radius, how, fargs, rkw = c
    return "%s-%dx%d-%dbit-r%d-%s-%s%s" % (fmt, w, h, bits, radius, how, ",".join("%s=%s" % kv for d in (skw, akw, fargs) for kv in sorted(d.items())), "-recalculated" if rkw else "")


def degrain_multi(c):
    fmt, w, h, bits, skw, akw, radius = c[:7]
    return mu.multi(fmt, bits, skw, akw, radius, w=w, h=h, nframes=2 * radius + 1, fmt_kw=FORMATS[fmt])


def degrain_inputs(c):
    """-> (the multi clip, DegrainN's radius, its other arguments, analysis data and blobs[n][r] of the vectors it is handed)"""
    m = degrain_multi(c)
    fargs, rkw = dict(c[8]), c[9]
    radius = fargs.pop("radius", m.radius)
    fargs.pop("out16", None)
    ads, blobs = m.recalc(**rkw) if rkw else (m.ads, m.blobs)
    return m, radius, fargs, ads[0], blobs


def degrain_ref(oracle, c):
    """the restatement of a "ref" / "out16" case: thresholds per distance from the formula in Python"""
    m, radius, dkw, ad, _ = degrain_inputs(c)
    make = o16.restatement if c[7] == "out16" else dc.restatement
    return make(oracle, radius, ad, *dc.tables(ad, radius, dkw), dkw, gray=m.fmt == "gray")


def degrain_expected(oracle, c, frames=None):
    """[n] -> planes, or None for a frame that is not compared"""
    m, radius, dkw, ad, blobs = degrain_inputs(c)
    frames = (0, m.n // 2, m.n - 1) if frames is None else frames
    how = c[7]
    out = [None] * m.n
    for n in frames:
        refs = [m.ref(n, r) for r in range(2 * radius)]
        if how == "oracle":
            out[n] = mo.Degrain(radius, m.osup, ad, **dkw).frame(m.frames[n], refs, blobs[n][:2 * radius])
        elif how == "ref":
            out[n] = degrain_ref(oracle, c).frame(m.frames[n], refs, blobs[n][:2 * radius])
        else:
            out[n] = o16.frame(degrain_ref(oracle, c), m.frames[n], refs, blobs[n][:2 * radius])
    return out


# ---- CompensateN: fmt, bits, geometry of tests/multi_cases.py, the clip's radius, name, CompensateN's arguments, extra host arguments, environment
# (96x64, 2 * radius + 3 frames: every output frame of every source frame is compared)
THSAD = mc.THSAD
# thscd1 / thscd2 at which, through the oracle's SADs, SOME (frame, field) pairs of the case are scene changes and some are not (tests/test_vs_multi_cases.py)
SC = dict(thscd1=150, thscd2=110)
COMPENSATE_CASES = [
    ("420", 8, mc.B84, 1, "tr1", dict(thsad=THSAD), (), {}),
    ("420", 8, mc.B84, 3, "tr3", dict(thsad=THSAD), (), {}),
    ("420", 16, mc.B160, 7, "tr7", dict(thsad=THSAD), (), {}),
    ("444", 8, mc.B84, 3, "tr2-of-3", dict(thsad=THSAD, tr=2), (), {}),
    ("420", 8, mc.B84, 2, "time50", dict(thsad=THSAD, time="50.0"), (), {}),
    ("420", 8, mc.B84, 3, "scene-scb0", dict(thsad=THSAD, scbehavior=0, **SC), (), {}),
    ("420", 8, mc.B84, 3, "scene-scb1", dict(thsad=THSAD, scbehavior=1, **SC), (), {}),
    ("gray", 8, mc.B160, 2, "gray", dict(thsad=THSAD), (), {}),
    # the same expectation however the frames are asked for: four threads asking for output frames only; last to first; a table of two sets, so that sets are
    # evicted and computed again
    ("420", 8, mc.B84, 3, "threads4", dict(thsad=THSAD), ("x.threads=4", "x.order=frame"), {}),
    ("420", 8, mc.B84, 3, "reverse", dict(thsad=THSAD), ("x.order=reverse",), {}),
    ("420", 8, mc.B84, 3, "threads4-two-sets", dict(thsad=THSAD), ("x.threads=4", "x.order=frame"), {"MVX_VS_MULTI_SETS": "2"}),
    ("420", 8, mc.B84, 3, "reverse-one-set", dict(thsad=THSAD), ("x.order=reverse",), {"MVX_VS_MULTI_SETS": "1"}),
]


def compensate_id(c):
    return "%s-%dbit-%s-r%d-%s" % (c[0], c[1], c[2][0], c[3], c[4])


def compensate_multi(c):
    fmt, bits, blk, radius = c[:4]
    return mu.multi(fmt, bits, blk[1], blk[2], radius, fmt_kw=FORMATS[fmt])


def compensate_tr(c):
    return c[5].get("tr", c[3])


def compensate_map(tr, k):
    """output k of a source frame, in temporal order (include/mvtools_amd.h, mvx_compensate_n_map): (offset of its frame, field of the multi blob or -1 for the centre) --
    before the centre the forward field (odd) of distance tr - k, behind it the backward field (even) of distance k - tr"""
    if k == tr:
        return 0, -1
    return (k - tr, 2 * (tr - k - 1) + 1) if k < tr else (k - tr, 2 * (k - tr - 1))


def compensate_expected(oracle, c):
    """[n * (2 tr + 1) + k] -> planes: oracle.Compensate of (frame n, its field's reference, its field's vectors); the centre is the clip's frame"""
    m = compensate_multi(c)
    tr = compensate_tr(c)
    ckw = {k: (float(v) if isinstance(v, str) else v) for k, v in c[5].items() if k != "tr"}
    comps = {}
    out = []
    for n in range(m.n):
        for k in range(2 * tr + 1):
            _, field = compensate_map(tr, k)
            if field < 0:
                out.append(m.frames[n])
                continue
            if field not in comps:
                comps[field] = mo.Compensate(m.osup, m.ads[field], **ckw)
            out.append(comps[field].frame(m.osf[n], m.ref(n, field), m.blobs[n][field]))
    return out


def scene_changes(m, fields, thscd1, thscd2):
    """[(n, field)] -> True where the oracle's vectors of a valid (frame, field) count as a scene change (MVAnalysisData.c:7-31, fgopIsUsable: the blocks whose SAD
    exceeds the scaled thscd1 number more than the scaled thscd2)"""
    out = {}
    for n in range(m.n):
        for f in fields:
            if m.nref(n, f) is None:
                continue
            _, s1, s2 = vector_fields.scaled_thresholds(m.ads[f], 400, thscd1, thscd2)
            sad = pl.blob_vectors(m.blobs[n][f], m.ads[f])[2]
            out[(n, f)] = int((sad > s1).sum()) > s2
    return out
