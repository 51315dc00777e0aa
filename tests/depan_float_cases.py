"""The float DepanCompensate / DepanStabilise cases shared by tests/test_depan_float_ref.py (CPU) and tests/test_gpu_depan_float.py,
tests/test_gpu_depan_stabilise_float.py (GPU): the geometries, transforms, mirror and blur values of depan_cases.CASES / LIBRARY_CASES and
depan_stab_cases.CASES (their `bits` is ignored: the clip is float32), with the sources a float path needs:
  int8     the values of the case's 8-bit noise clip as float32: what anchors the float rule to the integer restatement
  noise    float32 noise in [-0.25, 1.25): negative samples and values above 1 are ordinary in a float clip
  special  noise with NaNs of several payloads (quiet, signalling, negative), +-Inf, -0.0f, denormals and large negatives sprinkled in
  checker  the case's checkerboard, 0.0f / 1.0f
  flat     0.5f everywhere
The restatement's result is computed once per (case, source) and shared."""
import numpy as np

import depan_cases as dc
import depan_float_ref as fr
import depan_stab_cases as sc

f32, u32 = np.float32, np.uint32
SPECIALS = np.array([0x7FC00000, 0x7FC12345, 0x7F812345, 0xFFC00001, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x007FFFFF,
                     0xBFC00000, 0xFF7FFFFF, 0x7F7FFFFF], dtype=u32)   # NaNs, Infs, -0.0f, denormals, -1.5f, -+FLT_MAX


def eight(c):
    """the case with an 8-bit integer clip: the twin the anchoring tests give to depan_ref"""
    return dict(c, bits=8)


def _plane(shape, kind, rng, c):
    h, w = shape
    if kind == "noise":
        return (rng.random((h, w), dtype=f32) * f32(1.5) - f32(0.25)).astype(f32)
    if kind == "special":
        v = (rng.random((h, w), dtype=f32) * f32(1.5) - f32(0.25)).astype(f32).view(u32)
        pick = rng.random((h, w)) < 0.3
        return np.where(pick, SPECIALS[rng.integers(0, len(SPECIALS), (h, w))], v).astype(u32).view(f32)
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        return ((xx // 3 + yy // 3) & 1).astype(f32)
    if kind == "flat":
        return np.full((h, w), 0.5, f32)
    raise ValueError(kind)


def source(c, kind="noise"):
    if kind == "int8":
        return [p.astype(f32) for p in dc.source(eight(c))]
    rng = np.random.default_rng(c["seed"] + 100)
    return [_plane(s, kind, rng, c) for s in dc.planes_shape(c)]


def sources(c, kind="noise"):
    """three frames for a DepanStabilise case"""
    if kind == "int8":
        return [[p.astype(f32) for p in fr_] for fr_ in sc.sources(eight(c))]
    rng = np.random.default_rng(c["seed"] + 200)
    return [[_plane(s, kind, rng, c) for s in dc.planes_shape(c)] for _ in range(3)]


_memo = {}


def expected(c, kind="noise"):
    """DepanCompensate: the source planes, per transform the planes of the float restatement and their kind maps, and the counters"""
    key = ("c", c["name"], kind)
    if key not in _memo:
        src = source(c, kind)
        f = dc.FORMATS[c["fmt"]]
        stats, want, kinds = {}, [], []
        for t in c["trs"]:
            k = []
            want.append(fr.compensate_frame(src, t, c["sub"], f["subsampling"], f.get("gray", False), c["mirror"], c["blur"], c["mode"], stats, k))
            kinds.append(k)
        _memo[key] = (src, want, kinds, stats)
    return _memo[key]


def stab_expected(c, kind="noise", src=None):
    """DepanStabilise: the three source frames, per job the planes the float restatement paints and which pass each sample came from, the counters"""
    key = ("s", c["name"], kind)
    if src is not None or key not in _memo:
        frames = sources(c, kind) if src is None else src
        f = dc.FORMATS[c["fmt"]]
        stats, want, who = {}, [], []
        for cur, nxt, prev in c["jobs"]:
            w = []
            want.append(fr.paint(frames[0], cur, None if prev is None else (frames[prev[0]], prev[1]), None if nxt is None else (frames[nxt[0]], nxt[1]), c["sub"],
                                 f["subsampling"], f.get("gray", False), c["mirror"], c["blur"], stats, w))
            who.append(w)
        if src is not None:
            return frames, want, who, stats
        _memo[key] = (frames, want, who, stats)
    return _memo[key]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=f32).view(u32), np.ascontiguousarray(b, dtype=f32).view(u32))


def first_diff(got, want):
    g, w = np.ascontiguousarray(got, dtype=f32).view(u32), np.ascontiguousarray(want, dtype=f32).view(u32)
    d = np.argwhere(g != w)
    if not len(d):
        return "equal"
    y, x = d[0]
    return "%d samples differ, first at row %d column %d: got %08x (%r) want %08x (%r)" % (len(d), y, x, g[y, x], got[y, x], w[y, x], want[y, x])


# ---- what the GPU tests of the float DepanCompensate and DepanStabilise share

def check(full, want, tolerant=None):
    """full: the guarded buffers of depan_cases.guarded; want: per job the float32 planes.  Every sample as uint32; tolerant: per job and plane a
    mask of samples where two NaNs of different bits count as equal (arithmetic on special values).  Guard rows and row tails stay 0xA5"""
    for k, planes in enumerate(want):
        for p, wp in enumerate(planes):
            buf = full[k][p].cpu().numpy()
            got = np.ascontiguousarray(buf[1:-1, :wp.shape[1] * 4]).view(f32)
            if tolerant is None:
                assert same_bits(got, wp), "job %d plane %d: %s" % (k, p, first_diff(got, wp))
            else:
                t = tolerant[k][p]
                ok = (got.view(u32) == bits(wp)) | (t & np.isnan(got) & np.isnan(wp))
                assert ok.all(), "job %d plane %d: %d samples differ" % (k, p, (~ok).sum())
            assert np.all(buf[0] == 0xA5) and np.all(buf[-1] == 0xA5), "job %d plane %d: a guard row was written" % (k, p)
            assert np.all(buf[1:-1, wp.shape[1] * 4:] == 0xA5), "job %d plane %d: bytes beyond the width were written" % (k, p)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(u32)


def stab_plan(mv, cur, nxt, prev):
    p = mv.DepanStabilisePlan()
    p.tr[:] = [float(v) for v in cur]
    for name, s in (("next", nxt), ("prev", prev)):
        if s is not None:
            d = getattr(p, name)
            d.used, d.frame = 1, s[0]
            d.tr[:] = [float(v) for v in s[1]]
    return p


def once(cases):
    """the cases without the 16-bit twins of the 8-bit ones: a float clip has one depth"""
    return [c for c in cases if not c["name"].endswith("_16")]
