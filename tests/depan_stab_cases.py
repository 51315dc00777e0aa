"""The DepanStabilise painting cases shared by tests/test_depan_stab_ref.py (CPU: the kernel's per-sample text compiled for the host) and
tests/test_gpu_depan_stabilise.py (GPU), both bit-exact against the sequential painting of tests/depan_stab_ref.py.  A case is one filter object
and one mvx_depan_stabilise_frames call; its jobs are crafted plans over three noise frames (0 the current frame, 1 and 2 the usual next and
prev sources).  A job is (current transform, next, prev) with next / prev None or (source frame, luma transform).

Sizes as in tests/depan_cases.py: 206 x 118 4:2:0 (chroma 103 x 59), 70 x 38, and one case each of 4:2:2 at 10 bits, 4:4:4 and Gray.
`need` names counters of the restatement the case must reach, `zero` counters that must stay 0."""
import numpy as np

import depan_ref as dr
import depan_stab_ref as sr
from depan_cases import FORMATS, tr, rot, planes_shape

f32 = np.float32
# what was tried at 70 x 38 and 206 x 118: hundreds of samples from each of the three sources with every interpolator
T3 = (tr(9.3, -6.6), tr(-4, -11), tr(3, 2))
R3 = (rot(4, 1, 6.2, -5.1), rot(-3, 1.03, -7.5, 4.5), rot(1, 0.9, 2, 1))
Z3 = (tr(-6.3, 5.1, 1.04), tr(3.7, -2.2, 1.02), tr(0.5, 0.25, 0.9))


def track(n, seed, bad=(), pan=3.0, rot_deg=0.3, zoom=0.004):
    """a synthetic motion track: per data frame (dx, dy, zoom, rot), a random walk's steps of about +-pan pixels with small rotation and zoom;
    bad: frames whose dx is 0.0f"""
    r = np.random.default_rng(seed)
    m = [(f32(r.normal(0, pan)), f32(r.normal(0, pan)), f32(1 + r.normal(0, zoom)), f32(r.normal(0, rot_deg))) for _ in range(n)]
    for b in bad:
        m[b] = (f32(0), m[b][1], m[b][2], m[b][3])
    return m


def job(cur, nxt=None, prev=None, nsrc=1, psrc=2):
    return (cur, None if nxt is None else (nsrc, nxt), None if prev is None else (psrc, prev))


def combos():
    """the four combinations of prev / next; translation, zoom and rotation, alone and mixed across the sources of one job"""
    return [job(*T3), job(*R3), job(*Z3), job(Z3[0], R3[1], T3[2]), job(R3[0], T3[1], Z3[2]), job(T3[0], None, T3[2]), job(R3[0], None, R3[2]),
            job(T3[0], T3[1]), job(R3[0], Z3[1]), job(Z3[0]), job(R3[0])]


def _case(name, fmt, w, h, bits, sub, jobs, need=("from_cur", "from_next", "from_prev"), zero=(), mirror=0, blur=0, seed=1):
    return dict(name=name, fmt=fmt, w=w, h=h, bits=bits, sub=sub, jobs=jobs, need=tuple(need), zero=tuple(zero), mirror=mirror, blur=blur, seed=seed, src="noise")


def _cases():
    out = []
    nan = tr(np.nan, 0.0)
    for sub in (0, 1, 2):
        for bits in (8, 16):
            out.append(_case("combos_s%d_%d" % (sub, bits), "420", 206, 118, bits, sub, combos(), ("from_cur", "from_next", "from_prev", "cls0", "cls1", "cls2")))
            out.append(_case("small_s%d_%d" % (sub, bits), "420", 70, 38, bits, sub, combos()[:6] + combos()[-2:]))
        for m, need in ((1, ("mtop",)), (2, ("mbottom",)), (4, ("mleft",)), (8, ("mright",)), (15, ("mtop", "mbottom", "mleft", "mright"))):
            out.append(_case("mirror%d_s%d" % (m, sub), "420", 206, 118, 8, sub, combos()[:2] + combos()[5:], ("from_cur", "from_next", "from_prev") + need, mirror=m))
        out.append(_case("blur1_s%d" % sub, "420", 206, 118, 16, sub, [job(*T3), job(T3[0], None, T3[2]), job(T3[0], T3[1]), job(T3[0]), job(*Z3)],
                         ("from_cur", "from_next", "from_prev", "blur"), mirror=12, blur=1))
        out.append(_case("blur9_s%d" % sub, "420", 206, 118, 8, sub, [job(*T3), job(T3[0], None, T3[2]), job(T3[0], T3[1]), job(T3[0]), job(*Z3)],
                         ("from_cur", "from_next", "from_prev", "blur", "blur_short"), mirror=15, blur=9))
        out.append(_case("f422_s%d" % sub, "422", 206, 118, 10, sub, combos()[:5], mirror=15, blur=4))
        out.append(_case("f444_s%d" % sub, "444", 70, 38, 8, sub, combos()[:5], mirror=5))
        out.append(_case("gray_s%d" % sub, "gray", 70, 38, 16, sub, combos()[:5], mirror=10, blur=2))
        # divergence 5 of DepanCompensate: a NaN and an out-of-range current transform hand the whole plane to the other two sources, and with
        # no other source the whole plane takes the border value
        out.append(_case("undef_s%d" % sub, "420", 70, 38, 8, sub, [job(nan, T3[1], T3[2]), job(tr(3e9, 0.0), R3[1], R3[2]), job(nan, None, T3[2]), job(rot(2.0, 1e9), T3[1]), job(nan)],
                         ("from_next", "from_prev", "undef"), mirror=15))
        out.append(_case("undef_only_s%d" % sub, "420", 70, 38, 8, sub, [job(nan, T3[1], T3[2]), job(tr(0.0, -3e9), R3[1], None)], ("from_next", "from_prev"), zero=("from_cur",)))
        # a fill source that is the current frame itself with the current frame's transform: what fillBorderNext names when the frame after ndest is
        # bad, and fillBorderPrev at a base.  Nearest reaches one more row and column than bilinear and bicubic interpolate
        out.append(_case("self_s%d" % sub, "420", 70, 38, 8, sub, [job(T3[0], T3[0], T3[2], nsrc=0), job(R3[0], R3[0], R3[0], nsrc=0, psrc=0), job(Z3[0], None, Z3[0], psrc=0)],
                         ("from_cur", "from_prev") + (("from_next",) if sub else ())))
    # the current frame covers everything: no fill sample is read (bilinear's translation form leaves the last column to the border value)
    for sub in (0, 2):
        out.append(_case("covers_s%d" % sub, "420", 70, 38, 8, sub, [job(dr.null(), T3[1], T3[2]), job(dr.null(), None, R3[2]), job(dr.null(), R3[1])], ("from_cur",),
                         zero=("from_next", "from_prev"), mirror=15))
    return out


# the launch shape tools/depan_stabilise_bench.py measures: 1920 x 1080 4:2:0 8-bit with both fill sources
FULL_CASES = [_case("full_s0", "420", 1920, 1080, 8, 0, [job(rot(0.7, 1.003, 24.2, -13.3), rot(-0.4, 1.0, -10.0, 8.0), tr(5.0, 3.0))], mirror=15),
              _case("full_s1", "420", 1920, 1080, 8, 1, [job(rot(-0.6, 0.998, -26.5, 12.4), tr(8.0, -6.0), rot(0.3, 1.0, 4.0, 2.0))], mirror=15),
              _case("full_s2", "420", 1920, 1080, 8, 2, [job(tr(23.3, -12.7, 1.004), tr(-9.0, 7.0, 1.001), rot(0.5, 1.0, 3.0, 1.0))], mirror=15, blur=3)]
CASES = _cases()


def ids(cases):
    return [c["name"] for c in cases]


def sources(c):
    """three frames of noise"""
    pm = (1 << c["bits"]) - 1
    dt = np.uint16 if c["bits"] > 8 else np.uint8
    rng = np.random.default_rng(c["seed"])
    return [[rng.integers(0, pm + 1, s).astype(dt) for s in planes_shape(c)] for _ in range(3)]


_memo = {}


def expected(c):
    """the three source frames, per job the planes the restatement paints, and the counters summed over the case; computed once per case"""
    if c["name"] not in _memo:
        src = sources(c)
        f = FORMATS[c["fmt"]]
        stats = {}
        want = []
        for cur, nxt, prev in c["jobs"]:
            want.append(sr.paint(src[0], cur, None if prev is None else (src[prev[0]], prev[1]), None if nxt is None else (src[nxt[0]], nxt[1]), c["sub"], c["bits"],
                                 f["subsampling"], f.get("gray", False), c["mirror"], c["blur"], stats))
        _memo[c["name"]] = (src, want, stats)
    return _memo[c["name"]]


def missing(c, stats):
    return [k for k in c["need"] if not stats.get(k)] + [k for k in c["zero"] if stats.get(k)]
