"""The DepanCompensate parity cases shared by tests/test_depan_ref.py (CPU: every case is in domain and reaches the branches it names) and
tests/test_gpu_depan.py (GPU: bit-exact against tests/depan_ref.py).  A case is one filter object and one mvx_depan_compensate_frames call:
all its transforms are jobs of that call, on one source frame.

Sizes: 206 x 118 4:2:0 (chroma 103 x 59: odd, no multiple of the 256-sample workgroup or of the 64-column chain segment, with a row tail
under a 256-byte pitch), 70 x 38, and one case each of 4:2:2, 4:4:4 and Gray.  `need` names the counters of depan_ref the case must reach."""
import numpy as np

import depan_ref as dr

f32 = np.float32
FORMATS = {"420": dict(subsampling=(1, 1)), "422": dict(subsampling=(1, 0)), "444": dict(subsampling=(0, 0)), "gray": dict(subsampling=(0, 0), gray=True)}
up = lambda v: np.nextafter(f32(v), f32(np.inf))
dn = lambda v: np.nextafter(f32(v), f32(-np.inf))


def tr(dxc=0.0, dyc=0.0, dxx=1.0, dyy=None, dxy=0.0, dyx=None):
    return np.array([dxc, dxx, dxy, dyc, -dxy if dyx is None else dyx, dxx if dyy is None else dyy], dtype=f32)


def rot(deg, zoom=1.0, dxc=0.0, dyc=0.0):
    a = np.radians(deg)
    return tr(dxc, dyc, np.cos(a) * zoom, None, -np.sin(a) * zoom)


def fractions(w, sub=0):
    """translations: exactly on a table step of bilinear (1/32) and bicubic (1/256) and one ULP either side, -0.0, negative positions just
    above and below an integer, and shifts that leave two good columns at either side -- for bilinear, whose translation form is out of
    domain with fewer than two, two good columns of the half-width chroma planes of 4:2:0 (the luma planes then keep five and four; the
    4:4:4 and Gray cases have the shifts that leave two good luma columns)"""
    out = []
    for base in (2 + 5 / 32.0, 2 + 77 / 256.0, -4 + 31 / 32.0, -4 + 255 / 256.0):
        out += [tr(base, -base), tr(up(base), dn(-base)), tr(dn(base), up(-base))]
    out += [tr(-0.0, -0.0), tr(up(-3), dn(-3)), tr(dn(-3), up(-3)), tr(dn(0), up(0))]
    out += [tr(w - 5.5, 1.5), tr(-(w - 4), -1.5)] if sub == 1 else [tr(w - 3, 1.5), tr(-(w - 2), -1.5), tr(w - 3.5, 2.25)]
    return out


ZOOMS = [tr(0.25, -0.25, 1 + 2.0 ** -23), tr(-3.7, 2.2, 1.05), tr(6.3, -5.1, 0.93), tr(-0.0, -0.0, 1 - 2.0 ** -24), tr(up(-2), dn(3), 1.01), tr(40.5, 3.0, 1.3)]
# a rotation small enough that dxy != 0 while every position equals the zoom form's, real rotations either way, and one about the centre with zoom
ROTS = [tr(1.3, -2.6, 1.0, None, 1e-30), rot(1.7, 1.0, 3.2, -4.1), rot(-2.3, 1.02, -5.5, 6.5), rot(0.4, 0.97, -0.0, -0.0), rot(11.0, 1.0, -20.0, 9.0)]
SHIFTS = [tr(5.3, -4.6), tr(-5.3, 4.6), tr(-7.0, -3.0), tr(8.0, 2.0)]


def _case(name, fmt, w, h, bits, sub, trs, need, mirror=0, blur=0, mode="strict", src="noise", seed=1):
    return dict(name=name, fmt=fmt, w=w, h=h, bits=bits, sub=sub, trs=trs, need=tuple(need), mirror=mirror, blur=blur, mode=mode, src=src, seed=seed)


def _cases():
    out = []
    interp = {0: "nearest", 1: "interp", 2: "interp"}
    for sub in (0, 1, 2):
        for bits in (8, 16):
            tag = "s%d_%d" % (sub, bits)
            extra = ("near", "bottom", "edgecol") if sub == 2 else ("bottom",) if sub == 1 else ()
            # one good column is in domain everywhere but in bilinear's translation form
            one = [] if sub == 1 else [tr(206 - 2, 0.5)]
            out.append(_case("trans_" + tag, "420", 206, 118, bits, sub, fractions(206, sub) + one, ("cls0", interp[sub], "border") + extra))
            out.append(_case("zoom_" + tag, "420", 206, 118, bits, sub, ZOOMS, ("cls1", interp[sub], "border") + extra))
            out.append(_case("rot_" + tag, "420", 206, 118, bits, sub, ROTS, ("cls2", interp[sub], "border") + (("chain_differs",) if sub < 2 else ()) + (("neg_fix",) if sub else ())))
            out.append(_case("small_" + tag, "420", 70, 38, bits, sub, fractions(70, sub)[:6] + fractions(70, sub)[-2:] + ZOOMS[:3] + ROTS[:3], ("cls0", "cls1", "cls2")))
        for m, need in ((1, ("mtop",)), (2, ("mbottom",)), (4, ("mleft",)), (8, ("mright",)), (15, ("mtop", "mbottom", "mleft", "mright"))):
            out.append(_case("mirror%d_s%d" % (m, sub), "420", 206, 118, 8, sub, SHIFTS + ZOOMS[1:3] + ROTS[1:3], need, mirror=m))
        # blur 1, and 9: larger than the shift of 5 or 8, so that short runs occur; chroma takes blur / 2
        out.append(_case("blur1_s%d" % sub, "420", 206, 118, 16, sub, SHIFTS + ZOOMS[1:3], ("blur",), mirror=12, blur=1))
        out.append(_case("blur9_s%d" % sub, "420", 206, 118, 8, sub, SHIFTS + ZOOMS[1:3], ("blur", "blur_short"), mirror=15, blur=9))
        out.append(_case("f422_s%d" % sub, "422", 206, 118, 10, sub, SHIFTS[:2] + ZOOMS[1:2] + ROTS[1:3], ("cls0", "cls1", "cls2", "mleft"), mirror=15, blur=4))
        out.append(_case("f444_s%d" % sub, "444", 70, 38, 8, sub, SHIFTS[:2] + [tr(70 - 3, 0.5), tr(-(70 - 2), 0.5)] + ZOOMS[1:2] + ROTS[1:2], ("cls0", "cls1", "cls2"), mirror=5))
        out.append(_case("gray_s%d" % sub, "gray", 70, 38, 16, sub, SHIFTS[:2] + [tr(70 - 3, 0.5), tr(-(70 - 2), 0.5)] + ZOOMS[1:2] + ROTS[1:2], ("cls0", "cls1", "cls2"), mirror=10, blur=2))
    # bicubic overshoot on 0-and-max checkerboards: the clamp at both ends, at 8, 10 and 16 bits, in all three forms
    for bits in (8, 10, 16):
        out.append(_case("clamp_%d" % bits, "420", 70, 38, bits, 2, [tr(0.5, 0.5), tr(0.25, 0.75, 1.01), rot(3.0, 1.0, 0.5, 0.5)], ("clamp_lo", "clamp_hi", "trunc"), src="checker"))
    return out


def _library_cases():
    """out of domain on purpose: defined behaviour of the library (mvtools_amd.h, divergence 2 and 5), compared with depan_ref's library mode"""
    out = []
    for sub in (0, 1, 2):
        # a mirrored shift of at least the width, either side, with and without blur
        out.append(_case("lib_wide_s%d" % sub, "420", 70, 38, 8, sub, [tr(75.0, 1.0), tr(-75.5, -1.0), tr(150.0, 0.0), tr(-150.0, 0.0), tr(90.0, 0.5, 1.02)], ("ood",), mirror=15, mode="library"))
        out.append(_case("lib_wide_blur_s%d" % sub, "420", 70, 38, 16, sub, [tr(75.0, 1.0), tr(-75.5, -1.0), tr(150.0, 0.0), tr(-150.0, 0.0)], ("ood",), mirror=12, blur=7, mode="library"))
        out.append(_case("lib_undef_s%d" % sub, "420", 70, 38, 8, sub, [tr(3e9, 0.0), tr(0.0, -3e9), tr(np.nan, 0.0), tr(1.0, 1.0, 3e8), rot(2.0, 1e9), tr(np.inf, 1.0, 1.0, None, 0.01)],
                         ("undef",), mirror=15, mode="library"))
    # bilinear translation with fewer than two good columns: inttr0 >= row_size - 2 and inttr0 <= 1 - row_size
    out.append(_case("lib_tail_s1", "420", 70, 38, 8, 1, [tr(68.5, 0.5), tr(69.0, 0.0), tr(70.25, 1.0), tr(-69.5, 0.5), tr(-70.0, 0.0), tr(-71.5, 0.0)], ("cls0",), mirror=0, mode="library"))
    out.append(_case("lib_tail_mirror_s1", "420", 70, 38, 8, 1, [tr(68.5, 0.5), tr(69.0, 0.0), tr(-69.5, 0.5), tr(-70.0, 0.0)], ("cls0", "mright"), mirror=15, blur=3, mode="library"))
    return out


# the launch shape tools/depan_bench.py measures: 1920 x 1080 4:2:0 8-bit; rotation for nearest and bilinear (the chain at 1920 columns), zoom for bicubic
FULL_CASES = [_case("full_s0", "420", 1920, 1080, 8, 0, [rot(0.7, 1.003, 4.2, -3.3)], ("cls2", "chain_differs"), mirror=15),
              _case("full_s1", "420", 1920, 1080, 8, 1, [rot(-0.6, 0.998, -6.5, 2.4)], ("cls2", "chain_differs", "interp"), mirror=15),
              _case("full_s2", "420", 1920, 1080, 8, 2, [tr(3.3, -2.7, 1.004)], ("cls1", "interp", "near"), mirror=15, blur=3)]
CASES = _cases()
LIBRARY_CASES = _library_cases()


def ids(cases):
    return [c["name"] for c in cases]


def planes_shape(c):
    f = FORMATS[c["fmt"]]
    if f.get("gray"):
        return [(c["h"], c["w"])]
    sw, sh = f["subsampling"]
    return [(c["h"], c["w"]), (c["h"] >> sh, c["w"] >> sw), (c["h"] >> sh, c["w"] >> sw)]


def source(c):
    pm = (1 << c["bits"]) - 1
    dt = np.uint16 if c["bits"] > 8 else np.uint8
    rng = np.random.default_rng(c["seed"])
    out = []
    for h, w in planes_shape(c):
        if c["src"] == "checker":
            yy, xx = np.mgrid[0:h, 0:w]
            out.append((((xx // 3 + yy // 3) & 1) * pm).astype(dt))   # cells of 3 x 3: bicubic overshoots beside an edge, not on a 1-sample pattern
        else:
            out.append(rng.integers(0, pm + 1, (h, w)).astype(dt))
    return out


def expected(c):
    """per transform the planes the restatement gives, and the counters summed over the case"""
    src = source(c)
    f = FORMATS[c["fmt"]]
    stats = {}
    want = [dr.compensate_frame(src, t, c["sub"], c["bits"], f["subsampling"], f.get("gray", False), c["mirror"], c["blur"], c["mode"], stats) for t in c["trs"]]
    return src, want, stats


def missing(c, stats):
    return [k for k in c["need"] if not stats.get(k)]


# ---- what the GPU tests of DepanCompensate and DepanStabilise share

def guarded(g, n):
    """n output frames, each plane inside a buffer with one guard row either side, all 0xA5"""
    import torch
    full = [[torch.full((g.info.plane_height[p] + 2, g.pitch[p]), 0xA5, dtype=torch.uint8, device="cuda") for p in range(g.nplanes)] for _ in range(n)]
    return full, [[t[1:-1] for t in fr] for fr in full]


def check(full, want, dtype):
    import pipeline as pl
    item = np.dtype(dtype).itemsize
    for k, planes in enumerate(want):
        for p, wp in enumerate(planes):
            buf = full[k][p].cpu().numpy()
            got = np.ascontiguousarray(buf[1:-1, :wp.shape[1] * item]).view(dtype)
            assert np.array_equal(got, wp), "job %d plane %d: %s" % (k, p, pl.first_diff(got, wp))
            assert np.all(buf[0] == 0xA5) and np.all(buf[-1] == 0xA5), "job %d plane %d: a guard row was written" % (k, p)
            assert np.all(buf[1:-1, wp.shape[1] * item:] == 0xA5), "job %d plane %d: bytes beyond the width were written" % (k, p)
