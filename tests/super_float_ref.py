"""Numpy float32 restatement of the float Super (mvx_super_create_float), test infrastructure: written from the description of its arithmetic
(include/mvtools_amd.h), not from the kernels.  A float super clip has one level: the padded plane, for pel 2 the H / V / HV
half-pel planes, for pel 4 additionally the twelve averaged planes.  Every operation is the integer rule's in its order on np.float32: no
rounding term, a shift is a multiplication by the exact power of two, no clamp.

    sharp 0   (a + b) * 0.5; diagonal (((a + b) + c) + d) * 0.25, (a + c) * 0.5 in the last column, (a + b) * 0.5 in the last row, a in the corner
    sharp 1   ((s(X) + s(X+1)) * 9 - (s(X-1) + s(X+2))) * 0.0625, bilinear for X < 1 or X >= n - 3
    sharp 2   m2 = (m2 + m3) * 4; m2 -= (m1 + m4); m2 *= 5; m0 = (m0 + m5) + m2; m0 * 0.03125, bilinear for X < 2 or X >= n - 4
    X == n-1  the sample itself
    HV        sharp 1 and 2: the horizontal rule on the unrounded vertical plane
    pel 4     d = (a[shifted by ax, ay] + b) * 0.5 over (pw - ax) x (ph - ay), two dependent passes; the last column / row of a shifted one is 0

tests/test_super_float_ref.py anchors it to the oracle's Super on integer-valued clips."""
import numpy as np

F = np.float32

# (d, a, b, ax, ay): sub-pel plane d of pel 4 from planes a and b (MVFrame.cpp:1489-1524)
PASS1 = [(1, 0, 2, 0, 0), (9, 8, 10, 0, 0), (4, 0, 8, 0, 0), (6, 2, 10, 0, 0), (3, 0, 2, 1, 0), (11, 8, 10, 1, 0), (12, 0, 8, 0, 1), (14, 2, 10, 0, 1)]
PASS2 = [(5, 4, 6, 0, 0), (13, 12, 14, 0, 0), (7, 4, 6, 1, 0), (15, 12, 14, 1, 0)]


def half_rows(a, sharp):
    """the half-pel rule along the last axis of a float32 array"""
    a = np.asarray(a, F)
    n = a.shape[-1]
    X = np.arange(n)
    s = lambda k: a[..., np.clip(X + k, 0, n - 1)]
    out = (s(0) + s(1)) * F(0.5)
    if sharp == 1:
        v = ((s(0) + s(1)) * F(9.0) - (s(-1) + s(2))) * F(0.0625)
        out = np.where((X >= 1) & (X < n - 3), v, out)
    elif sharp == 2:
        m2 = (s(0) + s(1)) * F(4.0)
        m2 = m2 - (s(-1) + s(2))
        m2 = m2 * F(5.0)
        m0 = (s(-2) + s(3)) + m2
        out = np.where((X >= 2) & (X < n - 4), m0 * F(0.03125), out)
    out = np.where(X == n - 1, a, out)
    assert out.dtype == F
    return out


def half(a, sharp, axis):
    return np.moveaxis(half_rows(np.moveaxis(a, axis, -1), sharp), -1, axis)


def diagonal(p0):
    """the HV plane of sharp 0"""
    h, w = p0.shape
    Y, X = np.minimum(np.arange(h) + 1, h - 1), np.minimum(np.arange(w) + 1, w - 1)
    a, b, c, d = p0, p0[:, X], p0[Y, :], p0[Y][:, X]
    out = (((a + b) + c) + d) * F(0.25)
    out[:, w - 1] = ((a + c) * F(0.5))[:, w - 1]
    out[h - 1, :] = ((a + b) * F(0.5))[h - 1, :]
    out[h - 1, w - 1] = a[h - 1, w - 1]
    return out


def subpel_planes(plane, hpad, vpad, pel, sharp):
    """{sub-pel index: padded plane} of level 0 for one source plane (float32)"""
    p0 = np.pad(np.asarray(plane, F), ((vpad, vpad), (hpad, hpad)), mode="edge")
    if pel == 1:
        return {0: p0}
    H, V = half(p0, sharp, 1), half(p0, sharp, 0)
    HV = diagonal(p0) if sharp == 0 else half(V, sharp, 1)
    if pel == 2:
        return {0: p0, 1: H, 2: V, 3: HV}
    pl = {0: p0, 2: H, 8: V, 10: HV}
    ph, pw = p0.shape
    for ops in (PASS1, PASS2):
        new = {}
        for d, a, b, ax, ay in ops:
            o = np.zeros((ph, pw), F)
            o[:ph - ay, :pw - ax] = (pl[a][ay:, ax:] + pl[b][:ph - ay, :pw - ax]) * F(0.5)
            new[d] = o
        pl.update(new)
    return pl


def geometry(width, height, sub, gray, hpad, vpad, pel):
    """per plane (w, h, hpad, vpad) of a clip, and the super frame's plane shapes (rows, samples) at levels=1 (MVSuper.c:257-264)"""
    xr, yr = 1 << sub[0], 1 << sub[1]
    sw, sh = width + 2 * hpad, pel * pel * (height + 2 * vpad)
    if yr == 2 and sh & 1:
        sh += 1
    if xr == 2 and sw & 1:
        sw += 1
    planes = [(width, height, hpad, vpad)] + ([] if gray else [(width // xr, height // yr, hpad // xr, vpad // yr)] * 2)
    shapes = [(sh, sw)] + ([] if gray else [(sh // yr, sw // xr)] * 2)
    return planes, shapes


def frame(src, sub=(1, 1), gray=False, hpad=16, vpad=16, pel=2, sharp=2):
    """the super frame of one clip frame (float32 planes): -> (planes of the super clip's plane shapes, zero outside the defined rectangles,
    boolean masks of the defined samples)"""
    h, w = src[0].shape
    planes, shapes = geometry(w, h, sub, gray, hpad, vpad, pel)
    out, defined = [], []
    for p, ((pw_, ph_, hp, vp), shape) in enumerate(zip(planes, shapes)):
        o, m = np.zeros(shape, F), np.zeros(shape, bool)
        sp = subpel_planes(np.asarray(src[p], F)[:ph_, :pw_], hp, vp, pel, sharp)
        rows, cols = ph_ + 2 * vp, pw_ + 2 * hp
        for k, a in sp.items():
            o[k * rows:(k + 1) * rows, :cols] = a
            m[k * rows:(k + 1) * rows, :cols] = True
        out.append(o)
        defined.append(m)
    return out, defined
