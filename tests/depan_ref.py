"""CPU restatement of mv.DepanCompensate and mv.DepanAnalyse (test infrastructure; the GPU parity tests compare the HIP path, mvx_depan.hip and mvx_depan_warp.hip,
and the host estimator, mvx_depan_host.h, against it).

It follows the reference literally.  Citations are to dubhater/vapoursynth-mvtools src/MVDepan.cpp:
  transform algebra   :78-142 setNull / transform2motion / inversetransform, :1554-1615 motion2transform / sumtransform
  estimator           :145-199 TrasformUpdate, :203-234 RejectBadBlocks, :279-399 the iteration of depanAnalyseGetFrame
  compensation        :1626-1847 nearest, :1855-2193 bilinear, :2202-2585 bicubic, :2616-2715 depanCompensateGetFrame

Number formats: every float step is np.float32 in source order (no fused multiply-add exists in numpy); the double steps of bicubic's
near-edge rows are np.float64, which is the C double (their `sx * srcp[...]` products are float, as C's promotion rules make them).  sinf / cosf / expf / logf / atanf are the C library's float functions through
ctypes: numpy's float32 versions are its own SIMD code and can differ in the last place.  C `/` truncates while Python `//` floors:
cdiv() is used wherever an operand can be negative.  `>>` of a negative int is arithmetic in both.

The planes are computed whole: positions, branch masks and samples are (rows x columns) arrays.  The addition chain of the rotation form
of nearest and bilinear (xsrc += dxx per column, :1840, :2186) is a loop over columns with whole-column vectors.

Two modes.  `strict` raises OutOfDomain at the first index the reference would take outside its row or plane, and at positions that are
NaN or not inside (-2^30, 2^30), where its float -> int conversion is undefined.  `library` applies the library's rule (mvtools_amd.h,
divergence 2 and 5): the border value there, and nothing written outside the row.

Counters (stats) name what a frame reached, summed over its planes:
  cls0 / cls1 / cls2   planes that took the translation / zoom / rotation form
  interp               samples from the interpolator proper       nearest   samples copied from the nearest / edge column
  mtop / mbottom       rows (fast forms) or samples (rotation) whose row was mirrored     mleft / mright  samples mirrored at a side
  blur                 samples that are the mean of a blur run     blur_short  of these, runs shorter than blur
  near / bottom        samples of bicubic's near-edge rows (double) / of the last row rule      edgecol  bicubic's edge columns
  border               samples filled with the border value        clamp_lo / clamp_hi  bicubic results clamped at 0 / pixel_max
  ood                  (library mode) samples that took the border value because the reference's index left its row
  undef                (library mode) samples whose position is outside what the reference defines
  chain_differs        rotation form of nearest / bilinear: samples whose accumulated position differs from x0 + k * dxx
  trunc                bicubic translation: negative coefficient products with a remainder (C truncation differs from floor)
  neg_fix              rotation forms: positions whose (int) truncation was corrected downwards
"""
import ctypes as C
import ctypes.util

import numpy as np

f32 = np.float32
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("sinf", "cosf", "expf", "logf", "atanf", "sqrtf"):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float]
sinf, cosf, expf, logf, atanf, sqrtf = (lambda fn: (lambda x: f32(fn(float(x)))))(_libm.sinf), (lambda fn: (lambda x: f32(fn(float(x)))))(_libm.cosf), \
    (lambda fn: (lambda x: f32(fn(float(x)))))(_libm.expf), (lambda fn: (lambda x: f32(fn(float(x)))))(_libm.logf), \
    (lambda fn: (lambda x: f32(fn(float(x)))))(_libm.atanf), (lambda fn: (lambda x: f32(fn(float(x)))))(_libm.sqrtf)
PI = f32(3.1415926535897932384626433832795)
MOTIONBAD = f32(0.0)
LIMIT = f32(1073741824.0)
np.seterr(all="ignore")


class OutOfDomain(Exception):
    pass


def cdiv(a, b):
    """C's truncating integer division, scalars or arrays"""
    a = np.asarray(a, dtype=np.int64)
    q = np.abs(a) // abs(int(b))
    return np.where((a < 0) == (b < 0), q, -q)


# ------------------------------------------------------------------------------------------------ transform algebra

def null():
    return np.array([0, 1, 0, 0, 0, 1], dtype=f32)  # dxc dxx dxy dyc dyx dyy, :78-85


def transform2motion(tr, forward, xcenter, ycenter, pixaspect):
    """:88-122 -> dx, dy, rot, zoom"""
    dxc, dxx, dxy, dyc, dyx, dyy = [f32(v) for v in tr]
    xcenter, ycenter, pixaspect = f32(xcenter), f32(ycenter), f32(pixaspect)
    rotradian = -atanf(pixaspect * dxy / dxx)
    rot = rotradian * f32(180) / PI
    sinus, cosinus = sinf(rotradian), cosf(rotradian)
    zoom = dxx / cosinus
    if forward:
        dx = dxc - xcenter - (-xcenter * cosinus + ycenter / pixaspect * sinus) * zoom
        dy = dyc / pixaspect - ycenter / pixaspect - ((-ycenter) / pixaspect * cosinus + (-xcenter) * sinus) * zoom
    else:
        dx = dxc / zoom * cosinus + dyc / zoom / pixaspect * sinus - xcenter / zoom * cosinus + xcenter - ycenter / zoom / pixaspect * sinus
        dy = -dxc / zoom * sinus + dyc / zoom / pixaspect * cosinus + xcenter / zoom * sinus - (-ycenter / pixaspect) - ycenter / zoom / pixaspect * cosinus
    return f32(dx), f32(dy), f32(rot), f32(zoom)


def inversetransform(ta):
    """:128-142"""
    dxc, dxx, dxy, dyc, dyx, dyy = [f32(v) for v in ta]
    pixaspect = sqrtf(-dyx / dxy) if dxy != 0 else f32(1.0)
    ixx = dxx / (dxx * dxx + dxy * dxy * pixaspect * pixaspect)
    iyy = ixx
    ixy = -ixx * dxy / dxx
    iyx = -ixy * pixaspect * pixaspect
    ixc = -ixx * dxc - ixy * dyc
    iyc = -iyx * dxc - iyy * dyc
    return np.array([ixc, ixx, ixy, iyc, iyx, iyy], dtype=f32)


def motion2transform(dx1, dy1, rot, zoom1, pixaspect, xcenter, ycenter, forward, fractoffset):
    """:1554-1591"""
    dx1, dy1, rot, zoom1, pixaspect, xcenter, ycenter, fractoffset = [f32(v) for v in (dx1, dy1, rot, zoom1, pixaspect, xcenter, ycenter, fractoffset)]
    dx = fractoffset * dx1
    dy = fractoffset * dy1
    rotradian = fractoffset * rot * PI / f32(180)
    if abs(rotradian) < f32(1e-6):
        rotradian = f32(0.0)
    zoom = expf(fractoffset * logf(zoom1))
    if abs(zoom - f32(1.0)) < f32(1e-6):
        zoom = f32(1.0)
    sinus, cosinus = sinf(rotradian), cosf(rotradian)
    if forward:
        dxc = xcenter + (-xcenter * cosinus + ycenter / pixaspect * sinus) * zoom + dx
        dyc = ycenter + (((-ycenter) / pixaspect * cosinus + (-xcenter) * sinus) * zoom + dy) * pixaspect
    else:
        dxc = xcenter + ((-xcenter + dx) * cosinus - ((-ycenter) / pixaspect + dy) * sinus) * zoom
        dyc = ycenter + (((-ycenter) / pixaspect + dy) * cosinus + (-xcenter + dx) * sinus) * zoom * pixaspect
    return np.array([dxc, cosinus * zoom, -sinus / pixaspect * zoom, dyc, sinus * zoom * pixaspect, cosinus * zoom], dtype=f32)


def sumtransform(ta, tb):
    """:1599-1615 -> tba"""
    a = [f32(v) for v in ta]
    b = [f32(v) for v in tb]
    return np.array([b[0] + b[1] * a[0] + b[2] * a[3], b[1] * a[1] + b[2] * a[4], b[1] * a[2] + b[2] * a[5],
                     b[3] + b[4] * a[0] + b[5] * a[3], b[4] * a[1] + b[5] * a[4], b[4] * a[2] + b[5] * a[5]], dtype=f32)


def intoffset_of(offset):
    """:2835-2838"""
    o = f32(offset)
    return int(np.ceil(o)) if o > 0 else int(np.floor(o))


def frame_map(offset, ndest, num_frames):
    """:2594-2602 -> (nsrc, start, end) or None: the source frame passes through"""
    io = intoffset_of(offset)
    nsrc = ndest - io
    if io == 0 or nsrc < 0 or nsrc > num_frames - 1:
        return None
    return nsrc, min(nsrc, ndest), max(nsrc, ndest)


def motion_to_transform(motions, offset, width, height, pixaspect=1.0, fields=False, matchfields=True, top_field=None, tff=None, ndest=0):
    """:2616-2675 and the transform2motion of :2718-2719 -> trsum, (dx, dy, zoom, rot)"""
    io = intoffset_of(offset)
    forward = io > 0
    fractoffset = f32(offset)
    fractoffset = fractoffset + f32(1 if forward else -1)
    fractoffset = fractoffset - f32(io)
    nfields = 2 if fields else 1
    xcenter, ycenter = f32(width) / f32(2.0), f32(height) / f32(2.0)
    pa = f32(pixaspect) / f32(nfields)
    trsum = null()
    for m in motions:
        mx, my, mzoom, mrot = [f32(v) for v in m]
        if mx == MOTIONBAD:
            trsum = null()
            break
        trsum = sumtransform(trsum, motion2transform(mx, my, mrot, mzoom, pa, xcenter, ycenter, forward, fractoffset))
    if fields and matchfields:
        top = bool(top_field)
        if tff is not None:
            top = bool(tff) ^ bool(ndest % 2)
        trsum[3] = trsum[3] + (f32(-0.5) if top else f32(0.5))
    dx, dy, rot, zoom = transform2motion(trsum, forward, xcenter, ycenter, pa)
    return trsum, np.array([dx, dy, zoom, rot], dtype=f32)


def plane_transforms(trsum, subsampling, gray, blur):
    """:2683-2700 -> per plane (tr, blur)"""
    t = np.array(trsum, dtype=f32)
    if gray:
        return [(t, blur)]
    c = t.copy()
    cb = blur
    if tuple(subsampling) == (1, 1):
        c[0] = c[0] / f32(2)
        c[3] = c[3] / f32(2)
        cb = blur // 2
    elif tuple(subsampling) == (1, 0):
        c[0] = c[0] / f32(2)
        c[2] = c[2] / f32(2)
        c[4] = c[4] * f32(2)
        cb = blur // 2
    return [(t, blur), (c, cb), (c, cb)]


# ------------------------------------------------------------------------------------------------ compensation

def bicubic_table():
    """:2255-2260 -> (257, 4) ints"""
    i = np.arange(257, dtype=np.int64)
    return np.stack([-((i * (256 - i) * (256 - i)) // 8192), (256 * 256 * 256 - 2 * 256 * i * i + i * i * i) // 8192,
                     (i * (256 * 256 + 256 * i - i * i)) // 8192, -((i * i * (256 - i)) // 8192)], axis=1)


def _bump(stats, key, n=1):
    if stats is not None:
        stats[key] = stats.get(key, 0) + int(n)


class _Plane:
    """the output of one plane under construction: put() follows an if / else-if chain, the first mask that holds a sample wins"""

    def __init__(self, src, border, mode, stats):
        self.S = src.astype(np.int64)
        self.H, self.W = src.shape
        self.cs = np.concatenate([np.zeros((self.H, 1), np.int64), np.cumsum(self.S, axis=1)], axis=1)  # the blur runs are exact integer sums
        self.v = np.full((self.H, self.W), border, dtype=np.int64)
        self.done = np.zeros((self.H, self.W), dtype=bool)
        self.border, self.mode, self.stats = border, mode, stats

    def grid(self, a):
        return np.broadcast_to(a, (self.H, self.W))

    def put(self, mask, fn, key):
        m = self.grid(mask) & ~self.done
        if m.any():
            self.v[m] = fn(m)
            _bump(self.stats, key, m.sum())
        self.done = self.done | m

    def out_of_domain(self, mask, what, key="ood"):
        m = self.grid(mask) & ~self.done
        if m.any():
            if self.mode == "strict":
                y, x = np.argwhere(m)[0]
                raise OutOfDomain("%s at row %d column %d" % (what, y, x))
            _bump(self.stats, key, m.sum())
        self.done = self.done | m   # keeps the border value

    def at(self, y, x, m, dy=0, dx=0):
        return self.S[self.grid(y)[m] + dy, self.grid(x)[m] + dx]

    # the unchecked side mirrors of the translation and zoom forms (:1697-1716 and its copies): add is 1, or 2 in bilinear's middle rows
    def left(self, rows, hl, rl, mleft, blur):
        if not mleft:
            return
        c = rows & (rl < 0)
        self.out_of_domain(c & (-rl >= self.W), "left mirror beyond the row")
        if blur > 0:
            def run(m):
                r = self.grid(rl)[m]
                n = np.minimum(blur, -r)
                _bump(self.stats, "blur_short", (n < blur).sum())
                return (self.cs[self.grid(hl)[m], -r + 1] - self.cs[self.grid(hl)[m], -r - n + 1]) // n
            self.put(c, run, "blur")
        else:
            self.put(c, lambda m: self.S[self.grid(hl)[m], -self.grid(rl)[m]], "mleft")

    def right(self, rows, hl, rl, mright, blur, add, first):
        """first: the smallest rowleft that counts as beyond the right edge (row_size, or row_size - 1 in bilinear)"""
        if not mright:
            return
        c = rows & (rl >= first)
        lo = self.W + self.W - rl - 2
        self.out_of_domain(c & (lo < 0), "right mirror before the row")
        if blur > 0:
            def run(m):
                r, l = self.grid(rl)[m], self.grid(lo)[m]
                n = np.minimum(blur, r - self.W + add)
                _bump(self.stats, "blur_short", (n < blur).sum())
                return (self.cs[self.grid(hl)[m], l + n] - self.cs[self.grid(hl)[m], l]) // n
            self.put(c, run, "blur")
        else:
            self.put(c, lambda m: self.S[self.grid(hl)[m], self.grid(lo)[m]], "mright")

    def mirrored(self, hl, rl, mirror):
        """the rotation forms' fallback, every index checked (:1825-1838, :2171-2184, :2565-2578); hl, rl: (H, W)"""
        H, W = self.H, self.W
        rest = ~self.done
        t = rest & (hl < 0) & bool(mirror & 1)
        hl = np.where(t, -hl, hl)
        _bump(self.stats, "mtop", t.sum())
        t = rest & (hl >= H) & bool(mirror & 2)
        hl = np.where(t, H + H - hl - 2, hl)
        _bump(self.stats, "mbottom", t.sum())
        t = rest & (rl < 0) & bool(mirror & 4)
        rl = np.where(t, -rl, rl)
        _bump(self.stats, "mleft", t.sum())
        t = rest & (rl >= W) & bool(mirror & 8)
        rl = np.where(t, W + W - rl - 2, rl)
        _bump(self.stats, "mright", t.sum())
        self.put((rl >= 0) & (rl < W) & (hl >= 0) & (hl < H), lambda m: self.S[hl[m], rl[m]], "nearest")

    def finish(self, dtype):
        _bump(self.stats, "border", (~self.done).sum())
        return self.v.astype(dtype)  # the reference stores through PixelType


def _defined(pl, a):
    """the positions the reference defines, and the array with the others replaced by 0"""
    ok = np.abs(a) < LIMIT
    return ok, np.where(ok, a, f32(0))


def _mirror_rows(pl, hl, mirror):
    t = (hl < 0) & bool(mirror & 1)
    hl = np.where(t, -hl, hl)
    _bump(pl.stats, "mtop", t.sum())
    t = (hl >= pl.H) & bool(mirror & 2)
    _bump(pl.stats, "mbottom", t.sum())
    return np.where(t, pl.H + pl.H - hl - 2, hl)


def _chain(pl, tr):
    """:1804-1805,1840-1841 / :2136-2137,2186-2187: column k holds k sequential float additions"""
    dxc, dxx, dxy, dyc, dyx, dyy = tr
    hs = np.arange(pl.H, dtype=f32)
    xs, ys = dxc + dxy * hs, dyc + dyy * hs
    x0 = xs.copy()
    X, Y = np.empty((pl.H, pl.W), f32), np.empty((pl.H, pl.W), f32)
    for k in range(pl.W):
        X[:, k], Y[:, k] = xs, ys
        xs, ys = xs + dxx, ys + dyx
    _bump(pl.stats, "chain_differs", (X != x0[:, None] + np.arange(pl.W, dtype=f32)[None, :] * dxx).sum())
    return X, Y


def _undefined(pl, ok):
    pl.out_of_domain(~pl.grid(ok), "a position the reference does not define", "undef")


def compensate_plane(src, tr, subpixel, mirror=0, border=0, blur=0, pixel_max=255, mode="strict", stats=None):
    """one plane, compensate_plane_nearest / _bilinear / _bicubic by subpixel 0 / 1 / 2"""
    tr = [f32(v) for v in tr]
    dxc, dxx, dxy, dyc, dyx, dyy = tr
    pl = _Plane(src, border, mode, stats)
    H, W = pl.H, pl.W
    if H < 2 or W < 2:
        raise OutOfDomain("a plane smaller than 2 x 2")
    cls = 0 if (dxy == 0 and dyx == 0 and dxx == 1 and dyy == 1) else 1 if (dxy == 0 and dyx == 0) else 2   # :1666,1733
    _bump(stats, "cls%d" % cls)
    mleft, mright = bool(mirror & 4), bool(mirror & 8)
    hs, rs = np.arange(H, dtype=f32), np.arange(W, dtype=f32)
    S = pl.S

    if cls == 2:
        if subpixel == 2:
            X = (dxc + dxx * rs)[None, :] + (dxy * hs)[:, None]            # :2528-2529
            Y = (dyc + dyx * rs)[None, :] + (dyy * hs)[:, None]
        else:
            X, Y = _chain(pl, tr)
        okx, X = _defined(pl, X)
        oky, Y = _defined(pl, Y)
        _undefined(pl, okx & oky)
        if subpixel == 0:
            rl = np.trunc(X + f32(0.5)).astype(np.int64)                    # :1809,1815: (int), towards zero
            hl = np.trunc(Y + f32(0.5)).astype(np.int64)
            pl.put((rl >= 0) & (rl < W) & (hl >= 0) & (hl < H), lambda m: S[hl[m], rl[m]], "nearest")
        elif subpixel == 1:
            rl = np.trunc(X).astype(np.int64)                                # :2141-2153
            sx = X - rl.astype(f32)
            n = sx < 0
            sx, rl = np.where(n, sx + f32(1), sx), rl - n
            hl = np.trunc(Y).astype(np.int64)
            sy = Y - hl.astype(f32)
            n2 = sy < 0
            sy, hl = np.where(n2, sy + f32(1), sy), hl - n2
            _bump(stats, "neg_fix", n.sum() + n2.sum())
            kx, ky = np.trunc(sx * f32(32)).astype(np.int64), np.trunc(sy * f32(32)).astype(np.int64)

            def interp(m):
                y, x, a, b = hl[m], rl[m], kx[m], ky[m]
                return (((32 - a) * S[y, x] + a * S[y, x + 1]) * (32 - b) + ((32 - a) * S[y + 1, x] + a * S[y + 1, x + 1]) * b) >> 10   # :2164-2166
            pl.put((rl >= 0) & (rl < W - 1) & (hl >= 0) & (hl < H - 1), interp, "interp")
        else:
            rl = np.trunc(X).astype(np.int64)                                # :2530-2538
            n = X < rl.astype(f32)
            rl = rl - n
            hl = np.trunc(Y).astype(np.int64)
            n2 = Y < hl.astype(f32)
            hl = hl - n2
            _bump(stats, "neg_fix", n.sum() + n2.sum())
            tab = bicubic_table()

            def interp(m):
                y, x = hl[m], rl[m]
                cx = tab[np.trunc((X[m] - x.astype(f32)) * f32(256)).astype(np.int64)]
                cy = tab[np.trunc((Y[m] - y.astype(f32)) * f32(256)).astype(np.int64)]
                return _separable(pl, y, x, cx, cy, pixel_max)
            pl.put((rl >= 1) & (rl < W - 2) & (hl >= 1) & (hl < H - 2), interp, "interp")
        pl.mirrored(hl, rl, mirror)
        return pl.finish(src.dtype)

    # ---- translation and zoom: the row and the column are independent
    if cls == 0:
        ysrc = dyc + hs
        okx = np.full(W, bool(np.abs(dxc) < LIMIT))
        xsrc = np.full(W, dxc if okx[0] else f32(0), dtype=f32)
        oky0 = True if subpixel < 2 else bool(np.abs(dyc) < LIMIT)
    else:
        ysrc = dyc + dyy * hs
        okx, xsrc = _defined(pl, dxc + dxx * rs)
        oky0 = True
    oky, ysrc = _defined(pl, ysrc)
    oky = oky & oky0
    _undefined(pl, oky[:, None] & okx[None, :])
    half = f32(0.5) if subpixel == 0 else f32(0)
    hl0 = np.floor(ysrc + half).astype(np.int64) if subpixel == 0 else np.floor(ysrc).astype(np.int64)
    if cls == 0:
        inttr0 = int(np.floor(xsrc[0] + half)) if subpixel == 0 else int(np.floor(xsrc[0]))
        rl = inttr0 + np.arange(W, dtype=np.int64)
        fx = np.full(W, dxc - f32(inttr0), dtype=f32) if okx[0] else np.zeros(W, f32)
    else:
        rl = np.floor(xsrc + half).astype(np.int64) if subpixel == 0 else np.floor(xsrc).astype(np.int64)
        fx = xsrc - rl.astype(f32)
    fy = ysrc - hl0.astype(f32)                                              # before the mirror, as in the reference
    hl = _mirror_rows(pl, hl0, mirror)[:, None]
    rl = rl[None, :]
    inrow = (rl >= 0) & (rl < W)

    if subpixel == 0:                                                        # :1684-1727, :1755-1794
        rows = (hl >= 0) & (hl < H)
        pl.put(rows & inrow, lambda m: pl.at(hl, rl, m), "nearest")
        pl.left(rows, hl, rl, mleft, blur)
        pl.right(rows, hl, rl, mright, blur, 1, W)
        return pl.finish(src.dtype)

    if subpixel == 1:
        kx = np.floor(fx * f32(32)).astype(np.int64)[None, :]               # ix2 / 2, :1929, :2036
        ky = np.floor(fy * f32(32)).astype(np.int64)[:, None]               # iy2 / 2, :1923, :2052
        rows = (hl >= 0) & (hl < H - 1)
        good = (rl >= 0) & (rl < W - 1)
        if cls == 0 and mode == "strict":
            # :1946-1976: the paired loop's tail starts at rowgoodendpaired - 1; with fewer than two good columns it, or the "bad" loop, leaves the row
            if rows.any() and good.sum() < 2:
                raise OutOfDomain("bilinear translation with %d good columns" % good.sum())

        def interp(m):
            a, b = pl.grid(kx)[m], pl.grid(ky)[m]
            return ((32 - b) * (32 - a) * pl.at(hl, rl, m) + (32 - b) * a * pl.at(hl, rl, m, 0, 1) + b * (32 - a) * pl.at(hl, rl, m, 1, 0) + b * a * pl.at(hl, rl, m, 1, 1)) >> 10
        pl.put(rows & good, interp, "interp")
        pl.left(rows, hl, rl, mleft, blur)
        pl.right(rows, hl, rl, mright, blur, 2, W - 1)
        last = hl == H - 1                                                   # :2006-2018, :2113-2121
        pl.put(last & inrow, lambda m: pl.at(hl, rl, m), "bottom")
        if cls == 0:
            pl.left(last, hl, rl, mleft, 0)
            pl.right(last, hl, rl, mright, 0, 2, W - 1)
        return pl.finish(src.dtype)

    tab = bicubic_table()
    ix = np.trunc(fx * f32(256)).astype(np.int64)[None, :]                  # ix4 / 4, :2277, :2389
    iy = np.trunc(fy * f32(256)).astype(np.int64)[:, None]                  # iy4 / 4, :2271, :2398
    rows = (hl >= 1) & (hl < H - 2)
    if cls == 0:
        def interp(m):                                                        # :2279-2311
            cx, cy = tab[pl.grid(ix)[m]], tab[pl.grid(iy)[m]]
            acc = np.full(cx.shape[0], 1024, dtype=np.int64)
            for j in range(4):
                for i in range(4):
                    p = cy[:, j] * cx[:, i]
                    _bump(stats, "trunc", ((p < 0) & (p % 2048 != 0)).sum())
                    acc = acc + cdiv(p, 2048) * pl.at(hl, rl, m, j - 1, i - 1)
            assert np.abs(acc).max() < 2 ** 31
            return _clamp(pl, acc >> 11, pixel_max)
    else:
        def interp(m):                                                        # :2426-2438
            return _separable(pl, pl.grid(hl)[m], pl.grid(rl)[m], tab[pl.grid(ix)[m]], tab[pl.grid(iy)[m]], pixel_max)
    pl.put(rows & (rl >= 1) & (rl < W - 2), interp, "interp")
    pl.left(rows, hl, rl, mleft, blur)
    pl.right(rows, hl, rl, mright, blur, 1, W)
    pl.put(rows & ((rl == 0) | (rl == W - 1) | (rl == W - 2)), lambda m: pl.at(hl, rl, m), "edgecol")
    near = ~rows & ((hl == 0) | (hl == H - 2))                               # :2340-2358, :2465-2484
    if cls == 0:
        sx = np.full(W, dxc - f32(inttr0), dtype=f32)[None, :]
        sy = np.full(H, dyc - f32(int(np.floor(dyc))) if oky0 else f32(0), dtype=f32)[:, None]
    else:
        sx, sy = fx[None, :], fy[:, None]

    def edge(m):
        # (1.0 - sx) * srcp[w] is a double product, but sx * srcp[w + 1] is float * int: a FLOAT product, rounded before it joins the double sum
        a32 = pl.grid(sx)[m]
        a, b = a32.astype(np.float64), pl.grid(sy)[m].astype(np.float64)
        right = lambda dy: (a32 * pl.at(hl, rl, m, dy, 1).astype(f32)).astype(np.float64)
        v = np.trunc((1.0 - b) * ((1.0 - a) * pl.at(hl, rl, m) + right(0)) + b * ((1.0 - a) * pl.at(hl, rl, m, 1, 0) + right(1))).astype(np.int64)
        return _clamp(pl, v, pixel_max) if cls == 1 else v
    pl.put(near & (rl >= 0) & (rl < W - 1), edge, "near")
    pl.put(near & (rl == W - 1), lambda m: pl.at(hl, rl, m), "edgecol")
    pl.left(near, hl, rl, mleft, 0)
    pl.right(near, hl, rl, mright, 0, 1, W)
    last = ~rows & ~near & (hl == H - 1)                                     # :2359-2371, :2485-2497
    if cls == 0:
        pl.put(last & inrow, lambda m: pl.at(hl, rl, m), "bottom")
    else:
        pl.put(last & inrow, lambda m: (pl.at(hl, rl, m) + pl.at(hl, rl, m, -1, 0)) // 2, "bottom")
    pl.left(last, hl, rl, mleft, 0)
    pl.right(last, hl, rl, mright, 0, 1, W)
    return pl.finish(src.dtype)


def _clamp(pl, v, pixel_max):
    _bump(pl.stats, "clamp_lo", (v < 0).sum())
    _bump(pl.stats, "clamp_hi", (v > pixel_max).sum())
    return np.clip(v, 0, pixel_max)


def _separable(pl, y, x, cx, cy, pixel_max):
    """:2426-2438, :2549-2563: four row sums in int, the column sum in int64, >> 22"""
    S = pl.S
    ts = [cx[:, 0] * S[y - 1 + j, x - 1] + cx[:, 1] * S[y - 1 + j, x] + cx[:, 2] * S[y - 1 + j, x + 1] + cx[:, 3] * S[y - 1 + j, x + 2] for j in range(4)]
    assert max(np.abs(t).max() for t in ts) < 2 ** 31 if len(y) else True
    return _clamp(pl, (cy[:, 0] * ts[0] + cy[:, 1] * ts[1] + cy[:, 2] * ts[2] + cy[:, 3] * ts[3]) >> 22, pixel_max)


def compensate_frame(planes, trsum, subpixel, bits=8, subsampling=(1, 1), gray=False, mirror=0, blur=0, mode="strict", stats=None):
    """:2678-2711: every plane of a frame"""
    out = []
    for p, (t, b) in enumerate(plane_transforms(trsum, subsampling, gray, blur)):
        out.append(compensate_plane(planes[p], t, subpixel, mirror, 0 if p == 0 else 1 << (bits - 1), b, (1 << bits) - 1, mode, stats))
    return out


# ------------------------------------------------------------------------------------------------ estimator

def level0(blob, ad):
    """(validity, records as a structured array x / y / sad) of a MVTools_vectors blob (Fakery.c:110-146)"""
    b = np.ascontiguousarray(blob, dtype=np.uint8)
    ints = b[:8].view(np.int32)
    o = 8
    for _ in range(ad.nLvCount - 1):
        o += int(b[o:o + 4].view(np.int32)[0])
    n = ad.nBlkX * ad.nBlkY
    rec = b[o + 4:o + 4 + 16 * n].view(np.dtype([("x", "<i4"), ("y", "<i4"), ("sad", "<i8")]))
    return int(ints[1]), rec


class Analyse:
    """One DepanAnalyse filter over analysis data ad.  thscd1 / thscd2 are the scaled thresholds (MVAnalysisData.c:7-31)."""

    def __init__(self, ad, width, height, thscd1, thscd2, zoom=True, rot=True, pixaspect=1.0, error=15.0, wrong=10.0, zerow=0.05, fields=False, has_mask=False):
        self.ad, self.width, self.height = ad, width, height
        self.thscd1, self.thscd2 = int(thscd1), int(thscd2)
        self.zoom, self.rot, self.fields, self.has_mask = bool(zoom), bool(rot), bool(fields), bool(has_mask)
        self.pixaspect, self.error, self.wrong, self.zerow = f32(pixaspect), f32(error), f32(wrong), f32(zerow)
        nx, ny = ad.nBlkX, ad.nBlkY
        self.bx = np.tile(np.arange(nx, dtype=np.int64) * (ad.nBlkSizeX - ad.nOverlapX) + ad.nBlkSizeX // 2, ny)      # :307-308
        self.by = np.repeat(np.arange(ny, dtype=np.int64) * (ad.nBlkSizeY - ad.nOverlapY) + ad.nBlkSizeY // 2, nx)

    def usable(self, blob):
        if blob is None:
            return False
        valid, rec = level0(blob, self.ad)
        return valid == 1 and not int((rec["sad"] > self.thscd1).sum()) > self.thscd2

    def update(self, tr, dx, dy, w, safety, if_zoom, if_rot, pa):
        """:145-199; the sums are serial float chains in block order: a Python loop over float32 scalars"""
        tr = [f32(v) for v in tr]
        bxf, byf = self.bx.astype(f32), self.by.astype(f32)
        xdif = tr[0] + tr[1] * bxf + tr[2] * byf - bxf - dx                   # elementwise, each in source order
        ydif = tr[3] + tr[4] * bxf + tr[5] * byf - byf - dy
        two = f32(2)
        terms = [two * xdif * w, (two * bxf) * xdif * w, (two * byf) * xdif * w, two * ydif * w, (two * bxf) * ydif * w, (two * byf) * ydif * w,
                 w, (bxf * bxf) * w, (byf * byf) * w, (xdif * xdif + ydif * ydif) * w]
        start = [f32(0)] * 6 + [f32(0.1)] * 4
        acc = [_serial_sum(s, t) for s, t in zip(start, terms)]
        d_dxc, d_dxx, d_dxy, d_dyc, d_dyx, d_dyy, norm, x2, y2, error2 = acc
        if not if_zoom:
            d_dxx = d_dyy = f32(0)
        if not if_rot:
            d_dxy = d_dyx = f32(0)
        d_dxc = d_dxc / (norm * two)
        d_dxx = d_dxx / (x2 * two * f32(1.5))
        d_dxy = d_dxy / (y2 * two * f32(3))
        d_dyc = d_dyc / (norm * two)
        d_dyx = d_dyx / (x2 * two * f32(3))
        d_dyy = d_dyy / (y2 * two * f32(1.5))
        error2 = error2 / norm
        err = np.sqrt(error2)
        tr[0] = tr[0] - safety * d_dxc
        if if_zoom:
            tr[1] = tr[1] - safety * f32(0.5) * (d_dxx + d_dyy)
        tr[2] = tr[2] - safety * f32(0.5) * (d_dxy - d_dyx / (pa * pa))
        tr[3] = tr[3] - safety * d_dyc
        if if_zoom:
            tr[5] = tr[1]
        tr[4] = -pa * pa * tr[2]
        return tr, f32(err)

    def reject(self, tr, dx, dy, sad, wmask, global_dif, border, stats):
        """:203-234, vectorised: every test reads the inputs only"""
        nx, ny = self.ad.nBlkX, self.ad.nBlkY
        i, j = np.tile(np.arange(nx), ny), np.repeat(np.arange(ny), nx)
        bxf, byf = self.bx.astype(f32), self.by.astype(f32)
        nb = nx * ny
        n = np.arange(nb)
        offs = (-1 - nx, -nx, 1 - nx, -1, 1, -1 + nx, nx, 1 + nx)               # the reference's order of the eight neighbours
        inside = (n - 1 - nx >= 0) & (n + 1 + nx < nb)

        def deviation(D, inner):
            """the neighbours by flat index, as the reference reads them (at a side they wrap into the next row).  Where one lies outside
            the array -- only without the ignored border, i.e. with a mask -- the library skips the test (mvtools_amd.h, divergence 6)"""
            s = D[np.clip(n + offs[0], 0, nb - 1)] + D[np.clip(n + offs[1], 0, nb - 1)]
            for o in offs[2:]:
                s = s + D[np.clip(n + o, 0, nb - 1)]
            return inner & inside & (np.abs(s / f32(8) - D) > self.wrong)
        c_border = (i < border) | (i >= nx - border) | (j < border) | (j >= ny - border)
        c_sad = sad > self.thscd1
        _bump(stats, "r_outside", (~c_border & ~c_sad & ~inside & (((i > 0) & (i < nx - 1)) | ((j > 0) & (j < ny - 1)))).sum())
        c_x = deviation(dx, (i > 0) & (i < nx - 1))
        c_y = deviation(dy, (j > 0) & (j < ny - 1))
        c_gx = np.abs(tr[0] + tr[1] * bxf + tr[2] * byf - bxf - dx) > global_dif
        c_gy = np.abs(tr[3] + tr[4] * bxf + tr[5] * byf - byf - dy) > global_dif
        zero = (dx == 0) & (dy == 0)
        w = np.where(c_border | c_sad | c_x | c_y | c_gx | c_gy, f32(0), np.where(zero, self.zerow * wmask, wmask)).astype(f32)
        if stats is not None:
            first = lambda c, prev: int((c & ~prev).sum())
            prev = np.zeros_like(c_border)
            for key, c in (("r_border", c_border), ("r_sad", c_sad), ("r_x", c_x), ("r_y", c_y), ("r_gx", c_gx), ("r_gy", c_gy), ("r_zero", zero)):
                _bump(stats, key, first(c, prev))
                prev = prev | c
        return w

    def frame(self, blob, mask=None, top_field=False, stats=None):
        """:279-399 -> dict(dx, dy, zoom, rot, iter, error); the library's +0.011f where the reference draws the sign from rand()"""
        ad = self.ad
        n_fields = 2 if self.fields else 1
        pa = self.pixaspect / f32(n_fields)
        tr = null()
        errorcur = self.error * f32(2)
        it = 0
        if self.usable(blob):
            _, rec = level0(blob, ad)
            d_pel = f32(1.0) / f32(ad.nPel)
            dx, dy = rec["x"].astype(f32) * d_pel, rec["y"].astype(f32) * d_pel
            sad = rec["sad"].astype(np.int64)
            wmask = np.ones(len(dx), f32)
            if self.has_mask:
                inside = (self.bx < self.width) & (self.by < self.height)
                _bump(stats, "mask_outside", (~inside).sum())
                wmask = np.where(inside, mask[np.minimum(self.by, mask.shape[0] - 1), np.minimum(self.bx, mask.shape[1] - 1)].astype(f32), f32(1)).astype(f32)
            w = wmask.copy()
            border = 0 if self.has_mask else 4
            safety = f32(0.3)
            while it < 5:
                tr, errorcur = self.update(tr, dx, dy, w, safety, False, False, pa)
                w = self.reject(tr, dx, dy, sad, wmask, f32(1000.0), border, stats)
                it += 1
            errordif = f32(0.01)
            while it < 100:
                safety = f32(0.3) if it < 8 else f32(0.6) if it < 10 else f32(1.0)
                errorprev = errorcur
                tr, errorcur = self.update(tr, dx, dy, w, safety, self.zoom, self.rot, pa)
                if ((errorprev - errorcur) < errordif * f32(0.5) and it > 9) or errorcur < errordif:
                    break
                w = self.reject(tr, dx, dy, sad, wmask, errorcur * f32(2), border, stats)
                it += 1
        else:
            _bump(stats, "unusable")
        xcenter, ycenter = f32(self.width) / f32(2), f32(self.height) / f32(2)
        mx, my, mrot, mzoom = f32(0), f32(0), f32(0), f32(1)
        if errorcur < self.error:
            if ad.isBackward:
                _bump(stats, "inverse")
                mx, my, mrot, mzoom = transform2motion(inversetransform(tr), False, xcenter, ycenter, pa)
            else:
                mx, my, mrot, mzoom = transform2motion(tr, True, xcenter, ycenter, pa)
            if self.fields:
                my = my + (f32(0.5) if top_field else f32(-0.5)) * f32(2)
            if abs(mx) < f32(0.01):
                _bump(stats, "tiny_dx")
                mx = f32(0.011)
        elif self.usable(blob):
            _bump(stats, "bad_error")
        return dict(dx=f32(mx), dy=f32(my), zoom=f32(mzoom), rot=f32(mrot), iter=it, error=f32(errorcur))


def _serial_sum(start, terms):
    """((start + t0) + t1) + ... in float32: np.cumsum of a float32 array adds sequentially, one rounding per element"""
    if len(terms) == 0:
        return f32(start)
    a = np.concatenate([[f32(start)], terms.astype(f32)]).astype(f32)
    return f32(np.cumsum(a, dtype=f32)[-1])
