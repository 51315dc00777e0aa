"""CPU restatement of the float rule of DepanCompensate and DepanStabilise (test infrastructure: tests/test_depan_float_ref.py
anchors it to depan_ref on integer-valued clips and holds csrc/mvx_depan_sample_float.h, compiled for the host, to it;
tests/test_gpu_depan_float.py and tests/test_gpu_depan_stabilise_float.py hold the HIP path to it).

Positions are depan_ref's: the plane under construction is a depan_ref._Plane (its if / else-if chain put(), the out-of-row rule, the rotation
forms' checked mirror), and _defined / _mirror_rows / _chain / bicubic_table / plane_transforms are called as they are.  depan_ref computes a
plane's positions inside compensate_plane, next to the integer arithmetic, and does not expose them; that body is restated here branch for
branch, each branch with the float rule's value in place of the integer one:
  copies    the sample's 32 bits (planes are carried as uint32, so a NaN payload, a denormal or -0.0f arrives as it left)
  border    0.0f luma, 0.5f chroma
  blur run  the float32 sum from 0.0f in index order, divided by the run's length
  bilinear  top = (32 - kx) * a + kx * b, bot the same on the row below, ((32 - ky) * top + ky * bot) * (1 / 1024), in all three forms
  bicubic   four row sums over the integer table, their column sum, one division by the product of the two coefficient totals, in all three
            forms; the near-edge rows are the reference's expression in float32; the zoom form's bottom row is (a + b) * 0.5
Every float step is np.float32 in source order; numpy fuses nothing.  Integers (kx, table entries, run lengths) are converted to float32
before they meet a sample, as C's usual conversions do with a float operand.

kind names where a sample came from (BORDER, COPY, BLUR, INTERP, NEAR, MEAN).  DepanStabilise's paint is sequential, as depan_stab_ref's: a
pass that is not the first leaves a sample alone where its kind is BORDER -- the painted flag, since a float sample may be negative."""
import numpy as np

import depan_ref as dr

f32, u32 = np.float32, np.uint32
BORDER, COPY, BLUR, INTERP, NEAR, MEAN = range(6)
_KIND = dict(nearest=COPY, mleft=COPY, mright=COPY, edgecol=COPY, bottom=COPY, blur=BLUR, interp=INTERP, near=NEAR, mean=MEAN)
BORDER_VALUE = (f32(0.0), f32(0.5))   # luma, chroma


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(u32)


class _FPlane(dr._Plane):
    def __init__(self, src, chroma, mode, stats):
        self.S = bits(src)                    # what at(), mirrored() and the copies move
        self.F = self.S.view(f32)
        self.H, self.W = src.shape
        self.v = np.full((self.H, self.W), np.array([BORDER_VALUE[bool(chroma)]], f32).view(u32)[0], dtype=u32)
        self.kind = np.full((self.H, self.W), BORDER, dtype=np.int8)
        self.done = np.zeros((self.H, self.W), dtype=bool)
        self.border, self.mode, self.stats = BORDER_VALUE[bool(chroma)], mode, stats

    def put(self, mask, fn, key):
        m = self.grid(mask) & ~self.done
        if m.any():
            r = fn(m)
            assert r.dtype in (f32, u32), r.dtype
            self.v[m] = r.view(u32)
            self.kind[m] = _KIND[key]
            dr._bump(self.stats, "bottom" if key == "mean" else key, m.sum())
        self.done = self.done | m

    def run(self, hl, lo, n):
        """mean of F[hl, lo : lo + n] per element: ((0 + x0) + x1) + ... in float32, then / n"""
        s = np.zeros(len(lo), f32)
        for k in range(int(n.max()) if len(n) else 0):
            on = k < n
            s = np.where(on, s + self.F[hl, np.where(on, lo + k, 0)], s)
        return s / n.astype(f32)

    def left(self, rows, hl, rl, mleft, blur):
        if not mleft:
            return
        c = rows & (rl < 0)
        self.out_of_domain(c & (-rl >= self.W), "left mirror beyond the row")
        if blur > 0:
            def run(m):
                r = self.grid(rl)[m]
                n = np.minimum(blur, -r)
                dr._bump(self.stats, "blur_short", (n < blur).sum())
                return self.run(self.grid(hl)[m], -r - n + 1, n)
            self.put(c, run, "blur")
        else:
            self.put(c, lambda m: self.S[self.grid(hl)[m], -self.grid(rl)[m]], "mleft")

    def right(self, rows, hl, rl, mright, blur, add, first):
        if not mright:
            return
        c = rows & (rl >= first)
        lo = self.W + self.W - rl - 2
        self.out_of_domain(c & (lo < 0), "right mirror before the row")
        if blur > 0:
            def run(m):
                r, l = self.grid(rl)[m], self.grid(lo)[m]
                n = np.minimum(blur, r - self.W + add)
                dr._bump(self.stats, "blur_short", (n < blur).sum())
                return self.run(self.grid(hl)[m], l, n)
            self.put(c, run, "blur")
        else:
            self.put(c, lambda m: self.S[self.grid(hl)[m], self.grid(lo)[m]], "mright")

    def fat(self, y, x, m, dy=0, dx=0):
        return self.F[self.grid(y)[m] + dy, self.grid(x)[m] + dx]

    def finish(self):
        dr._bump(self.stats, "border", (~self.done).sum())
        return self.v.view(f32), self.kind


def _lerp(F, y, x, kx, ky):
    fx, gx, fy, gy = kx.astype(f32), (32 - kx).astype(f32), ky.astype(f32), (32 - ky).astype(f32)
    top = gx * F[y, x] + fx * F[y, x + 1]
    bot = gx * F[y + 1, x] + fx * F[y + 1, x + 1]
    return (gy * top + fy * bot) * f32(1.0 / 1024)


def _cubic(F, y, x, cx, cy):
    fx, fy = cx.astype(f32), cy.astype(f32)
    ts = [fx[:, 0] * F[y - 1 + j, x - 1] + fx[:, 1] * F[y - 1 + j, x] + fx[:, 2] * F[y - 1 + j, x + 1] + fx[:, 3] * F[y - 1 + j, x + 2] for j in range(4)]
    pixel = fy[:, 0] * ts[0] + fy[:, 1] * ts[1] + fy[:, 2] * ts[2] + fy[:, 3] * ts[3]
    return pixel / (cx.sum(axis=1) * cy.sum(axis=1)).astype(f32)


def plane(src, tr, subpixel, mirror=0, chroma=False, blur=0, mode="library", stats=None):
    """one float32 plane -> (values as float32, kind).  The branches are depan_ref.compensate_plane's, in its order."""
    tr = [f32(v) for v in tr]
    dxc, dxx, dxy, dyc, dyx, dyy = tr
    pl = _FPlane(src, chroma, mode, stats)
    H, W, S, F = pl.H, pl.W, pl.S, pl.F
    if H < 2 or W < 2:
        raise dr.OutOfDomain("a plane smaller than 2 x 2")
    cls = 0 if (dxy == 0 and dyx == 0 and dxx == 1 and dyy == 1) else 1 if (dxy == 0 and dyx == 0) else 2
    dr._bump(stats, "cls%d" % cls)
    mleft, mright = bool(mirror & 4), bool(mirror & 8)
    hs, rs = np.arange(H, dtype=f32), np.arange(W, dtype=f32)
    tab = dr.bicubic_table()

    if cls == 2:
        if subpixel == 2:
            X = (dxc + dxx * rs)[None, :] + (dxy * hs)[:, None]
            Y = (dyc + dyx * rs)[None, :] + (dyy * hs)[:, None]
        else:
            X, Y = dr._chain(pl, tr)
        okx, X = dr._defined(pl, X)
        oky, Y = dr._defined(pl, Y)
        dr._undefined(pl, okx & oky)
        if subpixel == 0:
            rl = np.trunc(X + f32(0.5)).astype(np.int64)
            hl = np.trunc(Y + f32(0.5)).astype(np.int64)
            pl.put((rl >= 0) & (rl < W) & (hl >= 0) & (hl < H), lambda m: S[hl[m], rl[m]], "nearest")
        elif subpixel == 1:
            rl = np.trunc(X).astype(np.int64)
            sx = X - rl.astype(f32)
            n = sx < 0
            sx, rl = np.where(n, sx + f32(1), sx), rl - n
            hl = np.trunc(Y).astype(np.int64)
            sy = Y - hl.astype(f32)
            n2 = sy < 0
            sy, hl = np.where(n2, sy + f32(1), sy), hl - n2
            dr._bump(stats, "neg_fix", n.sum() + n2.sum())
            kx, ky = np.trunc(sx * f32(32)).astype(np.int64), np.trunc(sy * f32(32)).astype(np.int64)
            pl.put((rl >= 0) & (rl < W - 1) & (hl >= 0) & (hl < H - 1), lambda m: _lerp(F, hl[m], rl[m], kx[m], ky[m]), "interp")
        else:
            rl = np.trunc(X).astype(np.int64)
            n = X < rl.astype(f32)
            rl = rl - n
            hl = np.trunc(Y).astype(np.int64)
            n2 = Y < hl.astype(f32)
            hl = hl - n2
            dr._bump(stats, "neg_fix", n.sum() + n2.sum())

            def interp(m):
                y, x = hl[m], rl[m]
                return _cubic(F, y, x, tab[np.trunc((X[m] - x.astype(f32)) * f32(256)).astype(np.int64)], tab[np.trunc((Y[m] - y.astype(f32)) * f32(256)).astype(np.int64)])
            pl.put((rl >= 1) & (rl < W - 2) & (hl >= 1) & (hl < H - 2), interp, "interp")
        pl.mirrored(hl, rl, mirror)
        return pl.finish()

    if cls == 0:
        ysrc = dyc + hs
        okx = np.full(W, bool(np.abs(dxc) < dr.LIMIT))
        xsrc = np.full(W, dxc if okx[0] else f32(0), dtype=f32)
        oky0 = True if subpixel < 2 else bool(np.abs(dyc) < dr.LIMIT)
    else:
        ysrc = dyc + dyy * hs
        okx, xsrc = dr._defined(pl, dxc + dxx * rs)
        oky0 = True
    oky, ysrc = dr._defined(pl, ysrc)
    oky = oky & oky0
    dr._undefined(pl, oky[:, None] & okx[None, :])
    half = f32(0.5) if subpixel == 0 else f32(0)
    hl0 = np.floor(ysrc + half).astype(np.int64) if subpixel == 0 else np.floor(ysrc).astype(np.int64)
    if cls == 0:
        inttr0 = int(np.floor(xsrc[0] + half)) if subpixel == 0 else int(np.floor(xsrc[0]))
        rl = inttr0 + np.arange(W, dtype=np.int64)
        fx = np.full(W, dxc - f32(inttr0), dtype=f32) if okx[0] else np.zeros(W, f32)
    else:
        rl = np.floor(xsrc + half).astype(np.int64) if subpixel == 0 else np.floor(xsrc).astype(np.int64)
        fx = xsrc - rl.astype(f32)
    fy = ysrc - hl0.astype(f32)
    hl = dr._mirror_rows(pl, hl0, mirror)[:, None]
    rl = rl[None, :]
    inrow = (rl >= 0) & (rl < W)

    if subpixel == 0:
        rows = (hl >= 0) & (hl < H)
        pl.put(rows & inrow, lambda m: pl.at(hl, rl, m), "nearest")
        pl.left(rows, hl, rl, mleft, blur)
        pl.right(rows, hl, rl, mright, blur, 1, W)
        return pl.finish()

    if subpixel == 1:
        kx = np.floor(fx * f32(32)).astype(np.int64)[None, :]
        ky = np.floor(fy * f32(32)).astype(np.int64)[:, None]
        rows = (hl >= 0) & (hl < H - 1)
        good = (rl >= 0) & (rl < W - 1)
        if cls == 0 and mode == "strict" and rows.any() and good.sum() < 2:
            raise dr.OutOfDomain("bilinear translation with %d good columns" % good.sum())
        pl.put(rows & good, lambda m: _lerp(F, pl.grid(hl)[m], pl.grid(rl)[m], pl.grid(kx)[m], pl.grid(ky)[m]), "interp")
        pl.left(rows, hl, rl, mleft, blur)
        pl.right(rows, hl, rl, mright, blur, 2, W - 1)
        last = hl == H - 1
        pl.put(last & inrow, lambda m: pl.at(hl, rl, m), "bottom")
        if cls == 0:
            pl.left(last, hl, rl, mleft, 0)
            pl.right(last, hl, rl, mright, 0, 2, W - 1)
        return pl.finish()

    ix = np.trunc(fx * f32(256)).astype(np.int64)[None, :]
    iy = np.trunc(fy * f32(256)).astype(np.int64)[:, None]
    rows = (hl >= 1) & (hl < H - 2)
    pl.put(rows & (rl >= 1) & (rl < W - 2), lambda m: _cubic(F, pl.grid(hl)[m], pl.grid(rl)[m], tab[pl.grid(ix)[m]], tab[pl.grid(iy)[m]]), "interp")
    pl.left(rows, hl, rl, mleft, blur)
    pl.right(rows, hl, rl, mright, blur, 1, W)
    pl.put(rows & ((rl == 0) | (rl == W - 1) | (rl == W - 2)), lambda m: pl.at(hl, rl, m), "edgecol")
    near = ~rows & ((hl == 0) | (hl == H - 2))
    if cls == 0:
        sx = np.full(W, dxc - f32(inttr0), dtype=f32)[None, :]
        sy = np.full(H, dyc - f32(int(np.floor(dyc))) if oky0 else f32(0), dtype=f32)[:, None]
    else:
        sx, sy = fx[None, :], fy[:, None]

    def edge(m):
        a, b, one = pl.grid(sx)[m], pl.grid(sy)[m], f32(1)
        return (one - b) * ((one - a) * pl.fat(hl, rl, m) + a * pl.fat(hl, rl, m, 0, 1)) + b * ((one - a) * pl.fat(hl, rl, m, 1, 0) + a * pl.fat(hl, rl, m, 1, 1))
    pl.put(near & (rl >= 0) & (rl < W - 1), edge, "near")
    pl.put(near & (rl == W - 1), lambda m: pl.at(hl, rl, m), "edgecol")
    pl.left(near, hl, rl, mleft, 0)
    pl.right(near, hl, rl, mright, 0, 1, W)
    last = ~rows & ~near & (hl == H - 1)
    if cls == 0:
        pl.put(last & inrow, lambda m: pl.at(hl, rl, m), "bottom")
    else:
        pl.put(last & inrow, lambda m: (pl.fat(hl, rl, m) + pl.fat(hl, rl, m, -1, 0)) * f32(0.5), "mean")
    pl.left(last, hl, rl, mleft, 0)
    pl.right(last, hl, rl, mright, 0, 1, W)
    return pl.finish()


def compensate_plane(src, tr, subpixel, mirror=0, chroma=False, blur=0, mode="library", stats=None):
    return plane(src, tr, subpixel, mirror, chroma, blur, mode, stats)[0]


def compensate_frame(planes, trsum, subpixel, subsampling=(1, 1), gray=False, mirror=0, blur=0, mode="library", stats=None, kinds=None):
    """every plane of a frame; kinds: a list that receives each plane's kind map"""
    out = []
    for p, (t, b) in enumerate(dr.plane_transforms(trsum, subsampling, gray, blur)):
        v, k = plane(planes[p], t, subpixel, mirror, p > 0, b, mode, stats)
        out.append(v)
        if kinds is not None:
            kinds.append(k)
    return out


CUR, NEXT, PREV = 0, 1, 2


def paint(cur, plan_tr, prev, next, subpixel, subsampling=(1, 1), gray=False, mirror=0, blur=0, stats=None, who=None):
    """DepanStabilise's three passes on one destination, in the reference's order (prev, next, the current frame), as depan_stab_ref.paint:
    cur: the planes of the current frame; prev / next: None or (planes, luma transform).  Only the first pass painted has the mirror bits and
    the border value; a later pass writes where it painted.  who: a list that receives per plane which pass each sample came from last"""
    out = []
    for p, (tc, b) in enumerate(dr.plane_transforms(plan_tr, subsampling, gray, blur)):
        dst, src_of = None, None
        passes = []
        if prev is not None:
            passes.append((PREV, prev[0][p], dr.plane_transforms(prev[1], subsampling, gray, blur)[p][0], 0))
        if next is not None:
            passes.append((NEXT, next[0][p], dr.plane_transforms(next[1], subsampling, gray, blur)[p][0], 0))
        passes.append((CUR, cur[p], tc, subpixel))
        for name, s, t, sub in passes:
            first = dst is None
            v, kind = plane(s, t, sub, mirror if first else 0, p > 0, b, "library", stats if first else None)
            if first:
                dst, src_of = bits(v).copy(), np.full(v.shape, name)
            else:
                painted = kind != BORDER
                dst = np.where(painted, bits(v), dst)
                src_of = np.where(painted, name, src_of)
        for name, key in ((CUR, "from_cur"), (NEXT, "from_next"), (PREV, "from_prev")):
            dr._bump(stats, key, (src_of == name).sum())
        dr._bump(stats, "passes", len(passes))
        out.append(dst.view(f32))
        if who is not None:
            who.append(src_of)
    return out
