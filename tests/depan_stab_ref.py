"""CPU restatement of mv.DepanStabilise (test infrastructure; tests/test_depan_stab_host.py holds the host planner, csrc/mvx_depan_stab_host.h,
to it, and tests/test_depan_stab_ref.py / tests/test_gpu_depan_stabilise.py the fused per-sample selection, csrc/mvx_depan_sample.h).

It follows the reference literally.  Citations are to dubhater/vapoursynth-mvtools src/MVDepan.cpp:
  creation      :3909-4163          Inertial      :2945-3115      Average   :3118-3246      InertialLimit :3249-3329
  the drivers   :3562-3709 (method 0), :3712-3885 (method 1)      the passes :3356-3546 compensateFrame / fillBorderPrev / fillBorderNext

Number formats as in depan_ref.py, whose transform algebra this imports: every float step is an np.float32 scalar in source order, libm's
float functions through ctypes.  The reference is C++ and includes <math.h>: sqrt, fabs and isfinite of a float are the float overloads.

The painting is sequential, as the reference does it: up to three calls of depan_ref.compensate_plane on one destination, each pass with
its own border value and mirror.  A pass with border -1 leaves a sample alone where the sample is undefined in its source; that set is
where compensate_plane with border 0 and with border pixel_max differ.  This is independent of the library's fused selection.
Chroma of the fill passes: the reference leaves tr[1] and tr[2] unassigned there; as the library does (mvtools_amd.h, DepanStabilise
divergence 1) each fill pass derives them from its own luma transform with depan_ref.plane_transforms.

Counters (stats) per painted frame, summed over its planes: from_cur / from_next / from_prev samples that end up from that source's
interior (for the first pass painted this includes its mirror, blur and border samples), passes: how many passes ran; and depan_ref's own
counters (mleft, blur, undef, ...) of the first pass painted, the only one with a mirror and a border value."""
import struct

import numpy as np

import depan_ref as dr
from depan_ref import f32, sqrtf, cosf

MOTIONBAD = f32(0.0)
DEFAULTS = dict(cutoff=1.0, damping=0.9, initzoom=1.0, addzoom=0, prev=0, next=0, mirror=0, blur=0, dxmax=60.0, dymax=30.0, zoommax=1.05, rotmax=1.0,
                subpixel=2, pixaspect=1.0, fitlast=0, tzoom=3.0, method=0, fields=0)


def cint(v):
    """C's (int) of a float, where it is defined"""
    return int(np.trunc(v))


class Stabilise:
    """the filter's state after depanStabiliseCreate; raises ValueError with the reference's text"""

    def __init__(self, width, height, num_frames, fps=(25, 1), bits=8, subsampling=(1, 1), gray=False, data_frames=None, **kw):
        a = dict(DEFAULTS)
        for k, v in kw.items():
            if k not in a:
                raise TypeError(k)
            if v is not None:
                a[k] = v
        self.args = dict(a)
        for k in ("cutoff", "damping", "initzoom", "dxmax", "dymax", "zoommax", "rotmax", "pixaspect", "tzoom"):
            setattr(self, k, f32(a[k]))
        for k in ("prev", "next", "mirror", "blur", "subpixel", "fitlast", "method"):
            setattr(self, k, int(a[k]))
        self.addzoom, self.fields = bool(a["addzoom"]), bool(a["fields"])
        self.width, self.height, self.num_frames, self.bits, self.subsampling, self.gray = width, height, num_frames, bits, tuple(subsampling), gray
        if self.cutoff <= 0:
            raise ValueError("DepanStabilise: cutoff must be greater than 0.")
        if self.prev < 0:
            raise ValueError("DepanStabilise: prev must not be negative.")
        if self.next < 0:
            raise ValueError("DepanStabilise: next must not be negative.")
        if self.subpixel < 0 or self.subpixel > 2:
            raise ValueError("DepanStabilise: subpixel must be between 0 and 2 (inclusive).")
        if self.pixaspect <= 0:
            raise ValueError("DepanStabilise: pixaspect must be greater than 0.")
        if self.mirror < 0 or self.mirror > 15:
            raise ValueError("DepanStabilise: mirror must be between 0 and 15 (inclusive).")
        if self.blur < 0:
            raise ValueError("DepanStabilise: blur must not be negative.")
        if self.method < 0 or self.method > 1:
            raise ValueError("DepanStabilise: method must be between 0 and 1 (inclusive).")
        if bits > 16 or tuple(subsampling) not in ((0, 0), (1, 0), (1, 1)):
            raise ValueError("DepanStabilise: clip must have constant format and dimensions, integer sample type, bit depth up to 16, and it must be Gray, 420, 422, or 444, and not RGB.")
        if fps[0] == 0 or fps[1] == 0:
            raise ValueError("DepanStabilise: clip must have known frame rate.")
        if num_frames > (num_frames if data_frames is None else data_frames):
            raise ValueError("DepanStabilise: data must have at least as many frames as clip.")
        # :4061
        self.zoommax = max(self.zoommax, self.initzoom) if self.zoommax > 0 else -max(-self.zoommax, self.initzoom)
        self.nfields = 2 if self.fields else 1
        one, six, three = f32(1), f32(6), f32(3)
        lam = sqrtf(one + six * self.damping * self.damping + sqrtf((one + six * self.damping * self.damping) * (one + six * self.damping * self.damping) + three))
        self.freqnative = self.cutoff / lam
        self.fps = f32(fps[0]) / f32(fps[1])
        five = f32(5)
        nl = {}
        nl["dxc"] = five / abs(self.dxmax) if self.dxmax != 0 else f32(0)
        nl["dxx"] = nl["dyy"] = five / (abs(self.zoommax) - one) if abs(self.zoommax) != 1 else f32(0)
        nl["dyc"] = five / abs(self.dymax) if self.dymax != 0 else f32(0)
        nl["dxy"] = nl["dyx"] = five / abs(self.rotmax) if self.rotmax != 0 else f32(0)
        self.nonlinfactor = nl
        self.initzoom = one / self.initzoom
        self.wintsize = cint(self.fps / (f32(4) * self.cutoff))
        self.radius = self.wintsize
        PI = f32(3.14159265258)
        half = f32(0.5)

        def table(size):
            w = np.zeros(self.wintsize + 1, dtype=f32)
            for i in range(size):
                w[i] = cosf(f32(i) * half * PI / f32(size))
            return w
        self.wint = table(self.wintsize)
        self.winrzsize = self.winfzsize = min(self.wintsize, cint(self.fps * self.tzoom / f32(4)))
        self.winrz, self.winfz = table(self.winrzsize), table(self.winfzsize)
        self.xcenter, self.ycenter = f32(width) / f32(2.0), f32(height) / f32(2.0)
        self.pixel_max = (1 << bits) - 1
        self.pa = self.pixaspect / f32(self.nfields)

    # ------------------------------------------------------------------------------------------ motions

    @staticmethod
    def motion(motions, n):
        """dx, dy, zoom, rot of data frame n as the filter holds it: frame 0 is set at creation, :4075-4078"""
        if n == 0:
            return f32(0), f32(0), f32(1), f32(0)
        return tuple(f32(v) for v in motions[n])

    def frame_transform(self, motions, n):
        dx, dy, zoom, rot = self.motion(motions, n)
        return dr.motion2transform(dx, dy, rot, zoom, self.pa, self.xcenter, self.ycenter, 1, 1.0)

    def zoom_transform(self, zoom):
        return dr.motion2transform(0, 0, 0, zoom, self.pa, self.xcenter, self.ycenter, 1, 1.0)

    def first_base(self, ndest):
        if self.method == 1:
            return max(0, ndest - self.radius)
        v = f32(ndest) - f32(10) * self.fps / self.cutoff
        return cint(v) if v > 0 else 0

    def window(self, ndest):
        """:3571-3591 / :3720-3763 -> data_first, data_last, clip_first, clip_last"""
        last = self.num_frames - 1
        nbase = self.first_base(ndest)
        nnext = min(ndest + self.next, last) if self.next else ndest
        dl = max(nnext, min(ndest + self.radius, last)) if self.method == 1 else nnext
        return nbase, dl, (max(nbase, ndest - self.prev) if self.prev else ndest), nnext

    # ------------------------------------------------------------------------------------------ smoothing

    def _azoom(self, trcur):
        dxc, dxx, dxy, dyc, dyx, dyy = [f32(v) for v in trcur]
        xc, yc, w, h, one = self.xcenter, self.ycenter, f32(self.width), f32(self.height), f32(1)
        az = self.initzoom
        t = one + (dxc + dxy * yc) / xc
        if t < az:
            az = t
        t = one - (dxc + dxx * w + dxy * yc - w) / xc
        if t < az:
            az = t
        t = one + (dyc + dyx * xc) / yc
        if t < az:
            az = t
        t = one - (dyc + dyx * xc + dyy * h - h) / yc
        if t < az:
            az = t
        return az

    def inertial(self, trcumul, nbase, ndest):
        """:2945-3115; trcumul[k] is frame nbase + k"""
        fn, two, half, one = self.freqnative, f32(2), f32(0.5), f32(1)
        cdamp = f32(12.56) * self.damping / self.fps
        cquad = f32(39.44) / (self.fps * self.fps)
        cnt = ndest - nbase + 1
        sm = [dr.null() for _ in range(cnt)]
        cu = trcumul

        def step(a, q, nl, s1, s2, c0, c1, c2):
            sn = two * s1 - s2 - \
                a * fn * (s1 - s2 - c1 + c2) * \
                (one + half * nl / fn * abs(s1 - s2 - c1 + c2)) - \
                q * fn * fn * (s1 - c1) * \
                (one + nl * abs(s1 - c1))
            sn = two * s1 - s2 - \
                a * fn * half * (sn - s2 - c0 + c2) * \
                (one + half * nl / fn * half * abs(sn - s2 - c0 + c2)) - \
                q * fn * fn * (s1 - c1) * \
                (one + nl * abs(s1 - c1))
            return f32(sn)
        DXC, DXX, DXY, DYC, DYX, DYY = range(6)
        nl = self.nonlinfactor
        for k in range(2, cnt):
            t = sm[k]
            t[DXC] = step(cdamp, cquad, nl["dxc"], sm[k - 1][DXC], sm[k - 2][DXC], cu[k][DXC], cu[k - 1][DXC], cu[k - 2][DXC])
            t[DXX] = half * (cu[k][DXX] + sm[k - 1][DXX])
            t[DXY] = step(cdamp * two, cquad * f32(4), nl["dxy"], sm[k - 1][DXY], sm[k - 2][DXY], cu[k][DXY], cu[k - 1][DXY], cu[k - 2][DXY])
            t[DYX] = -t[DXY] * self.pa * self.pa
            t[DYC] = step(cdamp, cquad, nl["dyc"], sm[k - 1][DYC], sm[k - 2][DYC], cu[k][DYC], cu[k - 1][DYC], cu[k - 2][DYC])
            t[DYY] = t[DXX]
        if self.addzoom:
            az = [self.initzoom] * cnt
            azs = [self.initzoom] * cnt

            def zstep(zf, s1, s2, a0, a1, a2):
                sn = two * s1 - s2 - \
                    zf * cdamp * fn * (s1 - s2 - a1 + a2) \
                    - zf * zf * cquad * fn * fn * (s1 - a1)
                sn = two * s1 - s2 - \
                    zf * cdamp * fn * half * (sn - s2 - a0 + a2) \
                    - zf * zf * cquad * fn * fn * (s1 - a1)
                return f32(sn)
            for k in range(2, cnt):
                trcur = dr.sumtransform(dr.inversetransform(cu[k]), sm[k])
                az[k] = self._azoom(trcur)
                zf = one / (self.cutoff * self.tzoom)
                azs[k] = zstep(zf, azs[k - 1], azs[k - 2], az[k], az[k - 1], az[k - 2])
                zf = zf * f32(0.7)
                if azs[k] > azs[k - 1]:
                    azs[k] = zstep(zf, azs[k - 1], azs[k - 2], az[k], az[k - 1], az[k - 2])
                if azs[k] > 1:
                    azs[k] = one
                sm[k] = dr.sumtransform(sm[k], self.zoom_transform(azs[k]))
        else:
            sm[cnt - 1] = dr.sumtransform(sm[cnt - 1], self.zoom_transform(self.initzoom))
        return dr.sumtransform(dr.inversetransform(cu[cnt - 1]), sm[cnt - 1])

    def average(self, trcumul, nbase, ndest, nmax):
        """:3118-3246; trcumul[k] is frame nbase + k"""
        cu = lambda n: trcumul[n - nbase]
        wint = self.wint
        DXC, DXX, DXY, DYC, DYX, DYY = range(6)
        sm = np.zeros(6, dtype=f32)
        norm = f32(0)
        for n in range(nbase, ndest):
            sm[DXC] = sm[DXC] + cu(n)[DXC] * wint[ndest - n]
            sm[DYC] = sm[DYC] + cu(n)[DYC] * wint[ndest - n]
            sm[DXY] = sm[DXY] + cu(n)[DXY] * wint[ndest - n]
            norm = norm + wint[ndest - n]
        for n in range(ndest, nmax + 1):
            sm[DXC] = sm[DXC] + cu(n)[DXC] * wint[n - ndest]
            sm[DYC] = sm[DYC] + cu(n)[DYC] * wint[n - ndest]
            sm[DXY] = sm[DXY] + cu(n)[DXY] * wint[n - ndest]
            norm = norm + wint[n - ndest]
        sm[DXC] = sm[DXC] / norm
        sm[DYC] = sm[DYC] / norm
        sm[DXY] = sm[DXY] / norm
        sm[DYX] = -sm[DXY] * self.pa * self.pa
        norm = f32(0)
        for n in range(max(nbase, ndest - 1), ndest):
            sm[DXX] = sm[DXX] + cu(n)[DXX] * wint[ndest - n]
            norm = norm + wint[ndest - n]
        for n in range(ndest, min(nmax, ndest + 1) + 1):
            sm[DXX] = sm[DXX] + cu(n)[DXX] * wint[n - ndest]
            norm = norm + wint[n - ndest]
        sm[DXX] = sm[DXX] / norm
        sm[DYY] = sm[DXX]
        if self.addzoom:
            nbasez, nmaxz = max(nbase, ndest - self.winfzsize), min(nmax, ndest + self.winrzsize)
            az = {nbasez: self.initzoom}
            for n in range(nbasez + 1, nmaxz + 1):
                az[n] = self._azoom(dr.sumtransform(dr.inversetransform(cu(n)), cu(n)))
            norm = f32(0)
            azs = f32(0)
            for n in range(nbasez, ndest):
                azs = azs + az[n] * self.winfz[ndest - n]
                norm = norm + self.winfz[ndest - n]
            for n in range(ndest, nmaxz + 1):
                azs = azs + az[n] * self.winrz[n - ndest]
                norm = norm + self.winrz[n - ndest]
            azs = azs / norm
            if azs > 1:
                azs = f32(1)
            sm = dr.sumtransform(sm, self.zoom_transform(azs))
        else:
            sm = dr.sumtransform(sm, self.zoom_transform(self.initzoom))
        return dr.sumtransform(dr.inversetransform(cu(ndest)), sm)

    def limit(self, dx, dy, zoom, rot, ndest, nbase, stats=None):
        """:3249-3329 -> dx, dy, zoom, rot, nbase"""
        one = f32(1)
        st = dict(v=[dx, dy, zoom, rot], nbase=nbase)

        def reset(which):
            st["v"] = [f32(0), f32(0), self.initzoom, f32(0)]
            st["nbase"] = ndest
            dr._bump(stats, "reset_" + which)

        def soft(i, vmax, which):
            v = st["v"][i]
            if not np.isfinite(v):
                reset(which)
            elif abs(v) > abs(vmax):
                if vmax >= 0:
                    st["v"][i] = sqrtf(v * vmax) if v >= 0 else -sqrtf(-v * vmax)
                    dr._bump(stats, "soft_" + which)
                else:
                    reset(which)
        soft(0, self.dxmax, "dx")
        soft(1, self.dymax, "dy")
        z = st["v"][2]
        if not np.isfinite(z):
            reset("zoom")
        elif abs(z - one) > abs(self.zoommax) - one:
            if self.zoommax >= 0:
                st["v"][2] = one + sqrtf(abs(z - one) * abs(self.zoommax - one)) if z >= 1 else one - sqrtf(abs(z - one) * abs(self.zoommax - one))
                dr._bump(stats, "soft_zoom")
            else:
                reset("zoom")
        soft(3, self.rotmax, "rot")
        return st["v"][0], st["v"][1], st["v"][2], st["v"][3], st["nbase"]

    # ------------------------------------------------------------------------------------------ one output frame

    def plan(self, ndest, motions, stats=None):
        """motions: per data frame of the whole clip (dx, dy, zoom, rot).  -> dict(tr, nbase, base, motion=(dx, dy, zoom, rot), prev, next) with
        prev / next None or dict(frame, tr); prev also carries `centred`, the frame the reference's dead test of :3415-3418 would name"""
        nbase = self.first_base(ndest)
        mx = lambda n: self.motion(motions, n)[0]

        def cumulative(first, last):
            cu = [dr.null()]
            for n in range(first + 1, last + 1):
                cu.append(dr.sumtransform(cu[-1], self.frame_transform(motions, n)))
            return cu
        for n in range(ndest, nbase - 1, -1):
            if mx(n) == MOTIONBAD:
                if n > nbase:
                    nbase = n
                break
        if self.method == 0:
            if nbase == ndest:
                trdif = self.zoom_transform(self.initzoom)
                dr._bump(stats, "scene_start")
            else:
                trdif = self.inertial(cumulative(nbase, ndest), nbase, ndest)
                dx, dy, rot, zoom = dr.transform2motion(trdif, 1, self.xcenter, self.ycenter, self.pa)
                if self.num_frames < self.fitlast + ndest + 1:
                    end = f32(self.num_frames - ndest - 1) / f32(self.fitlast)
                    dx, dy, rot = dx * end, dy * end, rot * end
                    zoom = self.initzoom + (zoom - self.initzoom) * end
                    dr._bump(stats, "fitlast")
                dx, dy, zoom, rot, nbase = self.limit(dx, dy, zoom, rot, ndest, nbase, stats)
                trdif = dr.motion2transform(dx, dy, rot, zoom, self.pa, self.xcenter, self.ycenter, 1, 1.0)
        else:
            nmax = min(ndest + self.radius, self.num_frames - 1)
            for n in range(ndest + 1, nmax + 1):
                if mx(n) == MOTIONBAD:
                    if n < nmax:
                        nmax = max(n - 1, ndest)
                    break
            smaller = min(nmax - ndest, ndest - nbase)
            if smaller < min(self.radius, ndest, self.num_frames - 1 - ndest):
                dr._bump(stats, "window_cut")
            nmax, nbase = ndest + smaller, ndest - smaller
            trdif = self.average(cumulative(nbase, nmax), nbase, ndest, nmax)
            dx, dy, rot, zoom = dr.transform2motion(trdif, 1, self.xcenter, self.ycenter, self.pa)
            trdif = dr.motion2transform(dx, dy, rot, zoom, self.pa, self.xcenter, self.ycenter, 1, 1.0)
        out = dict(tr=trdif, nbase=nbase, base=nbase == ndest, prev=None, next=None)
        if self.prev > 0:
            out["prev"] = self.fill_prev(motions, nbase, ndest, trdif, stats)
        if self.next > 0:
            out["next"] = self.fill_next(motions, ndest, trdif, stats)
        dx, dy, rot, zoom = dr.transform2motion(trdif, 1, self.xcenter, self.ycenter, self.pa)
        out["motion"] = np.array([dx, dy, zoom, rot], dtype=f32)
        # the library's rule (mvtools_amd.h, DepanStabilise divergence 6): which NaN an arithmetic ends on is not defined by IEEE 754 and differs
        # between builds of the same source, so a plan carries the positive quiet NaN wherever a coefficient is NaN
        for t in [out["tr"], out["motion"]] + [s["tr"] for s in (out["prev"], out["next"]) if s is not None]:
            t[np.isnan(t)] = np.uint32(0x7FC00000).view(f32)
        return out

    def fill_prev(self, motions, nbase, ndest, trdif, stats=None):
        """:3398-3419.  nprevbest = n is assigned unconditionally in every iteration, so the frame is always nprev"""
        nprev = max(ndest - self.prev, nbase)
        best, centred = nprev, nprev
        dabsmin = f32(10000)
        tr0 = np.array(trdif, dtype=f32)
        for n in range(ndest - 1, nprev - 1, -1):
            tr0 = dr.sumtransform(tr0, self.frame_transform(motions, n + 1))
            best = n
            dx, dy, _, _ = dr.transform2motion(tr0, 1, self.xcenter, self.ycenter, self.pa)
            d = abs(dx) + abs(dy) + f32(ndest) - f32(n)
            if d < dabsmin:
                dabsmin = d
                best = n
                centred = n
        if centred != best:
            dr._bump(stats, "prev_not_centred")
        return dict(frame=best, tr=tr0, centred=centred)

    def fill_next(self, motions, ndest, trdif, stats=None):
        """:3461-3502"""
        nnext = min(ndest + self.next, self.num_frames - 1)
        best = nnext
        dabsmin = f32(1000)
        tr0 = np.array(trdif, dtype=f32)
        for n in range(ndest + 1, nnext + 1):
            if self.motion(motions, n)[0] != MOTIONBAD:
                tr0 = dr.sumtransform(dr.inversetransform(self.frame_transform(motions, n)), tr0)
                dx, dy, _, _ = dr.transform2motion(tr0, 1, self.xcenter, self.ycenter, self.pa)
                d = abs(dx) + abs(dy) + f32(n) - f32(ndest)
                if d < dabsmin:
                    dabsmin = d
                    best = n
            else:
                best = n - 1
                dr._bump(stats, "next_cut")
                break
        if best == ndest:
            dr._bump(stats, "next_is_current")
        if best != nnext:
            dr._bump(stats, "next_chosen")
        return dict(frame=best, tr=tr0)

    # ------------------------------------------------------------------------------------------ painting

    def paint(self, cur, plan_tr, prev=None, next=None, stats=None):
        """the three passes of :3679-3693 on one destination.  cur: the planes of clip frame ndest; prev / next: None or (planes, luma
        transform) of that pass's source frame.  -> the planes"""
        return paint(cur, plan_tr, prev, next, self.subpixel, self.bits, self.subsampling, self.gray, self.mirror, self.blur, stats)


def plan_words(plan):
    """the 28 words of the library's plan structure as Stabilise.plan fills them: tr, nbase, base, motion, then prev and next as used, frame, tr"""
    def source(s):
        return bytes(32) if s is None else struct.pack("<2i", 1, s["frame"]) + np.asarray(s["tr"], f32).tobytes()
    b = np.asarray(plan["tr"], f32).tobytes() + struct.pack("<2i", plan["nbase"], int(plan["base"])) + np.asarray(plan["motion"], f32).tobytes() + \
        source(plan["prev"]) + source(plan["next"])
    return list(struct.unpack("<28I", b))


def _pass(dst, who, src, tr, subpixel, mirror, border, blur, pixel_max, name, stats=None):
    """one compensate_plane call on an existing destination; border < 0: samples undefined in src stay as they are.  `who` records which
    pass each sample came from last"""
    if border >= 0:
        out = dr.compensate_plane(src, tr, subpixel, mirror, border, blur, pixel_max, "library", stats)   # the first pass: depan_ref's counters too
        who[...] = name
        return out
    assert mirror == 0                                                    # mirror * notfilled, and notfilled is 0 whenever border is -1
    a = dr.compensate_plane(src, tr, subpixel, 0, 0, blur, pixel_max, "library")
    b = dr.compensate_plane(src, tr, subpixel, 0, pixel_max, blur, pixel_max, "library")
    defined = a == b
    who[defined] = name
    return np.where(defined, a, dst)


CUR, NEXT, PREV = 0, 1, 2


def paint(cur, plan_tr, prev, next, subpixel, bits=8, subsampling=(1, 1), gray=False, mirror=0, blur=0, stats=None):
    pm = (1 << bits) - 1
    out = []
    for p, (tc, b) in enumerate(dr.plane_transforms(plan_tr, subsampling, gray, blur)):
        border = 0 if p == 0 else 1 << (bits - 1)
        notfilled = 1
        dst = np.zeros_like(cur[p])           # never seen: the first pass paints every sample
        who = np.full(cur[p].shape, -1)
        if prev is not None:                   # fillBorderPrev: nearest, the full mirror, the border value
            tp = dr.plane_transforms(prev[1], subsampling, gray, blur)[p][0]
            dst = _pass(dst, who, prev[0][p], tp, 0, mirror, border, b, pm, PREV, stats)
            notfilled = 0
        if next is not None:                   # fillBorderNext: nearest, border -1 where prev painted, mirror * notfilled
            tn = dr.plane_transforms(next[1], subsampling, gray, blur)[p][0]
            dst = _pass(dst, who, next[0][p], tn, 0, mirror * notfilled, border if notfilled else -1, b, pm, NEXT, stats)
            notfilled = 0
        dst = _pass(dst, who, cur[p], tc, subpixel, mirror * notfilled, border if notfilled else -1, b, pm, CUR, stats)
        assert who.min() >= 0
        for name, key in ((CUR, "from_cur"), (NEXT, "from_next"), (PREV, "from_prev")):
            dr._bump(stats, key, (who == name).sum())
        dr._bump(stats, "passes", 1 + (prev is not None) + (next is not None))
        out.append(dst)
    return out
