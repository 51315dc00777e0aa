"""A restatement of mv.DepanEstimate (MVDepan.cpp:651-883 frame_data2d, mult_conj_data2d, get_motion_vector; :1000-1243 stages 2 and 3;
:1271-1433 creation) in np.float32, in source order, the serial scan and mean included.  Test infrastructure: the product never imports it.

The FFT is pluggable, because the reference's (FFTW, single precision) cannot be built here: FFT64 is scipy.fft in double, the yardstick;
FFT32 is scipy.fft in single precision (pocketfft: rfft2 of a float32 array returns complex64), an independent single-precision FFT
standing in for fftw3f.  The distance between the two is what a second single-precision FFT may differ by.

Deliberate differences from the reference, the library's numbered divergences 8 to 11 (include/mvtools_amd.h): samples are read in the
clip's own type; a float clip, a window that is no power of two from 8 to 8192 and a window outside the frame are refused; a tiny dx becomes
+0.011."""
import numpy as np
import scipy.fft

f32 = np.float32


class CreateError(Exception):
    pass


def FFT64(real=None, spec=None, shape=None):
    if real is not None:
        return scipy.fft.rfft2(real.astype(np.float64))
    return scipy.fft.irfft2(spec.astype(np.complex128), s=shape) * (shape[0] * shape[1])   # unnormalised, as FFTW's c2r


def FFT32(real=None, spec=None, shape=None):
    if real is not None:
        out = scipy.fft.rfft2(real.astype(np.float32))
        assert out.dtype == np.complex64
        return out
    out = scipy.fft.irfft2(spec.astype(np.complex64), s=shape)
    assert out.dtype == np.float32
    return out * f32(shape[0] * shape[1])


def auto_window(room):
    w = 1
    for _ in range(13):
        if w * 2 <= room:
            w = w * 2
    return w


class Estimate:
    """depanEstimateCreate, :1271-1433, then the library's refusals"""

    def __init__(self, width, height, bits=8, trust=4.0, winx=0, winy=0, wleft=-1, wtop=-1, dxmax=-1, dymax=-1, zoommax=1.0, stab=1.0, pixaspect=1.0,
                 fields=False, tff=None, num_frames=1 << 30, float_samples=False):
        self.trust_limit, self.zoommax, self.stab, self.pixaspect = f32(trust), f32(zoommax), f32(stab), f32(pixaspect)
        self.fields, self.tff, self.num_frames, self.width, self.height, self.bits = bool(fields), tff, num_frames, width, height, bits
        if self.trust_limit < 0 or self.trust_limit > 100:
            raise CreateError("DepanEstimate: trust must be between 0.0 and 100.0 (inclusive).")
        if self.pixaspect <= 0:
            raise CreateError("DepanEstimate: pixaspect must be positive.")
        if (not float_samples and not 8 <= bits <= 16) or (float_samples and bits != 32):
            raise CreateError("DepanEstimate: clip must have constant format and dimensions, it must be YUV or Gray, and it must be 8..16 bit integer or 32 bit float.")
        wleft0 = wleft
        if wleft < 0:
            wleft = 0
        if winx > width - wleft:
            raise CreateError("DepanEstimate: winx must not be greater than width-wleft.")
        if winx == 0:
            winx = auto_window(width - wleft)
        if self.zoommax != 1:
            winx = winx // 2
            if wleft0 < 0:
                wleft = (width - winx * 2) // 4
        elif wleft0 < 0:
            wleft = (width - winx) // 2
        wtop0 = wtop
        if wtop < 0:
            wtop = 0
        if winy > height - wtop:
            raise CreateError("DepanEstimate: winy must not be greater than height-wtop.")
        if winy == 0:
            winy = auto_window(height - wtop)
        if wtop0 < 0:
            wtop = (height - winy) // 2
        if dxmax < 0:
            dxmax = winx // 4
        if dymax < 0:
            dymax = winy // 4
        if dxmax >= winx // 2:
            raise CreateError("DepanEstimate: dxmax must be less than winx/2.")
        if dymax >= winy // 2:
            raise CreateError("DepanEstimate: dymax must be less than winy/2.")
        self.windows = 2 if self.zoommax != 1 else 1
        if float_samples:
            raise CreateError("DepanEstimate: float clips are not supported.")
        ok = lambda v: 8 <= v <= 8192 and v & (v - 1) == 0
        if not ok(winx) or not ok(winy):
            raise CreateError("DepanEstimate: winx (after the halving for zoom) and winy must be powers of two between 8 and 8192.")
        if wleft + (width // 2 if self.windows == 2 else 0) + winx > width or wtop + winy > height:
            raise CreateError("DepanEstimate: every window must lie inside the frame.")
        self.winx, self.winy, self.wleft, self.wtop, self.dxmax, self.dymax = winx, winy, wleft, wtop, dxmax, dymax
        self.spectrum_bytes = winy * (winx // 2 + 1) * 8

    # ---- stage 1
    def window(self, luma, w):
        left = self.wleft + (self.width // 2 if w else 0)
        return luma[self.wtop:self.wtop + self.winy, left:left + self.winx]

    def spectra(self, luma, fft):
        return [fft(real=self.window(luma, w).astype(np.float32)) for w in range(self.windows)]

    # ---- stage 2
    @staticmethod
    def mult_conj(cur, prev):
        """:689-691 with fftnext = cur, fftsrc = prev, in the precision of the spectra"""
        re = cur.real * prev.real + cur.imag * prev.imag
        im = cur.real * prev.imag - cur.imag * prev.real
        return re + 1j * im if cur.dtype == np.complex128 else (re + 1j * im).astype(np.complex64)

    def surface(self, cur, prev, fft):
        """the correlation surface as the reference holds it: float"""
        return np.asarray(fft(spec=self.mult_conj(cur, prev), shape=(self.winy, self.winx))).astype(np.float32)

    def scan(self, correl):
        """:717-767, serially in float.  -> dict(max, sum, imax, jmax, xp, xm, yp, ym)"""
        winx, winy, dxmax, dymax = self.winx, self.winy, self.dxmax, self.dymax
        correlmax = correl[0, 0]
        correlmean = f32(0)
        imax = jmax = 0
        rows = list(range(0, dymax + 1)) + list(range(winy - dymax, winy))
        cols = list(range(0, dxmax + 1)) + list(range(winx - dxmax, winx))
        for j in rows:
            line = correl[j]
            for i in cols:
                cur = line[i]
                correlmean = f32(correlmean + cur)
                if correlmax < cur:
                    correlmax, imax, jmax = cur, i, j
        ip, im = (imax + 1) % winx, (imax - 1) % winx
        jp, jm = (jmax + 1) % winy, (jmax - 1) % winy
        return dict(max=f32(correl[jmax, imax]), sum=correlmean, imax=imax, jmax=jmax, xp=correl[jmax, ip], xm=correl[jmax, im], yp=correl[jp, imax],
                    ym=correl[jm, imax])

    def vector(self, S, top_field):
        """:769-882 -> fdx, fdy, trust and what the cases' margins are measured on"""
        winx, winy, dxmax, dymax, stab = self.winx, self.winy, self.dxmax, self.dymax, self.stab
        count = (2 * dxmax + 1) * (2 * dymax + 1)
        correlmean = f32(S["sum"] / f32(count))
        correlmax = f32(S["max"] / f32(winx * winy))
        correlmean = f32(correlmean / f32(winx * winy))
        trust = f32(f32(f32(correlmax - correlmean) * f32(100)) / f32(correlmax + f32(0.1)))
        imax, jmax = S["imax"], S["jmax"]
        dx = imax if imax * 2 < winx else imax - winx
        dy = jmax if jmax * 2 < winy else jmax - winy
        k = f32(f32(dxmax + 1) / f32(f32(dxmax + 1) + f32(stab * f32(abs(dx)))))
        k = f32(k * f32(dymax + 1))
        k = f32(k / f32(f32(dymax + 1) + f32(stab * f32(abs(dy)))))
        trust = f32(trust * k)
        dbg = dict(trust=trust, scene_change=bool(trust < self.trust_limit), dx=dx, dy=dy, xadd=f32(0), yadd=f32(0), raw_fdx=f32(0))
        if trust < self.trust_limit:
            return f32(0), f32(0), trust, dbg
        two = f32(2)

        def sub(p, m, c):
            f1 = f32(f32(p - m) / two)
            f2 = f32(f32(p + m) - f32(c * two))
            if f2 == 0:
                return f32(0)
            with np.errstate(all="ignore"):
                a = f32(-f1 / f2)
            return f32(1) if a > 1 else f32(-1) if a < -1 else a
        xadd = sub(S["xp"], S["xm"], S["max"])
        dbg["xadd"] = xadd
        if abs(f32(f32(dx) + xadd)) > dxmax:
            xadd = f32(0)
        yadd = sub(S["yp"], S["ym"], S["max"])
        dbg["yadd"] = yadd
        if abs(f32(f32(dy) + yadd)) > dymax:
            yadd = f32(0)
        if self.fields:
            yadd = f32(yadd + f32(0.5)) if top_field else f32(yadd + f32(-0.5))
            yadd = f32(yadd * two)
            dy = dy * 2
        fdx = f32(f32(dx) + xadd)
        fdy = f32(f32(dy) + yadd)
        fdy = f32(fdy / self.pixaspect)
        dbg["raw_fdx"] = fdx
        if abs(fdx) < f32(0.01):
            fdx = f32(0.011)
        return fdx, fdy, trust, dbg

    def top_field(self, n, prop):
        """:1016-1029; prop: the _Field property or None"""
        if not self.fields:
            return 0
        if prop is None and self.tff is None:
            raise CreateError("DepanEstimate: _Field property not found in input frame. Therefore, you must pass tff argument.")
        top = 0 if prop is None else int(bool(prop))
        if self.tff is not None:
            top = int(bool(self.tff)) ^ (n % 2)
        return top

    def combine(self, scans, n, prop=None):
        """:1063-1140 from the scans of the windows -> dict(dx, dy, zoom, trust, good_zoom, dbg)"""
        top = self.top_field(n, prop)
        dx1, dy1, trust1, dbg1 = self.vector(scans[0], top)
        dbg = [dbg1]
        good = None
        if self.windows == 1:
            mx, my, mz, trust = dx1, dy1, f32(1), trust1
        else:
            dx2, dy2, trust2, dbg2 = self.vector(scans[1], top)
            dbg.append(dbg2)
            zoom = f32(f32(1) + f32(f32(dx2 - dx1) / f32(self.width // 2)))
            good = bool(dx1 != 0 and dx2 != 0 and abs(f32(zoom - f32(1))) < f32(self.zoommax - f32(1)))
            if good:
                mx, my, mz = f32(f32(dx1 + dx2) / f32(2)), f32(f32(dy1 + dy2) / f32(2)), zoom
            else:
                mx, my, mz = f32(0), f32(0), f32(1)
            trust = min(trust1, trust2)
            dbg[0]["zoom_raw"] = zoom
        if n == 0:
            mx = my = trust = f32(0)
            mz = f32(1)
        return dict(dx=mx, dy=my, zoom=mz, trust=trust, good_zoom=good, dbg=dbg)

    def pair(self, prev_luma, cur_luma, n, fft, prop=None):
        sp, sc = self.spectra(prev_luma, fft), self.spectra(cur_luma, fft)
        surfaces = [self.surface(sc[w], sp[w], fft) for w in range(self.windows)]
        scans = [self.scan(s) for s in surfaces]
        out = self.combine(scans, n, prop)
        out["scans"], out["surfaces"] = scans, surfaces
        return out

    # ---- stage 3
    def finish(self, n, trio):
        """:1200-1227; trio: the stage-2 results of frames max(0, n - 1), n, min(n + 1, num_frames - 1) -> dx, dy, zoom, rot"""
        t0, t1, t2 = (f32(r["trust"]) for r in trio)
        mx, my, mz = f32(trio[1]["dx"]), f32(trio[1]["dy"]), f32(trio[1]["zoom"])
        if n - 1 >= 0 and n < self.num_frames and t1 < f32(self.trust_limit * f32(2)) and t1 < f32(f32(0.5) * t0):
            mx, my, mz = f32(0), f32(0), f32(1)
        if n >= 0 and n + 1 < self.num_frames and t1 < f32(self.trust_limit * f32(2)) and t1 < f32(f32(0.5) * t2):
            mx, my, mz = f32(0), f32(0), f32(1)
        return mx, my, mz, f32(0)
