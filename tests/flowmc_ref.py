"""CPU restatement of mv.Flow and mv.FlowBlur (test infrastructure; the GPU parity tests compare the HIP path against it).

It follows the reference literally over the Finest frame that mvoracle.Super.finest builds: full-resolution int16 vector planes from the
small fields of tests/flow_ref.py (small_fields, half_uv, upsize_i16, whose int16 resizer is pinned to the reference's AVX2 object code),
then the per-sample loops.  Citations are to dubhater/vapoursynth-mvtools src/:
  Flow        MVFlow.cpp:163-370 (frame), :391-593 (creation); fetch :93-116 flowFetch, shift :119-148 flowShift, memset :312,336-337
  FlowBlur    MVFlowBlur.c:143-326 (frame), :346-552 (creation); :72-130 RealFlowBlur

Integer semantics: C `/` truncates while numpy `//` floors, so every division of a possibly negative value goes through cdiv; `>>` on
signed values is arithmetic in both; int16 planes are widened to int64 before any product.

flowShift writes in raster order and the last writer wins.  NumPy does not define which of several writes to one index wins, so the
winner per destination is np.maximum.at over raster indices + 1 (0 = nobody wrote); tests/test_flowmc_host.py pins that form against a
literal transcription of the loop (shift_loop).
"""
import ctypes as C

import numpy as np

import mvoracle
import pipeline as pl
from flow_ref import _lib, half_uv, small_fields, take, upsize_i16


def cdiv(a, b):
    """C's int division: truncates toward zero"""
    q = np.abs(a) // np.abs(b)
    return np.where((a < 0) != (b < 0), -q, q)


def _grid(h, w, pel, off):
    lp = {1: 0, 2: 1, 4: 2}[pel]
    return (np.arange(h, dtype=np.int64) << lp)[:, None] + off[0], (np.arange(w, dtype=np.int64) << lp)[None, :] + off[1], lp


def fetch(fin, off, v, t, pel, w, h, dtype):
    """MVFlow.cpp:93-116 flowFetch over one plane: v = (V * time256 + 128) >> 8, the sample Finest[(h << lp) + vy][(w << lp) + vx].
    fin = the Finest plane of nref, off = (row, column) of its unpadded sample (0, 0), v = (VX, VY) full planes."""
    Y, X, _ = _grid(h, w, pel, off)
    vx, vy = v[0][:h, :w].astype(np.int64), v[1][:h, :w].astype(np.int64)
    return take(fin, Y + ((vy * t + 128) >> 8), X + ((vx * t + 128) >> 8)).astype(dtype)


def shift_targets(v, t, pel, w, h):
    """MVFlow.cpp:128-140: destination (row, column) of every source sample and whether it lies inside the plane"""
    lp = {1: 0, 2: 1, 4: 2}[pel]
    rounding, shift = 128 << lp, 8 + lp
    vx, vy = v[0][:h, :w].astype(np.int64), v[1][:h, :w].astype(np.int64)
    dy = np.arange(h, dtype=np.int64)[:, None] + ((-vy * t + rounding) >> shift)
    dx = np.arange(w, dtype=np.int64)[None, :] + ((-vx * t + rounding) >> shift)
    return dy, dx, (dy >= 0) & (dy < h) & (dx >= 0) & (dx < w)


def shift_winners(v, t, pel, w, h):
    """per destination: 1 + the raster index of the last source (in raster order) that lands on it, 0 where none does"""
    dy, dx, inside = shift_targets(v, t, pel, w, h)
    win = np.zeros(h * w, np.int64)
    np.maximum.at(win, (dy * w + dx)[inside], (np.arange(h * w, dtype=np.int64).reshape(h, w) + 1)[inside])
    return win.reshape(h, w)


def shift(fin, off, v, t, pel, w, h, bits, dtype, stats=None):
    """MVFlow.cpp:119-148 flowShift over one plane after the memset to pixel_max (:312,336-337): each source sample Finest[h << lp][w << lp]
    goes to (h + vy, w + vx), v = (-V * time256 + (128 << lp)) >> (8 + lp).  stats (a dict) counts destinations that two or more sources
    with different samples reach ("collide") and destinations nobody reaches ("hole")."""
    Y, X, _ = _grid(h, w, pel, off)
    src = take(fin, Y, X).astype(np.int64)
    win = shift_winners(v, t, pel, w, h)
    out = np.full((h, w), (1 << bits) - 1, np.int64)
    has = win > 0
    out[has] = src.reshape(-1)[win[has] - 1]
    if stats is not None:
        dy, dx, inside = shift_targets(v, t, pel, w, h)
        d = (dy * w + dx)[inside]
        lo, hi = np.full(h * w, 1 << 20, np.int64), np.full(h * w, -1, np.int64)
        np.minimum.at(lo, d, src[inside])
        np.maximum.at(hi, d, src[inside])
        stats["collide"] = stats.get("collide", 0) + int(np.count_nonzero((hi >= 0) & (hi != lo)))
        stats["hole"] = stats.get("hole", 0) + int(np.count_nonzero(~has))
    return out.astype(dtype)


def shift_loop(src, vx, vy, t, pel, bits):
    """MVFlow.cpp:119-148 transcribed line by line (Python loops, for small planes): src = the integer-pel samples Finest[h << lp][w << lp]"""
    h, w = src.shape
    nPelLog = {1: 0, 2: 1, 4: 2}[pel]
    rounding, shift_ = 128 << nPelLog, 8 + nPelLog
    dst = [[(1 << bits) - 1] * w for _ in range(h)]
    for hh in range(h):
        for ww in range(w):
            x = (-int(vx[hh, ww]) * t + rounding) >> shift_
            y = (-int(vy[hh, ww]) * t + rounding) >> shift_
            href, wref = hh + y, ww + x
            if 0 <= href < h and 0 <= wref < w:
                dst[href][wref] = int(src[hh, ww])
    return np.array(dst, np.int64)


def blur(fin, off, vb, vf, blur256, prec, pel, w, h, dtype, stats=None, probe=None):
    """MVFlowBlur.c:72-130 RealFlowBlur over one plane (fin = the Finest plane of frame n): per sample and for F then B, m = (max(|vx0|, |vy0|)
    / prec) >> 8 with v0 = V * blur256; if m > 0, v0 /= m (truncating) and m taps at ((i + 1) * v0) >> 8; the mean of the sample and the
    taps.  stats counts samples with taps ("taps"), samples without ("notaps") and negative v0 with a remainder ("trunc").  probe (a dict)
    keeps the largest sum of a sample and its taps ("max_sum") and the largest divisor ("max_count")."""
    Y, X, _ = _grid(h, w, pel, off)
    total = take(fin, Y, X).astype(np.int64)
    count = np.ones((h, w), np.int64)
    for v in (vf, vb):
        vx0 = v[0][:h, :w].astype(np.int64) * blur256
        vy0 = v[1][:h, :w].astype(np.int64) * blur256
        m = (np.maximum(np.abs(vx0), np.abs(vy0)) // prec) >> 8          # non-negative operands
        mm = np.maximum(m, 1)
        if stats is not None:
            trunc = (m > 0) & (((vx0 < 0) & (vx0 % mm != 0)) | ((vy0 < 0) & (vy0 % mm != 0)))
            stats["trunc"] = stats.get("trunc", 0) + int(np.count_nonzero(trunc))
        vx0, vy0 = np.where(m > 0, cdiv(vx0, mm), vx0), np.where(m > 0, cdiv(vy0, mm), vy0)
        ax, ay = vx0.copy(), vy0.copy()
        for i in range(int(m.max()) if m.size else 0):
            live = i < m
            total += np.where(live, take(fin, np.where(live, Y + (ay >> 8), 0), np.where(live, X + (ax >> 8), 0)), 0)
            ax += vx0
            ay += vy0
        count += m
    if stats is not None:
        stats["taps"] = stats.get("taps", 0) + int(np.count_nonzero(count > 1))
        stats["notaps"] = stats.get("notaps", 0) + int(np.count_nonzero(count == 1))
    if probe is not None:
        probe["max_sum"], probe["max_count"] = max(probe.get("max_sum", 0), int(total.max())), max(probe.get("max_count", 0), int(count.max()))
    return (total // count).astype(dtype)                               # non-negative operands


class _Base:
    def _init(self, ad, num_frames, nplanes, hpad, vpad, bits, thscd1, thscd2):
        self.ad = mvoracle.AnalysisData.from_buffer_copy(bytes(ad))
        self.in_frames, self.nplanes, self.hpad, self.vpad, self.bits = num_frames, nplanes, hpad, vpad, bits
        s1, s2 = C.c_int64(thscd1), C.c_int(thscd2)
        _lib().mvo_scale_thscd(C.byref(s1), C.byref(s2), C.byref(self.ad))   # MVAnalysisData.c:7-31
        self.thscd1, self.thscd2 = s1.value, s2.value
        self.delta = self.ad.nDeltaFrame

    def usable(self, blob, ad):
        b = np.ascontiguousarray(np.asarray(blob, np.uint8))
        return bool(_lib().mvo_blob_is_usable(C.byref(ad), C.c_void_p(b.ctypes.data), self.thscd1, self.thscd2))

    def _planes(self, p):
        a = self.ad
        xr, yr = (a.xRatioUV, a.yRatioUV) if p else (1, 1)
        off = ((self.vpad // yr) * a.nPel, (self.hpad // xr) * a.nPel)     # nOffsetY / nOffsetUV, MVFlow.cpp:306-307
        return xr, yr, a.nWidth // xr, a.nHeight // yr, off


class Flow(_Base):
    """One Flow filter over vector clip analysis data ad (time is a double argument, MVFlow.cpp:434)."""

    def __init__(self, ad, num_frames, nplanes, hpad, vpad, bits, time=100.0, mode=0, thscd1=400, thscd2=130):
        self._init(ad, num_frames, nplanes, hpad, vpad, bits, thscd1, thscd2)
        self.mode = mode
        self.time256 = int(float(time) * 256.0 / 100.0)
        a = self.ad
        self.isb = a.isBackward
        step = (a.nBlkSizeX - a.nOverlapX, a.nBlkSizeY - a.nOverlapY)        # MVFlow.cpp:535-546
        self.XP, self.YP = a.nBlkX, a.nBlkY
        while self.XP * step[0] + a.nOverlapX < a.nWidth:
            self.XP += 1
        while self.YP * step[1] + a.nOverlapY < a.nHeight:
            self.YP += 1
        self.wP, self.hP = self.XP * step[0] + a.nOverlapX, self.YP * step[1] + a.nOverlapY

    def ref(self, n):
        """MVFlow.cpp:170-176"""
        d = self.delta
        return (n + d if self.isb else n - d) if d > 0 else -d

    def frame(self, n, clip, finest, blob, field_shift=0, stats=None):
        """clip: input frames; finest: callable k -> the Finest frame of k; blob: the vectors at n (None = copy).  Sets last_kind:
        "copy" (unusable vectors or no reference frame), "fetch" or "shift"."""
        nref = self.ref(n)
        self.last_kind = "copy"
        if blob is None or not (0 <= nref < self.in_frames) or not self.usable(blob, self.ad):   # :364-368
            return [p.copy() for p in clip[n][:self.nplanes]]
        self.last_kind = "shift" if self.mode else "fetch"
        a = self.ad
        vx, vy = pl.blob_vectors(blob, a)[:2]
        VX, VY = small_fields(vx, vy, self.XP, self.YP)
        VY = (VY.astype(np.int64) + field_shift).astype(np.int16)                              # :296-300
        fin = finest(nref)
        out = []
        for p in range(self.nplanes):
            xr, yr, lw, lh, off = self._planes(p)
            sx, sy = (half_uv(VX, xr), half_uv(VY, yr)) if p else (VX, VY)                    # :322-323
            dw, dh = self.wP // xr, self.hP // yr
            v = (upsize_i16(sx, dw, dh, lw, lh, a.nPel, True), upsize_i16(sy, dw, dh, lw, lh, a.nPel, False))
            if self.mode:
                out.append(shift(fin[p], off, v, self.time256, a.nPel, lw, lh, self.bits, clip[n][p].dtype, stats))
            else:
                out.append(fetch(fin[p], off, v, self.time256, a.nPel, lw, lh, clip[n][p].dtype))
        return out


class FlowBlur(_Base):
    """One FlowBlur filter over analysis data ad_bw / ad_fw (blur is a float argument, MVFlowBlur.c:354,385)."""

    def __init__(self, ad_bw, ad_fw, num_frames, nplanes, hpad, vpad, bits, blur=50.0, prec=1, thscd1=400, thscd2=130):
        self._init(ad_bw, num_frames, nplanes, hpad, vpad, bits, thscd1, thscd2)
        self.fw = mvoracle.AnalysisData.from_buffer_copy(bytes(ad_fw))
        self.prec = prec
        self.blur256 = int(np.float32(blur) * np.float32(256.0) / np.float32(200.0))

    def frame(self, n, clip, finest, blobs_bw, blobs_fw, stats=None, probe=None):
        """blobs_*: per input frame blobs of the two vector clips.  Sets last_kind "copy" or "blur".  probe: see blur."""
        d = self.delta
        self.last_kind = "copy"
        ok = n - d >= 0 and n + d < self.in_frames                                                  # :158-178
        ok = ok and self.usable(blobs_fw[n + d], self.fw) and self.usable(blobs_bw[n - d], self.ad)
        if not ok:
            return [p.copy() for p in clip[n][:self.nplanes]]
        self.last_kind = "blur"
        a = self.ad
        vb, vf = pl.blob_vectors(blobs_bw[n - d], a), pl.blob_vectors(blobs_fw[n + d], self.fw)
        small = [(x.astype(np.int16), y.astype(np.int16)) for x, y in (vb[:2], vf[:2])]            # :217-218, no padding
        fin = finest(n)
        out = []
        for p in range(self.nplanes):
            xr, yr, lw, lh, off = self._planes(p)
            full = []
            for sx, sy in small:
                if p:
                    sx, sy = half_uv(sx, xr), half_uv(sy, yr)                                      # :251-257
                full.append((upsize_i16(sx, lw, lh, lw, lh, a.nPel, True), upsize_i16(sy, lw, lh, lw, lh, a.nPel, False)))
            out.append(blur(fin[p], off, full[0], full[1], self.blur256, self.prec, a.nPel, lw, lh, clip[n][p].dtype, stats, probe))
        return out
