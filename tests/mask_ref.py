"""CPU restatement of mv.Mask (test infrastructure; the GPU parity tests compare the HIP path, mvx_mask.hip, against it).

It follows the reference literally.  Citations are to dubhater/vapoursynth-mvtools src/:
  creation    MVMask.c:227-346 (argument rounding :235-241, factors :304-307, geometry :309-315, time256 :334)
  frame       MVMask.c:75-211; mvmaskLength :66-72
  masks       MaskFun.cpp:85-90 ByteOccMask, :92-132 MakeVectorOcclusionMaskTime, :135-139 ByteNorm, :142-166 MakeSADMaskTime
  upsizer     SimpleResize.cpp:27-121, uint8_t form: the oracle's mvo_simple_resize_u8 through flow_ref.upsize_u8, which oracle/ pins to
              the reference's AVX2 object code

Number formats: ml and gamma are float arguments, and fMaskNormFactor, fMaskNormFactor2 and fHalfGamma are floats formed from them
(np.float32 here); time is a double argument.  pow is the C library's double pow (math.pow).  Kinds 3-5 are float expressions, evaluated
left to right in np.float32.  C `/` truncates while Python `//` floors: cdiv() is used wherever an operand can be negative.

The one place where this file states the library and not the reference: where 255 * pow(...) of the occlusion mask exceeds the int range,
the reference's cast is undefined (x86: INT_MIN, the cell keeps its value); the library saturates the cell to 255, and so does occ_value().

Counters (stats) name what a frame exercised:
  moved  a kind 1 block that took another block's SAD          back   a kind 1 block whose source fell outside the grid and fell back
  cut    a value cut at 255                                    span   an occlusion range that covers more than two blocks
  edgex / edgey  samples taken by the right / bottom edge replication   sc  an unusable frame filled with ysc
  trunc  a negative product with a remainder in a truncating division
pow_dist is the condition the GPU cases must meet (see pow_distance): the smallest distance of any 255 * pow(...) whose exponent is not 1
and whose result is not exact by construction to the integer it must not cross.
"""
import ctypes as C
import math

import numpy as np

import flow_ref
import mvoracle
import pipeline as pl


def cdiv(a, b):
    """C's truncating integer division"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def c_pow(b, e):
    """glibc's pow; an overflowing result is +inf as in C"""
    try:
        return math.pow(b, e)
    except OverflowError:
        return math.inf


def pow_distance(l, base, exponent):
    """the distance that decides whether another pow, a few ULP off, could give another byte: None where the result is exact by construction
    (exponent 1: no pow on the device; base 0 or exponent 0: pow is exactly 0 or 1), else the distance of l to the nearest integer while
    l <= 255, and to 255 above it (a value just above 255 is cut to 255, just below it is 254)"""
    if exponent == 1.0 or base == 0.0 or exponent == 0.0:
        return None
    return abs(l - round(l)) if l <= 255 else l - 255


class Mask:
    """One mv.Mask filter over analysis data ad (a ctypes structure with the reference's fields).  The clip has the vector clip's size
    and chroma ratios (the library rejects any other)."""

    def __init__(self, ad, ml=100.0, gamma=1.0, kind=0, time=100.0, ysc=0, thscd1=400, thscd2=130):
        self.ad = a = mvoracle.AnalysisData.from_buffer_copy(bytes(ad))
        f32 = np.float32
        self.ml, self.fGamma = f32(ml), f32(gamma)                                # MVMask.c:235-241
        self.kind, self.ysc = kind, ysc
        s1, s2 = C.c_int64(thscd1), C.c_int(thscd2)
        flow_ref._lib().mvo_scale_thscd(C.byref(s1), C.byref(s2), C.byref(a))    # MVAnalysisData.c:7-31
        self.thscd1, self.thscd2 = s1.value, s2.value
        self.fMaskNormFactor = f32(1.0) / self.ml                                  # MVMask.c:304-307
        self.fMaskNormFactor2 = self.fMaskNormFactor * self.fMaskNormFactor
        self.fHalfGamma = self.fGamma * f32(0.5)
        assert all(isinstance(v, np.float32) for v in (self.fMaskNormFactor, self.fMaskNormFactor2, self.fHalfGamma))
        self.step = (a.nBlkSizeX - a.nOverlapX, a.nBlkSizeY - a.nOverlapY)
        self.wB, self.hB = a.nBlkX * self.step[0] + a.nOverlapX, a.nBlkY * self.step[1] + a.nOverlapY   # MVMask.c:309-310
        self.wUV, self.hUV = a.nWidth // a.xRatioUV, a.nHeight // a.yRatioUV     # :312-315
        self.wBUV, self.hBUV = self.wB // a.xRatioUV, self.hB // a.yRatioUV
        self.time256 = int(time * 256 / 100)                                      # :334, in double
        self.pow_dist = math.inf

    # ---------------------------------------------------------------- the small masks

    def _note(self, l, base, exponent):
        d = pow_distance(l, base, exponent)
        if d is not None:
            self.pow_dist = min(self.pow_dist, d)

    def length_mask(self, vx, vy, stats):
        """MVMask.c:139-141 with mvmaskLength :66-72"""
        pel, f2, hg = self.ad.nPel, float(self.fMaskNormFactor2), float(self.fHalfGamma)
        out = np.zeros(vx.shape, np.uint8)
        for idx in np.ndindex(vx.shape):
            x, y = int(vx[idx]), int(vy[idx])
            n2 = x * x + y * y
            assert n2 < 2 ** 31, "the reference's int sum would overflow"
            norme = float(n2) / (pel * pel)
            base = norme * f2
            l = 255 * c_pow(base, hg)
            self._note(l, base, hg)
            if l > 255:
                stats["cut"] = stats.get("cut", 0) + 1
            out[idx] = int(255 if l > 255 else l)
        return out

    def sad_mask(self, vx, vy, sad, stats):
        """MakeSADMaskTime, MaskFun.cpp:142-166, as MVMask.c:143 calls it: bitsPerSample is the 8-bit mask clip's, so the SAD is not shifted"""
        a = self.ad
        nby, nbx = vx.shape
        factor = 4.0 * float(self.fMaskNormFactor) / (a.nBlkSizeX * a.nBlkSizeY)
        g = float(self.fGamma)
        tx = (256 - self.time256) * 16 // (self.step[0] * a.nPel)                 # non-negative operands
        ty = (256 - self.time256) * 16 // (self.step[1] * a.nPel)
        out = np.zeros((nby, nbx), np.uint8)
        for by in range(nby):
            for bx in range(nbx):
                px, py = int(vx[by, bx]) * tx, int(vy[by, bx]) * ty
                if (px < 0 and px % 4096) or (py < 0 and py % 4096):
                    stats["trunc"] = stats.get("trunc", 0) + 1
                bxi, byi = bx - cdiv(px, 4096), by - cdiv(py, 4096)
                if bxi < 0 or bxi >= nbx or byi < 0 or byi >= nby:
                    bxi, byi = bx, by
                    stats["back"] = stats.get("back", 0) + 1
                elif (bxi, byi) != (bx, by):
                    stats["moved"] = stats.get("moved", 0) + 1
                s = int(sad[byi, bxi]) >> (8 - 8)
                base = s * factor
                l = 255 * c_pow(base, g)                                          # ByteNorm, :135-139
                self._note(l, base, g)
                if l > 255:
                    stats["cut"] = stats.get("cut", 0) + 1
                out[by, bx] = int(255 if l > 255 else l)
        return out

    def occ_value(self, o, norm, stats):
        """ByteOccMask's new value, MaskFun.cpp:85-90"""
        g = float(self.fGamma)
        if g == 1.0:
            l = 255 * o * norm
        else:
            base = o * norm
            l = 255 * c_pow(base, g)
            self._note(l, base, g)
        if l >= 255:
            stats["cut"] = stats.get("cut", 0) + 1
        return 255 if l >= 2.0 ** 31 else min(int(l), 255)                        # beyond int: the library saturates (see the module text)

    def occlusion_mask(self, vx, vy, stats):
        """MakeVectorOcclusionMaskTime, MaskFun.cpp:92-132, as MVMask.c:145 calls it"""
        a = self.ad
        nby, nbx = vx.shape
        back = a.isBackward
        divider = 1.0 / float(self.fMaskNormFactor)
        tx, ty = self.time256 * 16 // (self.step[0] * a.nPel), self.time256 * 16 // (self.step[1] * a.nPel)
        normx, normy = 80.0 / (divider * self.step[0] * a.nPel), 80.0 / (divider * self.step[1] * a.nPel)
        m = np.zeros((nby, nbx), np.int64)

        def span(lo, hi):
            if hi - lo + 1 > 2:
                stats["span"] = stats.get("span", 0) + 1

        for by, bx in zip(*np.nonzero(vx[:, 1:] < vx[:, :-1])):                   # right neighbour, bx < nBlkX - 1
            o = int(vx[by, bx]) - int(vx[by, bx + 1])                             # positive, so o * tx / 4096 has no negative operand
            minb = max(0, bx + 1 - o * tx // 4096) if back else bx
            maxb = bx + 1 if back else min(bx + 1 - o * tx // 4096, nbx - 1)
            if maxb >= minb:
                span(minb, maxb)
                m[by, minb:maxb + 1] = np.maximum(m[by, minb:maxb + 1], self.occ_value(o, normx, stats))
        for by, bx in zip(*np.nonzero(vy[1:, :] < vy[:-1, :])):                   # bottom neighbour, by < nBlkY - 1
            o = int(vy[by, bx]) - int(vy[by + 1, bx])
            minb = max(0, by + 1 - o * ty // 4096) if back else by
            maxb = by + 1 if back else min(by + 1 - o * ty // 4096, nby - 1)
            if maxb >= minb:
                span(minb, maxb)
                m[minb:maxb + 1, bx] = np.maximum(m[minb:maxb + 1, bx], self.occ_value(o, normy, stats))
        return m.astype(np.uint8)

    def component_mask(self, v, stats):
        """MVMask.c:148,151,155-156: max(0, min(255, (int)(v * fMaskNormFactor * 100 + 128))) in float, left to right"""
        f32 = np.float32
        val = (v.astype(np.float32) * self.fMaskNormFactor) * f32(100) + f32(128)
        assert val.dtype == np.float32
        i = val.astype(np.int64)                                                   # C's conversion truncates; so does astype
        if np.any(i > 255):
            stats["cut"] = stats.get("cut", 0) + int(np.count_nonzero(i > 255))
        return np.clip(i, 0, 255).astype(np.uint8)

    def small_masks(self, blob, stats):
        """the nBlkX x nBlkY byte masks of one usable frame, MVMask.c:139-158: (smallMask, smallMaskV); smallMaskV is None except for kind 5"""
        vx, vy, sad = pl.blob_vectors(blob, self.ad)
        k = self.kind
        if k == 0:
            return self.length_mask(vx, vy, stats), None
        if k == 1:
            return self.sad_mask(vx, vy, sad, stats), None
        if k == 2:
            return self.occlusion_mask(vx, vy, stats), None
        if k == 3:
            return self.component_mask(vx, stats), None
        if k == 4:
            return self.component_mask(vy, stats), None
        return self.component_mask(vx, stats), self.component_mask(vy, stats)

    # ---------------------------------------------------------------- planes

    def plane(self, small, wb, hb, w, h, stats):
        """MVMask.c:163-169 / :173-189: the upsized mask in the covered rectangle, then every row's right fill from column wb - 1, then the rows
        below from row hb - 1 (row by row, so every one of them equals it)"""
        out = np.zeros((h, w), np.uint8)
        out[:hb, :wb] = flow_ref.upsize_u8(small, wb, hb)
        if w > wb:
            out[:hb, wb:] = out[:hb, wb - 1:wb]
            stats["edgex"] = stats.get("edgex", 0) + (w - wb) * hb
        if h > hb:
            out[hb:, :] = out[hb - 1:hb, :]
            stats["edgey"] = stats.get("edgey", 0) + (h - hb) * w
        return out

    def usable(self, blob):
        if blob is None:
            return False
        b = np.ascontiguousarray(np.asarray(blob, np.uint8))
        return bool(flow_ref._lib().mvo_blob_is_usable(C.byref(self.ad), C.c_void_p(b.ctypes.data), self.thscd1, self.thscd2))

    def frame(self, blob, clip_luma=None, stats=None):
        """the three output planes of one frame; blob None = no vectors (unusable); clip_luma: the clip's luma plane (kind 5)"""
        a = self.ad
        stats = {} if stats is None else stats
        w, h = a.nWidth, a.nHeight
        luma = np.array(clip_luma[:h, :w], np.uint8) if self.kind == 5 else None
        if not self.usable(blob):                                                  # MVMask.c:193-201
            stats["sc"] = stats.get("sc", 0) + 1
            fill = lambda hh, ww: np.full((hh, ww), self.ysc, np.uint8)
            return [luma if self.kind == 5 else fill(h, w), fill(self.hUV, self.wUV), fill(self.hUV, self.wUV)]
        small, small_v = self.small_masks(blob, stats)
        if self.kind != 5:
            luma = self.plane(small, self.wB, self.hB, w, h, stats)
        u = self.plane(small, self.wBUV, self.hBUV, self.wUV, self.hUV, stats)
        v = self.plane(small_v, self.wBUV, self.hBUV, self.wUV, self.hUV, stats) if self.kind == 5 else u.copy()
        return [luma, u, v]
