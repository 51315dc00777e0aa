"""CPU restatement of mv.FlowInter and mv.FlowFPS (test infrastructure; the GPU parity tests compare the HIP path against it).

It follows the reference literally: full-resolution int16 vector planes and byte masks per output frame, the three interpolation
formulas over the Finest frame that mvoracle.Super.finest builds (so a match also proves that the GPU path's direct addressing of the
super frame's sub-pel planes is right), and the Blend / copy fallbacks.  Citations are to dubhater/vapoursynth-mvtools src/:
  FlowInter   MVFlowInter.c:80-452 (frame), :473-678 (creation)
  FlowFPS     MVFlowFPS.c:86-524 (frame), :565-802 (creation); FlowFPSHelper MVFlowFPSHelper.c:49-93
  fields      MaskFun.cpp:38-60 CheckAndPadSmallY, :63-80 CheckAndPadMaskSmall, :86-130 MakeVectorOcclusionMaskTime,
              :169-181 MakeVectorSmallMasks, :183-203 VectorSmallMaskYToHalfUV
  formulas    MaskFun.cpp:349-371 Blend, :374-414 FlowInter, :417-490 FlowInterExtra, :493-551 FlowInterSimple
  upsizers    SimpleResize.cpp:27-57 InitTables, :60-121 simpleResize (int16 form here; the u8 form and the tables are the oracle's,
              mvo_simple_resize_u8 / mvo_resize_tables)

The reference's default opt=1 runs SimpleResize_AVX2.cpp and MaskFun_AVX2.cpp.  The int16 resizer here is pinned against that AVX2 object
code (tests/test_flow_ref.py) at nBlkXP >= 8 (below 8 small-field columns the AVX2 form reads before its buffers).  MaskFun_AVX2.cpp
computes the same integers as the C templates on every input the kernels can see.  It holds samples, masks and vectors in 32-bit lanes
(cvtepu8_epi32 / cvtepi16_epi32).  In the 8-bit forms the sample x mask products (at most 255 * 255 = 65025) are formed with mullo_epi16: the
lane's high half is 0 * 0 and its low half keeps all 16 bits of a product below 2^16, so the 32-bit lane holds the exact product.  FlowInter's
third factor (a mask times a sum of at most 255 * 255) is a mullo_epi32 (below 2^24), Simple's time256 == 128 term a madd_epi16 of
(dB - dF, mF - mB) pairs.  In the 16-bit forms every product is a mullo_epi32 below 2^24, except FlowInter's mask x (sum of at most
65535 * 255), which is a mul_epu32 into 64-bit lanes, exact like the C template's int64.  The vector scaling is a madd_epi16 by time256
(products below 2^31) and srai, the C template's (v * t) >> 8; the addresses are formed in 32 bits as in C.

Integer semantics: C `/` truncates while numpy `//` floors -- every division below has non-negative operands; `>>` on signed values is
arithmetic in both; int16 planes are widened to int64 before any product.
"""
import ctypes as C

import numpy as np

import mvoracle
import pipeline as pl

MAX_SAD = 8 * 8 * 255


def _lib():
    L = mvoracle.lib()
    L.mvo_simple_resize_u8.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_int] * 4
    L.mvo_scale_thscd.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(mvoracle.AnalysisData)]
    return L


def resize_tables(out, inn):
    """SimpleResize.cpp:27-57 InitTables (the oracle's restatement): offsets, weights of the second line / column"""
    o, w = np.zeros(out, np.int32), np.zeros(out, np.int32)
    _lib().mvo_resize_tables(o.ctypes.data, w.ctypes.data, out, inn)
    return o, w


def upsize_u8(small, dw, dh):
    """SimpleResize.cpp:60-121, uint8_t form (no limiting): the oracle's mvo_simple_resize_u8"""
    sh, sw = small.shape
    src = np.zeros((sh + 1, sw + 8), np.uint8)
    src[:sh, :sw] = small
    dst = np.zeros((dh, dw + 8), np.uint8)
    _lib().mvo_simple_resize_u8(dst.ctypes.data, dst.shape[1], src.ctypes.data, src.shape[1], dw, dh, sw, sh)
    return dst[:, :dw].copy()


def upsize_i16_parts(small, dw, dh, limit_w, limit_h, pel, horizontal):
    """SimpleResize.cpp:60-121, int16_t form, before the limiting: (the rounded result, its lower limits, its upper limits)"""
    sh, sw = small.shape
    vo, vw = resize_tables(dh, sh)
    ho, hw = resize_tables(dw, sw)
    s = small.astype(np.int64)
    vw, hw = vw.astype(np.int64), hw.astype(np.int64)
    work = ((s[vo] * (16384 - vw)[:, None] + s[vo + 1] * vw[:, None] + 8192) >> 14).astype(np.int16).astype(np.int64)
    res = (work[:, ho] * (16384 - hw)[None, :] + work[:, ho + 1] * hw[None, :] + 8192) >> 14
    if horizontal:
        x = np.arange(dw, dtype=np.int64)[None, :]
        lo, hi = -x * pel, (limit_w - x) * pel - 1
    else:
        y = np.arange(dh, dtype=np.int64)[:, None]
        lo, hi = -y * pel, (limit_h - y) * pel - 1
    return res, lo, hi


def upsize_i16(small, dw, dh, limit_w, limit_h, pel, horizontal):
    """SimpleResize.cpp:60-121, int16_t form: vertical pass rounded into an int16 work row, horizontal pass rounded, then limited to
    [-x * pel, (limit_w - x) * pel - 1] (horizontal vectors, :99-113) or [-y * pel, (limit_h - y) * pel - 1] (vertical vectors, :117-119)"""
    res, lo, hi = upsize_i16_parts(small, dw, dh, limit_w, limit_h, pel, horizontal)
    return np.maximum(lo, np.minimum(res, hi)).astype(np.int16)


def small_fields(vx, vy, XP, YP):
    """MaskFun.cpp:169-181 MakeVectorSmallMasks into int16 planes of pitch nBlkXP, then :38-60 CheckAndPadSmallY"""
    nby, nbx = vx.shape
    VX, VY = np.zeros((YP, XP), np.int16), np.zeros((YP, XP), np.int16)
    VX[:nby, :nbx] = vx.astype(np.int16)
    VY[:nby, :nbx] = vy.astype(np.int16)
    if XP > nbx:
        VX[:nby, nbx:] = np.minimum(VX[:nby, nbx - 1:nbx], 0)
        VY[:nby, nbx:] = VY[:nby, nbx - 1:nbx]
    if YP > nby:
        VX[nby:, :] = VX[nby - 1:nby, :]
        VY[nby:, :] = np.minimum(VY[nby - 1:nby, :], 0)
    return VX, VY


def half_uv(v, ratio):
    """MaskFun.cpp:183-203 VectorSmallMaskYToHalfUV"""
    return (v >> 1).astype(np.int16) if ratio == 2 else v.copy()


def occlusion_mask(vx, vy, is_backward, ml, pel, XP, YP, time256, stepx, stepy):
    """MaskFun.cpp:86-130 MakeVectorOcclusionMaskTime with fGamma 1, then :63-80 CheckAndPadMaskSmall"""
    nby, nbx = vx.shape
    m = np.zeros((YP, XP), np.int64)
    tx, ty = time256 * 16 // (stepx * pel), time256 * 16 // (stepy * pel)   # non-negative operands
    normx, normy = 80.0 / (ml * stepx * pel), 80.0 / (ml * stepy * pel)
    for by, bx in zip(*np.nonzero(vx[:, 1:] < vx[:, :-1])):                   # right neighbour, bx < nBlkX - 1
        o = int(vx[by, bx]) - int(vx[by, bx + 1])
        minb = max(0, bx + 1 - o * tx // 4096) if is_backward else bx
        maxb = bx + 1 if is_backward else min(bx + 1 - o * tx // 4096, nbx - 1)
        if maxb >= minb:
            m[by, minb:maxb + 1] = np.maximum(m[by, minb:maxb + 1], min(int(255 * o * normx), 255))
    for by, bx in zip(*np.nonzero(vy[1:, :] < vy[:-1, :])):                   # bottom neighbour, by < nBlkY - 1
        o = int(vy[by, bx]) - int(vy[by + 1, bx])
        minb = max(0, by + 1 - o * ty // 4096) if is_backward else by
        maxb = by + 1 if is_backward else min(by + 1 - o * ty // 4096, nby - 1)
        if maxb >= minb:
            m[minb:maxb + 1, bx] = np.maximum(m[minb:maxb + 1, bx], min(int(255 * o * normy), 255))
    m = m.astype(np.uint8)
    if XP > nbx:
        m[:nby, nbx:] = m[:nby, nbx - 1:nbx]
    if YP > nby:
        m[nby:, :] = m[nby - 1:nby, :]
    return m


def blend(l, r, t, dtype):
    """MaskFun.cpp:349-371 Blend"""
    return ((l.astype(np.int64) * (256 - t) + r.astype(np.int64) * t) >> 8).astype(dtype)


def take(fin, rows, cols):
    """fin[rows, cols] after checking that every index lies inside the plane: numpy wraps negative indices silently, which would let this
    restatement agree with a kernel that reads the wrong sample (the reference would read outside its frame there)"""
    rows, cols = np.broadcast_arrays(rows, cols)
    assert rows.min() >= 0 and rows.max() < fin.shape[0] and cols.min() >= 0 and cols.max() < fin.shape[1], (
        "fetch outside the Finest plane", int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max()), fin.shape)
    return fin[rows, cols]


def flow_inter(kind, t, fin_b, fin_f, off, pel, vb, vf, mb, mf, w, h, dtype, vbb=None, vff=None, probe=None):
    """kind 'simple' / 'regular' / 'extra': MaskFun.cpp:493-551 / :374-414 / :417-490 over one plane.  fin_b = the right Finest plane
    (prefB), fin_f = the left one (prefF); off = (row, column) of the unpadded sample (0, 0) in them; v* = (VX, VY) full planes.
    probe (a dict of lists) collects intermediates for the tests that show what a case reaches: the fetched samples "dF" / "dB", the
    masks "MF" / "MB" and, for 'regular', the two inner products "inner" (int64: what a 32-bit kernel must hold without wrapping)."""
    lp = {1: 0, 2: 1, 4: 2}[pel]
    Y = (np.arange(h, dtype=np.int64) << lp)[:, None] + off[0]
    X = (np.arange(w, dtype=np.int64) << lp)[None, :] + off[1]
    cut = lambda a: a[:h, :w].astype(np.int64)
    MF, MB = cut(mf), cut(mb)

    def fetch(fin, v, tt):
        return take(fin, Y + ((cut(v[1]) * tt) >> 8), X + ((cut(v[0]) * tt) >> 8)).astype(np.int64)

    dF, dB = fetch(fin_f, vf, t), fetch(fin_b, vb, 256 - t)
    if probe is not None:
        for k, v in (("dF", dF), ("dB", dB), ("MF", MF), ("MB", MB)):
            probe.setdefault(k, []).append(v)
    if kind == "simple":
        if t == 128:
            out = (((dF + dB) << 8) + (dB - dF) * (MF - MB)) >> 9
        else:
            out = ((((dF * (255 - MF) + dB * MF + 255) >> 8) * (256 - t) + ((dB * (255 - MB) + dF * MB + 255) >> 8) * t) >> 8)
    elif kind == "regular":
        dF0, dB0 = take(fin_f, Y, X).astype(np.int64), take(fin_b, Y, X).astype(np.int64)
        inner_a, inner_b = MF * (dB * (255 - MB) + MB * dF0) + 255, MB * (dF * (255 - MF) + MF * dB0) + 255
        a = (dF * (255 - MF) + (inner_a >> 8) + 255) >> 8
        b = (dB * (255 - MB) + (inner_b >> 8) + 255) >> 8
        if probe is not None:
            probe.setdefault("inner", []).extend([inner_a, inner_b])
        out = (a * (256 - t) + b * t) >> 8
    else:
        dFF, dBB = fetch(fin_f, vff, t), fetch(fin_b, vbb, 256 - t)
        mn, mx = np.minimum(dB, dF), np.maximum(dB, dF)
        medBB, medFF = np.maximum(mn, np.minimum(dBB, mx)), np.maximum(mn, np.minimum(dFF, mx))
        out = (((medBB * MF + dF * (255 - MF) + 255) >> 8) * (256 - t) + ((medFF * MB + dB * (255 - MB) + 255) >> 8) * t) >> 8
    return out.astype(dtype)


class Flow:
    """One FlowInter (fps=None) or FlowFPS filter over analysis data ad_bw / ad_fw (ctypes structures with the reference's fields)."""

    def __init__(self, ad_bw, ad_fw, num_frames, nplanes, hpad, vpad, fps=None, time=50.0, num=None, den=None, mask=2, ml=100.0, blend=1,
                 thscd1=400, thscd2=130):
        self.bw, self.fw = mvoracle.AnalysisData.from_buffer_copy(bytes(ad_bw)), mvoracle.AnalysisData.from_buffer_copy(bytes(ad_fw))
        self.in_frames, self.nplanes, self.blend, self.is_fps, self.mask = num_frames, nplanes, 1 if blend else 0, fps is not None, mask
        self.hpad, self.vpad = hpad, vpad
        s1, s2 = C.c_int64(thscd1), C.c_int(thscd2)
        _lib().mvo_scale_thscd(C.byref(s1), C.byref(s2), C.byref(self.bw))   # MVAnalysisData.c:7-31
        self.thscd1, self.thscd2 = s1.value, s2.value
        self.delta = self.bw.nDeltaFrame
        if self.is_fps:                                                        # MVFlowFPS.c:714-744
            self.ml = float(ml)
            num = 25 if num is None else num
            den = 1 if den is None else den
            n_, d_ = (num, den) if num != 0 and den != 0 else (fps[0] * 2, fps[1])
            fa, fb = d_ * fps[0], n_ * fps[1]
            g = np.gcd(fa, fb)
            self.fa, self.fb = fa // g, fb // g
            x = np.gcd(n_, d_)
            self.fps = (n_ // x, d_ // x) if n_ > 0 and d_ > 0 else (0, 1)
            self.num_frames = int(1 + (num_frames - 1) * self.fb // self.fa)
        else:                                                                  # MVFlowInter.c:481-516: float arguments
            self.time256 = int(np.float32(time) * np.float32(256.0) / np.float32(100.0))
            self.ml = float(np.float32(ml))
            self.num_frames = num_frames
        a = self.bw
        self.XP, self.YP = a.nBlkX, a.nBlkY
        step = (a.nBlkSizeX - a.nOverlapX, a.nBlkSizeY - a.nOverlapY)
        while self.XP * step[0] + a.nOverlapX < a.nWidth:
            self.XP += 1
        while self.YP * step[1] + a.nOverlapY < a.nHeight:
            self.YP += 1
        self.step = step
        self.wP, self.hP = self.XP * step[0] + a.nOverlapX, self.YP * step[1] + a.nOverlapY

    def map(self, n):
        if not self.is_fps:
            return n, n + self.delta, self.time256
        nleft = int(n * self.fa // self.fb)
        t = int((float(n) * self.fa / self.fb - nleft) * 256 + 0.5)
        if self.delta > 1:
            t = t // self.delta
        return nleft, nleft + self.delta, t

    def _usable(self, blob, ad):
        b = np.ascontiguousarray(np.asarray(blob, np.uint8))
        return bool(_lib().mvo_blob_is_usable(C.byref(ad), C.c_void_p(b.ctypes.data), self.thscd1, self.thscd2))

    def frame(self, n, clip, finest, blobs_bw, blobs_fw, probe=None):
        """clip: input frames (lists of numpy planes); finest: Finest frames (mvoracle.Super.finest) per input frame, or a callable
        n -> Finest frame; blobs_*: per input frame blobs of the two vector clips.  Sets last_kind: "copy", "blend", "left", or the
        formula "simple" / "regular" / "extra", with "128" appended at time256 128.  probe: see flow_inter."""
        nl, nr, t = self.map(n)
        last = self.in_frames - 1
        L, R = clip[min(nl, last)], clip[min(nr, last)]
        dtype = L[0].dtype
        self.last_kind = "copy"
        if self.is_fps and t == 0:
            return [p.copy() for p in L[:self.nplanes]]
        if self.is_fps and t == 256:
            return [p.copy() for p in R[:self.nplanes]]
        ok = nl < self.in_frames and nr < self.in_frames
        ok = ok and self._usable(blobs_fw[nr], self.fw) and self._usable(blobs_bw[nl], self.bw)
        if not ok:
            self.last_kind = "blend" if self.blend else "left"
            if not self.blend:
                return [p.copy() for p in L[:self.nplanes]]
            return [blend(L[p], R[p], t, dtype) for p in range(self.nplanes)]
        a = self.bw
        vb = pl.blob_vectors(blobs_bw[nl], a)
        vf = pl.blob_vectors(blobs_fw[nr], self.fw)
        want_extra = not self.is_fps or self.mask == 2
        extra = want_extra and self._usable(blobs_fw[nl], self.fw) and self._usable(blobs_bw[nr], self.bw)
        if not self.is_fps:
            kind = "extra" if extra else "regular"
        else:
            kind = "regular" if self.mask == 1 else ("extra" if extra else "simple")
        self.last_kind = kind + ("128" if t == 128 else "")
        get = finest if callable(finest) else (lambda k: finest[k])
        finL, finR = get(nl), get(nr)
        SB, SF = small_fields(vb[0], vb[1], self.XP, self.YP), small_fields(vf[0], vf[1], self.XP, self.YP)
        MB = occlusion_mask(vb[0], vb[1], 1, self.ml, a.nPel, self.XP, self.YP, 256 - t, *self.step)
        MF = occlusion_mask(vf[0], vf[1], 0, self.ml, a.nPel, self.XP, self.YP, t, *self.step)
        SBB = SFF = None
        if kind == "extra":
            vbb, vff = pl.blob_vectors(blobs_bw[nr], a), pl.blob_vectors(blobs_fw[nl], self.fw)
            SBB, SFF = small_fields(vbb[0], vbb[1], self.XP, self.YP), small_fields(vff[0], vff[1], self.XP, self.YP)
        out = []
        for p in range(self.nplanes):
            xr, yr = (a.xRatioUV, a.yRatioUV) if p else (1, 1)
            dw, dh = self.wP // xr, self.hP // yr
            lw, lh = a.nWidth // xr, a.nHeight // yr

            def full(S):
                if S is None:
                    return None
                vx, vy = (half_uv(S[0], xr), half_uv(S[1], yr)) if p else S
                return (upsize_i16(vx, dw, dh, lw, lh, a.nPel, True), upsize_i16(vy, dw, dh, lw, lh, a.nPel, False))

            off = ((self.vpad // yr) * a.nPel, (self.hpad // xr) * a.nPel)     # nOffsetY / nOffsetUV, MVFlowInter.c:218-219
            out.append(flow_inter(kind, t, finR[p], finL[p], off, a.nPel, full(SB), full(SF), upsize_u8(MB, dw, dh), upsize_u8(MF, dw, dh),
                                  lw, lh, dtype, full(SBB), full(SFF), probe))
        return out
