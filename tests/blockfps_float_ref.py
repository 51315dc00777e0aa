"""Numpy float32 restatement of BlockFPS on a float clip (mvx_blockfps_create_float), test infrastructure: written from the description in
include/mvtools_amd.h, not from the kernel.  tests/test_blockfps_float_ref.py anchors it to oracle.BlockFPS on integer-valued frames.

Control (the integer filter's, MVBlockFPS.c:229-676), none of which sees a sample:
    usable        both super frames and both blobs are there, 0 < time256 < 256, both blobs are valid and neither has more than nSCD2 level-0
                  blocks with a SAD above nSCD1
    plan          block (bx, by) sits at x = bx * stepX, y = by * stepY (luma).  b is fetched from the RIGHT super frame at
                  (x * pel + ((vB.x * (256 - t)) >> 8)) / xRatio, fw from the LEFT one at (x * pel + ((vF.x * t) >> 8)) / xRatio -- C's division
                  by the subsampling ratio, towards zero, not a shift -- and likewise in y; mvpGetPointer picks the sub-pel plane
    masks         modes 3..5: MakeVectorOcclusionMaskTime of mvfw at time t (forward) and of mvbw at 256 - t (backward); modes 6..8:
                  MakeSADMaskTime with the SADs >> (bitsPerSample of the search - 8) and factor 4 / (ml * blkSizeX * blkSizeY); then the right /
                  bottom clone padding to the padded grid, O = F * B / 255 on the padded small masks, and the 8-bit SimpleResize to the padded
                  frame size, luma and chroma
    interior      the left / right frame at the output position is the super plane at hpad, vpad (luma) and at hpad >> 1, vpad >> 1 (chroma,
                  whatever the subsampling: the reference's offsets, MVBlockFPS.c:455-464)

The float sample: the table of include/mvtools_amd.h (mvx_blockfps_create_float), np.float32 operation by operation.

Super frames are given as arrays of level 0: per plane the pel * pel sub-pel planes stacked, as tests/degrain_float_ref.py takes them."""
import numpy as np

import degrain_n_ref
import flow_ref
import pipeline as pl

F = np.float32
K = F(0.00390625)


# ------------------------------------------------------------------------------------------------ the per-sample rule

def fmin(a, b):
    return np.where(a < b, a, b)


def fmax(a, b):
    return np.where(a > b, a, b)


def med(a, b, c):
    return fmax(fmin(a, b), fmin(fmax(a, b), c))


def time_(right, left, t):
    """(right * ft + left * fu) * K"""
    r = (right * F(t) + left * F(256 - t)) * K
    assert r.dtype == F
    return r


def mix(m, p, q):
    """((float)m * p + (float)(255 - m) * q) / 255, m an integer array 0..255"""
    m = np.asarray(m, np.int64)
    r = (m.astype(F) * p + (255 - m).astype(F) * q) / F(255.0)
    assert r.dtype == F
    return r


def value(mode, t, s, r, b, fw, mF, mB, mO):
    """one sample of a block, all arguments arrays of one shape (s, r, b, fw float32; the masks integers)"""
    if mode == 0:
        return time_(b, fw, t)
    if mode == 1:
        return med(r, s, time_(b, fw, t))
    if mode == 2:
        return med(time_(r, s, t), b, fw)
    if mode in (3, 6):
        return time_(mix(mB, fw, b), mix(mF, b, fw), t)
    if mode in (4, 7):
        return mix(mO, time_(r, s, t), time_(mix(mB, fw, b), mix(mF, b, fw), t))
    return np.asarray(mO, np.int64).astype(F) / F(255.0)


# ------------------------------------------------------------------------------------------------ control

def cdiv(a, d):
    """C's integer division of an int64 array by a positive int"""
    return np.sign(a) * (np.abs(a) // d)


def sad_mask(vx, vy, sad, bits, ml, pel, bsx, bsy, XP, YP, time256, stepx, stepy):
    """MaskFun.cpp:133-166 MakeSADMaskTime (gamma 1), then :63-80 CheckAndPadMaskSmall"""
    nby, nbx = vx.shape
    tx, ty = (256 - time256) * 16 // (stepx * pel), (256 - time256) * 16 // (stepy * pel)
    bx, by = np.meshgrid(np.arange(nbx), np.arange(nby))
    bxi, byi = bx - cdiv(vx.astype(np.int64) * tx, 4096), by - cdiv(vy.astype(np.int64) * ty, 4096)
    out = (bxi < 0) | (bxi >= nbx) | (byi < 0) | (byi >= nby)
    bxi, byi = np.where(out, bx, bxi), np.where(out, by, byi)
    s = sad.astype(np.int64)[byi, bxi] >> (bits - 8)
    l = 255 * (s.astype(np.float64) * (4.0 / (ml * bsx * bsy)))
    m = np.zeros((YP, XP), np.uint8)
    m[:nby, :nbx] = np.where(l > 255, 255, l).astype(np.int64).astype(np.uint8)
    m[:nby, nbx:] = m[:nby, nbx - 1:nbx]
    m[nby:, :] = m[nby - 1:nby, :]
    return m


class BlockFPSFloat:
    """ad_bw / ad_fw: the VECTORS' analysis data (an 8..16 bit search); nscd1, nscd2: the scaled thresholds (vector_fields.scaled_thresholds)"""

    def __init__(self, oracle, ad_bw, ad_fw, nscd1, nscd2, mode=3, ml=100.0, blend=1, gray=False):
        self.oracle, self.ad, self.adf = oracle, ad_bw, ad_fw
        self.nscd1, self.nscd2 = int(nscd1), int(nscd2)
        self.mode, self.ml, self.blend = 3 if mode is None else int(mode), float(ml), 1 if blend is None else int(bool(blend))
        self.nplanes = 1 if gray else 3
        ad = ad_bw
        self.sub = [(0, 0)] + [(ad.xRatioUV.bit_length() - 1, ad.yRatioUV.bit_length() - 1)] * 2
        self.overlap = ad.nOverlapX > 0 or ad.nOverlapY > 0
        sx, sy = ad.nBlkSizeX - ad.nOverlapX, ad.nBlkSizeY - ad.nOverlapY
        self.XP, self.YP = ad.nBlkX, ad.nBlkY
        while self.XP * sx + ad.nOverlapX < ad.nWidth:
            self.XP += 1
        while self.YP * sy + ad.nOverlapY < ad.nHeight:
            self.YP += 1
        self.WP, self.HP = self.XP * sx + ad.nOverlapX, self.YP * sy + ad.nOverlapY
        self.win = {}
        self.masks = None  # after a usable frame in a mask mode: the upsized luma masks (F, B, O), cut to the frame

    def interior(self, sup, p):
        ad = self.ad
        sx, sy = self.sub[p]
        h, w = ad.nHeight >> sy, ad.nWidth >> sx
        vp, hp = (ad.nVPadding, ad.nHPadding) if p == 0 else (ad.nVPadding >> 1, ad.nHPadding >> 1)
        return np.array(np.asarray(sup[p])[vp:vp + h, hp:hp + w])

    def usable(self, t, src_sup, ref_sup, blob_f, blob_b):
        if src_sup is None or ref_sup is None or blob_f is None or blob_b is None or not 0 < t < 256:
            return False
        return degrain_n_ref.usable(blob_f, self.adf, self.nscd1, self.nscd2) and degrain_n_ref.usable(blob_b, self.ad, self.nscd1, self.nscd2)

    def small_masks(self, t, vF, vB):
        """the padded small masks (F, B, O) of a usable frame; vF / vB: (vx, vy, sad) of mvfw at nright / mvbw at nleft"""
        ad = self.ad
        sx, sy = ad.nBlkSizeX - ad.nOverlapX, ad.nBlkSizeY - ad.nOverlapY
        if self.mode <= 5:
            mF = flow_ref.occlusion_mask(vF[0], vF[1], False, self.ml, ad.nPel, self.XP, self.YP, t, sx, sy)
            mB = flow_ref.occlusion_mask(vB[0], vB[1], True, self.ml, ad.nPel, self.XP, self.YP, 256 - t, sx, sy)
        else:
            mF = sad_mask(*vF, ad.bitsPerSample, self.ml, ad.nPel, ad.nBlkSizeX, ad.nBlkSizeY, self.XP, self.YP, t, sx, sy)
            mB = sad_mask(*vB, ad.bitsPerSample, self.ml, ad.nPel, ad.nBlkSizeX, ad.nBlkSizeY, self.XP, self.YP, 256 - t, sx, sy)
        mO = ((mF.astype(np.int64) * mB.astype(np.int64)) // 255).astype(np.uint8)
        return mF, mB, mO

    def frame(self, t, clip_l, clip_r, src_sup, ref_sup, blob_f, blob_b):
        """one output frame at time256 t between clip_l / clip_r (float32 planes; their super frames and blobs None outside the clip)"""
        ad, mode = self.ad, self.mode
        if not self.usable(t, src_sup, ref_sup, blob_f, blob_b):
            self.masks = None
            if t <= 0 or (t < 256 and not self.blend):
                return [np.array(clip_l[p]) for p in range(self.nplanes)]
            if t >= 256:
                return [np.array(clip_r[p]) for p in range(self.nplanes)]
            return [time_(np.asarray(clip_r[p]), np.asarray(clip_l[p]), t) for p in range(self.nplanes)]
        logpel = {1: 0, 2: 1, 4: 2}[ad.nPel]
        nbx, nby = ad.nBlkX, ad.nBlkY
        vF = pl.blob_vectors(blob_f, self.adf)
        vB = pl.blob_vectors(blob_b, ad)
        small = self.small_masks(t, vF, vB) if mode >= 3 else None
        bxs, bys = np.tile(np.arange(nbx), nby), np.repeat(np.arange(nby), nbx)
        stepx0, stepy0 = ad.nBlkSizeX - ad.nOverlapX, ad.nBlkSizeY - ad.nOverlapY
        flat = lambda a: a.reshape(-1).astype(np.int64)
        bX = bxs * stepx0 * ad.nPel + ((flat(vB[0]) * (256 - t)) >> 8)
        bY = bys * stepy0 * ad.nPel + ((flat(vB[1]) * (256 - t)) >> 8)
        fX = bxs * stepx0 * ad.nPel + ((flat(vF[0]) * t) >> 8)
        fY = bys * stepy0 * ad.nPel + ((flat(vF[1]) * t) >> 8)
        out = []
        for p in range(self.nplanes):
            sx, sy = self.sub[p]
            H, W = ad.nHeight >> sy, ad.nWidth >> sx
            bw, bh, ox, oy = ad.nBlkSizeX >> sx, ad.nBlkSizeY >> sy, ad.nOverlapX >> sx, ad.nOverlapY >> sy
            stepx, stepy = bw - ox, bh - oy
            covW, covH = (nbx * stepx0 + ad.nOverlapX) >> sx, (nby * stepy0 + ad.nOverlapY) >> sy
            hpad, vpad = (ad.nHPadding >> sx) * ad.nPel, (ad.nVPadding >> sy) * ad.nPel
            prows = H + 2 * (ad.nVPadding >> sy)
            s_in, r_in = self.interior(src_sup, p), self.interior(ref_sup, p)
            dst = time_(r_in, s_in, t)  # the strips no block covers; the rest is overwritten
            jj, ii = np.arange(bh)[None, :, None], np.arange(bw)[None, None, :]

            def fetch(sup, X, Y):
                nx, ny = cdiv(X, 1 << sx) + hpad, cdiv(Y, 1 << sy) + vpad
                idx = (nx & (ad.nPel - 1)) | ((ny & (ad.nPel - 1)) << logpel)
                rows, cols = (idx * prows + (ny >> logpel))[:, None, None] + jj, (nx >> logpel)[:, None, None] + ii
                return np.asarray(sup[p])[rows, cols]
            b, fw = fetch(ref_sup, bX, bY), fetch(src_sup, fX, fY)
            assert b.dtype == F and fw.dtype == F
            rows, cols = (bys * stepy)[:, None, None] + jj, (bxs * stepx)[:, None, None] + ii
            zero = np.zeros(rows.shape[:1] + (bh, bw), np.int64)
            mF = mB = mO = zero
            if mode >= 3:
                dw, dh = (self.WP, self.HP) if p == 0 else (self.WP // ad.xRatioUV, self.HP // ad.yRatioUV)
                full = [flow_ref.upsize_u8(m, dw, dh).astype(np.int64) for m in small]
                if p == 0:
                    self.masks = [m[:H, :W] for m in full]
                mF, mB, mO = (m[rows, cols] for m in full)
                if mode in (5, 8):
                    mF = mB = zero
                elif mode in (3, 6):
                    mO = zero
            V = value(mode, t, s_in[rows, cols], r_in[rows, cols], b, fw, mF, mB, mO)
            assert V.dtype == F
            if not self.overlap:
                for k in range(nbx * nby):
                    dst[bys[k] * bh:(bys[k] + 1) * bh, bxs[k] * bw:(bxs[k] + 1) * bw] = V[k]
            else:
                key = (bw, bh, ox, oy)
                if key not in self.win:
                    self.win[key] = degrain_n_ref.windows(self.oracle, bw, bh, ox, oy)
                win = self.win[key]
                acc, wsum = np.zeros((covH, covW), F), np.zeros((covH, covW), np.int64)
                for k in range(nbx * nby):  # by outer, bx inner
                    by, bx = int(bys[k]), int(bxs[k])
                    w9 = (0 if by == 0 else 6 if by == nby - 1 else 3) + (2 if bx == nbx - 1 else (0 if bx == 0 else 1))
                    ys, xs = slice(by * stepy, by * stepy + bh), slice(bx * stepx, bx * stepx + bw)
                    acc[ys, xs] = acc[ys, xs] + V[k] * win[w9].astype(F)
                    wsum[ys, xs] += win[w9]
                res = acc / wsum.astype(F)
                assert res.dtype == F
                dst[:covH, :covW] = res
            out.append(dst)
        return out
