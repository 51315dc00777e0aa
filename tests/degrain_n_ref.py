"""Numpy restatement of the reference's Degrain at ANY temporal radius (test infrastructure): the yardstick of mv.DegrainN beyond radius 6,
where the CPU oracle's arrays end.  Written from the reference, whose arithmetic is a template over the radius:

    DegrainWeight              MVDegrains.h:184-189
    useBlock                   MVDegrains.h:192-206   (an unusable reference: weight 0)
    normaliseWeights<radius>   MVDegrains.h:208-223
    Degrain_C<radius>          MVDegrains.h:30-53
    LimitChanges_C             MVDegrains.h:163-181
    mvdegrainGetFrame          MVDegrains.cpp:85-330  (plane selection, the block loop, uncovered strips)
    overlaps_c / ToPixels      Overlap.cpp:143-158,335-356
    fgopIsUsable               Fakery.c:52-58,103-107,144-146
    mvpGetPointer              MVFrame.cpp:1686-1704,1732-1734

It takes the thresholds as TABLES per temporal distance, already scaled (MVDegrains.cpp:658-659), so no cosine is restated here; reference r
(order mvbw, mvfw, mvbw2, mvfw2, ...) is weighed against entry r // 2.  The nine overlap windows come from the oracle's overInit
(mvo_over_init, Overlap.cpp:40-125): they do not depend on the radius, and float cosines are not worth a second implementation.
tests/test_degrain_n_ref.py holds this file byte for byte to oracle.Degrain at radii 1, 2, 3 and 6."""
import ctypes as C

import numpy as np

import pipeline as pl


def degrain_weights(th, sad):
    """MVDegrains.h:184-189 on int64 arrays.  The reference forms (thSAD - blockSAD) * (thSAD + blockSAD) * 256 in int64, which wraps for
    thresholds beyond about 1.9e8: the product is formed modulo 2^64 here too."""
    th, sad = np.broadcast_arrays(np.asarray(th, np.int64), np.asarray(sad, np.int64))
    live = sad < th
    s = np.where(live, sad, 0)
    num = ((th - s).astype(np.uint64) * (th + s).astype(np.uint64) * np.uint64(256)).astype(np.int64)
    den = (th * th + s * s).astype(np.float64)
    w = np.trunc(num.astype(np.float64) / np.where(live, den, 1.0)).astype(np.int64)
    return np.where(live, w, 0)


def normalise(w):
    """MVDegrains.h:208-223 on [..., references]: -> (WSrc[...], WRefs[..., references])"""
    w = np.asarray(w, np.int64)
    scale = 256.0 / (257 + w.sum(axis=-1)).astype(np.float64)
    out = np.trunc(w.astype(np.float64) * scale[..., None]).astype(np.int64)
    return 256 - out.sum(axis=-1), out


def usable(blob, ad, nscd1, nscd2):
    """fgopIsUsable: validity == 1 and not more than nscd2 level-0 blocks with a SAD above nscd1"""
    b = np.asarray(blob, np.uint8)
    if int(b[4:8].view(np.int32)[0]) != 1:
        return False
    _, _, sad = pl.blob_vectors(b, ad)
    return not int(np.count_nonzero(sad > nscd1)) > nscd2


def windows(oracle, bw, bh, ox, oy):
    """the nine windows of overInit as int64 [9, bh, bw]"""
    w = np.zeros(9 * bw * bh, np.int16)
    oracle.lib().mvo_over_init(w.ctypes.data_as(C.c_void_p), bw, bh, ox, oy)
    return w.reshape(9, bh, bw).astype(np.int64)


class DegrainN:
    """radius: any; ad: the vector clips' analysis data; th_luma / th_chroma: scaled thresholds per distance 1..radius; nscd1 / nscd2: the scaled
    scene-change thresholds; plane 0..4 and limit / limitc as the filter's arguments.  gray: a one-plane clip."""

    def __init__(self, oracle, radius, ad, th_luma, th_chroma, nscd1, nscd2, plane=4, limit=None, limitc=None, gray=False):
        assert len(th_luma) == radius and len(th_chroma) == radius
        self.oracle, self.radius, self.ad, self.n = oracle, radius, ad, 2 * radius
        self.th = [np.repeat(np.asarray(t, np.int64), 2) for t in (th_luma, th_chroma)]  # per reference
        self.nscd1, self.nscd2 = int(nscd1), int(nscd2)
        self.nplanes = 1 if gray else 3
        yuv = (1, 2, 4, 6, 7)[plane]
        self.process = [bool(yuv & 1), bool(yuv & 2), bool(yuv & 4)]
        pm = (1 << ad.bitsPerSample) - 1
        limit = pm if limit is None else limit
        self.limit = [limit, limit if limitc is None else limitc, limit if limitc is None else limitc]
        self.sub = [(0, 0)] + [(ad.xRatioUV.bit_length() - 1, ad.yRatioUV.bit_length() - 1)] * 2
        self.overlap = ad.nOverlapX > 0 or ad.nOverlapY > 0
        self.win = {}
        self.plan = None  # after frame(): per plane class (WSrc[blocks], WRefs[blocks, references]), normalised

    def _weights(self, sads, ok):
        """sads: int64 [references, blocks]; ok: bool [references] -> per class (WSrc, WRefs)"""
        out = []
        for c in range(2):
            w = degrain_weights(self.th[c][:, None], sads) * np.asarray(ok, np.int64)[:, None]
            out.append(normalise(w.T))
        return out

    def weigh(self, ref_supers, blobs):
        """useBlock + DegrainWeight + normaliseWeights for every block: sets self.plan; -> (usable[references], vx, vy [references, blocks])"""
        ad, n = self.ad, self.n
        ok = [ref_supers[r] is not None and usable(blobs[r], ad, self.nscd1, self.nscd2) for r in range(n)]
        vx, vy, sad = (np.zeros((n, ad.nBlkY * ad.nBlkX), np.int64) for _ in range(3))
        for r in range(n):
            if ok[r]:
                x, y, s = pl.blob_vectors(blobs[r], ad)
                vx[r], vy[r], sad[r] = x.reshape(-1), y.reshape(-1), s.reshape(-1)
        self.plan = self._weights(sad, ok)
        return ok, vx, vy

    def frame(self, src, ref_supers, blobs):
        """src: the clip frame's planes; ref_supers[r]: super frame planes or None; blobs[r]: MVTools_vectors -> output planes"""
        ad, n = self.ad, self.n
        logpel = {1: 0, 2: 1, 4: 2}[ad.nPel]
        nbx, nby = ad.nBlkX, ad.nBlkY
        ok, vx, vy = self.weigh(ref_supers, blobs)
        bxs, bys = np.tile(np.arange(nbx), nby), np.repeat(np.arange(nby), nbx)
        stepx0, stepy0 = ad.nBlkSizeX - ad.nOverlapX, ad.nBlkSizeY - ad.nOverlapY
        out = []
        for p in range(self.nplanes):
            s = np.asarray(src[p])
            if not self.process[p]:  # MVDegrains.cpp:211-214
                out.append(s.copy())
                continue
            sx, sy = self.sub[p]
            H, W = ad.nHeight >> sy, ad.nWidth >> sx
            bw, bh, ox, oy = ad.nBlkSizeX >> sx, ad.nBlkSizeY >> sy, ad.nOverlapX >> sx, ad.nOverlapY >> sy
            stepx, stepy = bw - ox, bh - oy
            WB, HB = (nbx * stepx0 + ad.nOverlapX) >> sx, (nby * stepy0 + ad.nOverlapY) >> sy
            hpad, vpad = (ad.nHPadding >> sx) * ad.nPel, (ad.nVPadding >> sy) * ad.nPel
            prows = H + 2 * (ad.nVPadding >> sy)  # rows of one sub-pel plane of level 0
            wsrc, wref = self.plan[1 if p else 0]
            jj, ii = np.arange(bh)[None, :, None], np.arange(bw)[None, None, :]
            y0, x0 = (bys * stepy)[:, None, None], (bxs * stepx)[:, None, None]
            total = 128 + s[y0 + jj, x0 + ii].astype(np.int64) * wsrc[:, None, None]  # MVDegrains.h:40-48
            for r in range(n):
                if not ok[r]:
                    continue
                blx, bly = ((bxs * stepx0) << logpel) + vx[r], ((bys * stepy0) << logpel) + vy[r]  # Fakery.c:31-32, MVDegrains.h:196-197
                if p:
                    blx, bly = blx >> sx, bly >> sy
                nx, ny = blx + hpad, bly + vpad
                idx = (nx & (ad.nPel - 1)) | ((ny & (ad.nPel - 1)) << logpel)
                rows, cols = (idx * prows + (ny >> logpel))[:, None, None] + jj, (nx >> logpel)[:, None, None] + ii
                total += np.asarray(ref_supers[r][p])[rows, cols].astype(np.int64) * wref[:, r][:, None, None]
            val = (total >> 8).astype(s.dtype).astype(np.int64)
            dst = s.copy()  # the strips no block covers keep the source (MVDegrains.cpp:238-249,290-298)
            if not self.overlap:
                for b in range(nbx * nby):
                    dst[bys[b] * bh:(bys[b] + 1) * bh, bxs[b] * bw:(bxs[b] + 1) * bw] = val[b]
            else:
                key = (bw, bh, ox, oy)
                if key not in self.win:
                    self.win[key] = windows(self.oracle, bw, bh, ox, oy)
                win = self.win[key]
                acc = np.zeros((HB, WB), np.uint16 if ad.bitsPerSample <= 8 else np.uint32)
                for b in range(nbx * nby):  # overlaps_c
                    by, bx = int(bys[b]), int(bxs[b])
                    wby = ((by + nby - 3) // (nby - 2)) * 3
                    wbx = 2 if bx == nbx - 1 else (0 if bx == 0 else 1)
                    acc[by * stepy:by * stepy + bh, bx * stepx:bx * stepx + bw] += ((val[b] * win[wby + wbx]) >> 6).astype(acc.dtype)
                a = (acc.astype(np.int64) + 16) >> 5  # ToPixels
                dst[:HB, :WB] = np.minimum(a, (1 << ad.bitsPerSample) - 1 if ad.bitsPerSample > 8 else 255).astype(s.dtype)
            lim = self.limit[p]
            if lim < (1 << ad.bitsPerSample) - 1:  # LimitChanges_C
                si = s.astype(np.int64)
                dst = np.minimum(np.maximum(dst.astype(np.int64), si - lim), si + lim).astype(s.dtype)
            out.append(dst)
        return out

    def shares(self, min_distance=7):
        """among the luma (block, reference) pairs of distance >= min_distance in the last frame's plan: (share with W > 0, share with W == 0)"""
        w = self.plan[0][1][:, 2 * (min_distance - 1):]
        return float(np.mean(w > 0)), float(np.mean(w == 0))
