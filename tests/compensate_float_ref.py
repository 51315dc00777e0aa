"""Numpy float32 restatement of Compensate / CompensateN on a float clip (mvx_compensate_create_float, mvx_compensate_n_create_float), test
infrastructure: written from the description in include/mvtools_amd.h, not from the kernel.  tests/test_compensate_float_ref.py anchors it to
oracle.Compensate on integer-valued frames.

Control, per field (the integer filter's, MVCompensate.c:73-374):
    usable        the reference is inside the clip, the blob is valid and no more than nSCD2 of its level-0 blocks have a SAD above nSCD1
    not usable    the output is the reference frame at scbehavior 0 where there is one, else the source frame
    a block       comes from the reference super frame at its own place plus its vector scaled by time (v * time256 / 256, truncated towards 0)
                  when its SAD is below the scaled thsad, else from the source super frame at its own place
    strips        what no block covers is the source frame at scbehavior 1, the reference frame at 0
    CompensateN   output k of 2 * tr + 1 is the source for k == tr, before it the forward field (odd) of distance tr - k, behind it the backward
                  field (even) of distance k - tr

The float cell:
    every copy    bit for bit: the centre, an unusable field, the strips, blocks side by side (overlap 0)
    overlap > 0   acc = 0; over the covering blocks, by outer and bx inner, ascending: acc = acc + v * float(win); out = acc / float(wsum), wsum the
                  integer sum of the same window weights; no shift, no rounding term, no clamp

Super frames are given as arrays of level 0: per plane the pel * pel sub-pel planes stacked, as tests/degrain_float_ref.py takes them."""
import numpy as np

import degrain_n_ref
import pipeline as pl

F = np.float32


def field_of(tr, k):
    """output k of a CompensateN job -> its field, -1 for the centre"""
    if k == tr:
        return -1
    return 2 * (tr - k - 1) + 1 if k < tr else 2 * (k - tr - 1)


class CompensateFloat:
    """ad: the VECTORS' analysis data (an 8..16 bit search); thsad, nscd1, nscd2: the scaled thresholds (vector_fields.scaled_thresholds);
    time: 0..100; gray: a one-plane clip"""

    def __init__(self, oracle, ad, thsad, nscd1, nscd2, time=100.0, scbehavior=1, gray=False):
        self.oracle, self.ad = oracle, ad
        self.thsad, self.nscd1, self.nscd2 = int(thsad), int(nscd1), int(nscd2)
        self.time256 = int(time * 256 / 100)
        self.scbehavior = 1 if scbehavior is None else int(bool(scbehavior))
        self.nplanes = 1 if gray else 3
        self.sub = [(0, 0)] + [(ad.xRatioUV.bit_length() - 1, ad.yRatioUV.bit_length() - 1)] * 2
        self.overlap = ad.nOverlapX > 0 or ad.nOverlapY > 0
        self.win = {}
        self.wsum_range = None  # after a field with overlap: (min, max) of the windows' totals over the covered samples
        self.from_ref = None    # after a usable field: bool per block, True where the block is compensated

    def inner(self, sup, p):
        """the frame inside a super plane: the unpadded window of sub-pel plane 0"""
        ad = self.ad
        sx, sy = self.sub[p]
        h, w, vp, hp = ad.nHeight >> sy, ad.nWidth >> sx, ad.nVPadding >> sy, ad.nHPadding >> sx
        return np.array(np.asarray(sup[p])[vp:vp + h, hp:hp + w])

    def usable(self, ref_sup, blob):
        return ref_sup is not None and degrain_n_ref.usable(blob, self.ad, self.nscd1, self.nscd2)

    def field(self, src_sup, ref_sup, blob):
        """one compensated frame: src_sup / ref_sup are level-0 super frame planes (ref_sup None: outside the clip) -> planes of their dtype"""
        ad = self.ad
        if not self.usable(ref_sup, blob):
            self.from_ref = None
            pick = ref_sup if (not self.scbehavior and ref_sup is not None) else src_sup
            return [self.inner(pick, p) for p in range(self.nplanes)]
        logpel = {1: 0, 2: 1, 4: 2}[ad.nPel]
        nbx, nby = ad.nBlkX, ad.nBlkY
        vx, vy, sad = (a.reshape(-1).astype(np.int64) for a in pl.blob_vectors(blob, ad))
        bxs, bys = np.tile(np.arange(nbx), nby), np.repeat(np.arange(nby), nbx)
        stepx0, stepy0 = ad.nBlkSizeX - ad.nOverlapX, ad.nBlkSizeY - ad.nOverlapY
        from_ref = sad < self.thsad
        self.from_ref = from_ref
        trunc = lambda v: np.sign(v) * (np.abs(v) // 256)  # C's division
        blx0 = bxs * stepx0 * ad.nPel + np.where(from_ref, trunc(vx * self.time256), 0)
        bly0 = bys * stepy0 * ad.nPel + np.where(from_ref, trunc(vy * self.time256), 0)
        out = []
        for p in range(self.nplanes):
            sx, sy = self.sub[p]
            H = ad.nHeight >> sy
            bw, bh, ox, oy = ad.nBlkSizeX >> sx, ad.nBlkSizeY >> sy, ad.nOverlapX >> sx, ad.nOverlapY >> sy
            stepx, stepy = bw - ox, bh - oy
            WB, HB = (nbx * stepx0 + ad.nOverlapX) >> sx, (nby * stepy0 + ad.nOverlapY) >> sy
            hpad, vpad = (ad.nHPadding >> sx) * ad.nPel, (ad.nVPadding >> sy) * ad.nPel
            prows = H + 2 * (ad.nVPadding >> sy)
            blx, bly = (blx0 >> sx, bly0 >> sy) if p else (blx0, bly0)
            nx, ny = blx + hpad, bly + vpad
            idx = (nx & (ad.nPel - 1)) | ((ny & (ad.nPel - 1)) << logpel)
            jj, ii = np.arange(bh)[None, :, None], np.arange(bw)[None, None, :]
            rows, cols = (idx * prows + (ny >> logpel))[:, None, None] + jj, (nx >> logpel)[:, None, None] + ii
            s, r = np.asarray(src_sup[p]), np.asarray(ref_sup[p])
            V = np.where(from_ref[:, None, None], r[rows, cols], s[rows, cols])  # (a selection: the bytes are not touched)
            assert V.dtype == s.dtype
            dst = self.inner(src_sup if self.scbehavior else ref_sup, p)
            if not self.overlap:
                for b in range(nbx * nby):
                    dst[bys[b] * bh:(bys[b] + 1) * bh, bxs[b] * bw:(bxs[b] + 1) * bw] = V[b]
            else:
                assert V.dtype == F, "overlapped blocks are float arithmetic"
                key = (bw, bh, ox, oy)
                if key not in self.win:
                    self.win[key] = degrain_n_ref.windows(self.oracle, bw, bh, ox, oy)
                win = self.win[key]
                acc, wsum = np.zeros((HB, WB), F), np.zeros((HB, WB), np.int64)
                for b in range(nbx * nby):  # by outer, bx inner
                    by, bx = int(bys[b]), int(bxs[b])
                    k = (0 if by == 0 else 6 if by == nby - 1 else 3) + (2 if bx == nbx - 1 else (0 if bx == 0 else 1))
                    ys, xs = slice(by * stepy, by * stepy + bh), slice(bx * stepx, bx * stepx + bw)
                    acc[ys, xs] = acc[ys, xs] + V[b] * win[k].astype(F)
                    wsum[ys, xs] += win[k]
                lo, hi = int(wsum.min()), int(wsum.max())
                self.wsum_range = (lo, hi) if self.wsum_range is None else (min(lo, self.wsum_range[0]), max(hi, self.wsum_range[1]))
                res = acc / wsum.astype(F)
                assert res.dtype == F
                dst[:HB, :WB] = res
            out.append(dst)
        return out

    def job(self, tr, src_sup, ref_sups, blobs):
        """CompensateN: ref_sups / blobs per field in the order mvbw1, mvfw1, mvbw2, ... -> 2 * tr + 1 frames in temporal order"""
        out = []
        for k in range(2 * tr + 1):
            f = field_of(tr, k)
            out.append([self.inner(src_sup, p) for p in range(self.nplanes)] if f < 0 else self.field(src_sup, ref_sups[f], blobs[f]))
        return out
