"""Numpy float32 restatement of DegrainN on a float clip (mvx_degrain_n_create_float), test infrastructure: written from the description of its
arithmetic (include/mvtools_amd.h), not from the kernel.  Usable references, weights, normalisation and the lists are the
integer filter's for the same blobs and come from tests/degrain_n_ref.py; what is restated here is the float cell:

    block value   S = float(WSrc) * s; for each list entry in reference order S = S + float(w) * ref; V = S * (1 / 256)
    overlap 0     out = V
    overlap > 0   acc = 0; over the covering blocks, by outer and bx inner, ascending: acc = acc + V * float(win); out = acc / float(wsum),
                  wsum the integer sum of the same window weights
    limit         8-bit scale: below 255, L = float(limit) / 255 and out = max(s - L, min(s + L, out))
    passed through bit for bit: a plane not selected, the strips no block covers, a job without a usable reference

A list holds the references whose weight is not 0 before the normalisation; one whose normalised weight is 0 adds float(0) * ref, which changes no
value (inputs are finite), so entries are taken by their normalised weight here.  tests/test_degrain_float_ref.py anchors this file to
tests/degrain_n_ref.py on integer-valued clips."""
import numpy as np

import degrain_n_ref

F = np.float32


class DegrainFloat:
    """arguments as degrain_n_ref.DegrainN; ad is the VECTORS' analysis data (an 8..16 bit search), limit / limitc are 0..255 or None"""

    def __init__(self, oracle, radius, ad, th_luma, th_chroma, nscd1, nscd2, plane=4, limit=None, limitc=None, gray=False):
        self.core = degrain_n_ref.DegrainN(oracle, radius, ad, th_luma, th_chroma, nscd1, nscd2, plane=plane, gray=gray)
        limit = 255 if limit is None else limit
        self.limit = [limit] + [limit if limitc is None else limitc] * 2
        self.win = {}

    @property
    def plan(self):
        return self.core.plan

    def frame(self, src, ref_supers, blobs):
        """src: float32 planes of the clip frame; ref_supers[r]: float32 super frame planes or None; blobs[r]: MVTools_vectors -> float32 planes"""
        core = self.core
        ad, n = core.ad, core.n
        logpel = {1: 0, 2: 1, 4: 2}[ad.nPel]
        nbx, nby = ad.nBlkX, ad.nBlkY
        ok, vx, vy = core.weigh(ref_supers, blobs)
        if not any(ok):
            return [np.array(src[p], F) for p in range(core.nplanes)]
        bxs, bys = np.tile(np.arange(nbx), nby), np.repeat(np.arange(nby), nbx)
        stepx0, stepy0 = ad.nBlkSizeX - ad.nOverlapX, ad.nBlkSizeY - ad.nOverlapY
        out = []
        for p in range(core.nplanes):
            s = np.array(src[p], F)
            if not core.process[p]:
                out.append(s)
                continue
            sx, sy = core.sub[p]
            H = ad.nHeight >> sy
            bw, bh, ox, oy = ad.nBlkSizeX >> sx, ad.nBlkSizeY >> sy, ad.nOverlapX >> sx, ad.nOverlapY >> sy
            stepx, stepy = bw - ox, bh - oy
            WB, HB = (nbx * stepx0 + ad.nOverlapX) >> sx, (nby * stepy0 + ad.nOverlapY) >> sy
            hpad, vpad = (ad.nHPadding >> sx) * ad.nPel, (ad.nVPadding >> sy) * ad.nPel
            prows = H + 2 * (ad.nVPadding >> sy)
            wsrc, wref = core.plan[1 if p else 0]
            jj, ii = np.arange(bh)[None, :, None], np.arange(bw)[None, None, :]
            y0, x0 = (bys * stepy)[:, None, None], (bxs * stepx)[:, None, None]
            S = wsrc.astype(F)[:, None, None] * s[y0 + jj, x0 + ii]
            for r in range(n):
                if not ok[r]:
                    continue
                blx, bly = ((bxs * stepx0) << logpel) + vx[r], ((bys * stepy0) << logpel) + vy[r]
                if p:
                    blx, bly = blx >> sx, bly >> sy
                nx, ny = blx + hpad, bly + vpad
                idx = (nx & (ad.nPel - 1)) | ((ny & (ad.nPel - 1)) << logpel)
                rows, cols = (idx * prows + (ny >> logpel))[:, None, None] + jj, (nx >> logpel)[:, None, None] + ii
                w = wref[:, r]
                t = S + w.astype(F)[:, None, None] * np.asarray(ref_supers[r][p], F)[rows, cols]
                S = np.where((w != 0)[:, None, None], t, S)
            V = S * F(1.0 / 256.0)
            assert V.dtype == F
            dst = s.copy()
            if not core.overlap:
                for b in range(nbx * nby):
                    dst[bys[b] * bh:(bys[b] + 1) * bh, bxs[b] * bw:(bxs[b] + 1) * bw] = V[b]
            else:
                key = (bw, bh, ox, oy)
                if key not in self.win:
                    self.win[key] = degrain_n_ref.windows(core.oracle, bw, bh, ox, oy)
                win = self.win[key]
                acc, wsum = np.zeros((HB, WB), F), np.zeros((HB, WB), np.int64)
                for b in range(nbx * nby):  # by outer, bx inner
                    by, bx = int(bys[b]), int(bxs[b])
                    k = ((by + nby - 3) // (nby - 2)) * 3 + (2 if bx == nbx - 1 else (0 if bx == 0 else 1))
                    ys, xs = slice(by * stepy, by * stepy + bh), slice(bx * stepx, bx * stepx + bw)
                    acc[ys, xs] = acc[ys, xs] + V[b] * win[k].astype(F)
                    wsum[ys, xs] += win[k]
                dst[:HB, :WB] = acc / wsum.astype(F)
            lim = self.limit[p]
            if lim < 255:
                L = F(lim) / F(255.0)
                dst = np.maximum(s - L, np.minimum(s + L, dst))
            assert dst.dtype == F
            out.append(dst)
        return out
