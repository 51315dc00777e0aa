"""CPU restatement of deep mv.Mask: masks of 9 to 16 bits for clips of that depth (mvx_mask_create_deep; include/mvtools_amd.h states the
semantics, which are the library's own -- the reference refuses such clips, MVMask.c:321).  A subclass of mask_ref.Mask with three additions:

  the depth    B = bits of the clip argument, s = B - 8; the vector clip's own depth is not consulted
  the shift    kind 1 shifts the int64 SAD right by s, arithmetically, before it becomes a double: MakeSADMaskTime's
               `sad >> (bitsPerSample - 8)`, MaskFun.cpp:162, with bitsPerSample the clip's
  expansion    everything else (small masks, upsizer, edge replication, usability, the ysc fill) works on bytes as in mask_ref; every byte
               m then becomes expand(m): a weight (kinds 0-2) replicates its bits, (m << s) | (m >> (8 - s)); an offset (kinds 3, 4 and
               kind 5's U and V) scales, m << s.  Kind 5's luma is the clip's own at its depth.  At B = 8 expand(m) = m and the planes are bytes.

Counters beside mask_ref's:
  shifted  the kind 1 cells whose byte differs from what the unshifted SAD gives        cells  the kind 1 cells of usable frames
"""
import numpy as np

import mask_ref


def expand(m, s, weight):
    """E(m) for bytes m (array or int) at depth 8 + s"""
    m = np.asarray(m).astype(np.uint16)
    assert 0 <= s <= 8 and np.all(m <= 255)
    out = (m << s) | (m >> (8 - s)) if weight else m << s
    return out.astype(np.uint16)


class DeepMask(mask_ref.Mask):
    def __init__(self, ad, bits, **kw):
        super().__init__(ad, **kw)
        assert 8 <= bits <= 16
        self.bits, self.s = bits, bits - 8
        self.weight = self.kind <= 2
        self._plain = mask_ref.Mask(ad, **kw)      # the unshifted SAD mask, for the counter only
        self.shifted = self.cells = 0

    def sad_mask(self, vx, vy, sad, stats):
        sad = np.asarray(sad, np.int64)
        out = super().sad_mask(vx, vy, sad >> self.s, stats)                     # numpy's >> on int64 is arithmetic, as C's on int64_t
        plain = self._plain.sad_mask(vx, vy, sad, {})
        self.shifted += int(np.count_nonzero(out != plain))
        self.cells += out.size
        return out

    def expand(self, m):
        e = expand(m, self.s, self.weight)
        return e.astype(np.uint8) if self.bits == 8 else e

    def frame(self, blob, clip_luma=None, stats=None):
        """three planes of uint16 (uint8 at 8 bits); clip_luma: the clip's luma at its own depth (kind 5)"""
        a = self.ad
        dummy = np.zeros((a.nHeight, a.nWidth), np.uint8) if self.kind == 5 else None
        planes = [self.expand(p) for p in super().frame(blob, dummy, stats)]
        if self.kind == 5:
            luma = np.asarray(clip_luma)[:a.nHeight, :a.nWidth]
            assert luma.dtype == planes[1].dtype and int(luma.max()) < 1 << self.bits
            planes[0] = np.array(luma)
        return planes
