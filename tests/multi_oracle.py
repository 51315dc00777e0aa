"""What the RecalculateN tests and the tests of the temporal-radius filters in the VapourSynth shell share (test infrastructure): a clip and what
the CPU ORACLE makes of it at a radius -- super frames, the oracle.Analyse blob of every (frame, field), oracle.Recalculate on those -- computed once
per case and shared, never changed.  Nothing here comes from the library, the Python package or the shell.

The clip is tests/multi_cases.py's: the (1, 0)-per-frame moving texture of tests/degrain_n_cases.py at 96x64 with 2 * radius + 3 frames.  Every frame
is a job, so the first and the last `radius` frames have references outside the clip on one side."""
import numpy as np

import degrain_n_cases as dc
import multi_cases as mc
import mvoracle as mo
import pipeline as pl

# the RecalculateN geometries: (tag, super kwargs, analyse kwargs, recalculate kwargs)
R168_84 = ("16-8to8-4", dict(pel=2), dict(blksize=16, overlap=8), dict(blksize=8, overlap=4))
R84_80 = ("8-4to8-0", dict(pel=2), dict(blksize=8, overlap=4), dict(blksize=8, overlap=0))
RECALC_GEOS = (R168_84, R84_80)
RECALC_FORMATS = (("420", 8), ("420", 16), ("444", 8))

# thsad of every RecalculateN case: chosen on the CPU (tests/test_multi_recalculate_cases.py) so that, through the oracle alone, at least a fiftieth of
# the blocks of the valid fields keep their interpolated vector and at least a fiftieth are searched again (the shares it leaves: 0.40 .. 0.48 searched
# again, 0.52 .. 0.60 kept)
RECALC_THSAD = 150
SHARE = 0.02


def recalc_cases():
    """(fmt, bits, geometry, radius, extra recalculate kwargs)"""
    out = [(fmt, bits, geo, radius, {}) for fmt, bits in RECALC_FORMATS for geo in RECALC_GEOS for radius in mc.RADII]
    out += [("420", 8, R168_84, 2, dict(divide=1)), ("420", 16, R168_84, 3, dict(divide=1)), ("420", 8, R84_80, 2, dict(smooth=0)),
            ("444", 8, R168_84, 3, dict(smooth=0)), ("420", 8, R168_84, 2, dict(divide=1, smooth=0))]
    return out


def recalc_id(c):
    fmt, bits, geo, radius, extra = c
    return "%s-%dbit-%s-r%d%s" % (fmt, bits, geo[0], radius, "".join("-%s%s" % kv for kv in sorted(extra.items())))


class Multi:
    """frames, osup, osf (super frames), ads[r], blobs[n][r] (oracle.Analyse(isb, delta) of frame n against its field's reference; the invalid blob outside
    the clip) of one clip at a radius"""

    def __init__(self, fmt, bits, skw, akw, radius, w=mc.W, h=mc.H, nframes=None, frames=None, fmt_kw=None):
        self.fmt, self.bits, self.radius, self.w, self.h = fmt, bits, radius, w, h
        self.frames = frames if frames is not None else dc.clip(w, h, bits, nframes or mc.nframes(radius), fmt)
        self.n = len(self.frames)
        self.skw, self.akw = dict(skw), dict(akw)
        self.osup = mo.Super(w, h, bits, **dict(dc.FORMATS[fmt] if fmt_kw is None else fmt_kw, **skw))
        self.osf = [self.osup.frame(f) for f in self.frames]
        ans = [mo.Analyse(self.osup, num_frames=self.n, isb=mc.field_of(r)[0], delta=mc.field_of(r)[1], **akw) for r in range(2 * radius)]
        self.ads = [a.ad for a in ans]
        self.blobs = [[ans[r].frame(self.osf[n], self.ref(n, r)) for r in range(2 * radius)] for n in range(self.n)]
        self._recalc = {}

    def nref(self, n, r):
        isb, d = mc.field_of(r)
        m = n + d if isb else n - d
        return m if 0 <= m < self.n else None

    def ref(self, n, r):
        m = self.nref(n, r)
        return None if m is None else self.osf[m]

    def recalc(self, **rkw):
        """(ads[r], blobs[n][r]) of oracle.Recalculate(**rkw) on every field"""
        key = tuple(sorted(rkw.items()))
        if key not in self._recalc:
            rcs = [mo.Recalculate(self.osup, self.ads[r], **rkw) for r in range(2 * self.radius)]
            self._recalc[key] = ([rc.ad for rc in rcs],
                                 [[rcs[r].frame(self.osf[n], self.ref(n, r), self.blobs[n][r]) for r in range(2 * self.radius)] for n in range(self.n)])
        return self._recalc[key]

    def recalc_shares(self, **rkw):
        """the shares of blocks, over every valid (frame, field), that Recalculate(**rkw) searches again / leaves on the interpolated vector: a block is
        searched again exactly when the SAD of its interpolated vector -- what a Recalculate with a threshold nothing exceeds reports -- is above the
        scaled thsad (PlaneOfBlocks.cpp:1158-1424)"""
        rc = mo.Recalculate(self.osup, self.ads[0], **rkw)
        never = dict(rkw, thsad=10 ** 7)
        ads, blobs = self.recalc(**{k: v for k, v in never.items() if k != "divide"})
        again = total = 0
        for n in range(self.n):
            for r in range(2 * self.radius):
                if self.nref(n, r) is None:
                    continue
                sad = pl.blob_vectors(blobs[n][r], ads[r])[2]
                again += int((sad > rc.d.thSAD).sum())
                total += sad.size
        return again / total, 1 - again / total


_multis = {}


def multi(fmt, bits, skw, akw, radius, **kw):
    key = (fmt, bits, tuple(sorted(skw.items())), tuple(sorted(akw.items())), radius, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _multis:
        _multis[key] = Multi(fmt, bits, skw, akw, radius, **kw)
    return _multis[key]


def recalc_multi(case):
    fmt, bits, geo, radius, _ = case
    return multi(fmt, bits, geo[1], geo[2], radius)


def recalc_kwargs(case):
    return dict(case[2][3], thsad=RECALC_THSAD, **case[4])


def fields_of_dump(data, nframes, nfields):
    """what the mini host's vector pipelines write -- per frame and field 84 bytes of analysis data, then the blob, whose first int is its size -- ->
    [n][r] = (84 bytes, blob)"""
    data = np.frombuffer(data, dtype=np.uint8)
    out, off = [], 0
    for n in range(nframes):
        row = []
        for r in range(nfields):
            ad = data[off:off + 84]
            size = int(data[off + 84:off + 88].view(np.int32)[0])
            row.append((ad.tobytes(), data[off + 84:off + 84 + size]))
            off += 84 + size
        out.append(row)
    assert off == data.size, "the dump holds %d bytes, its fields %d" % (data.size, off)
    return out
