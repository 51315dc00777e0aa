"""Numpy restatement of mv.Flow and mv.FlowBlur on float clips (mvx_flowcomp_create_float, mvx_flowblur_create_float), test infrastructure:
written from the description of their arithmetic (include/mvtools_amd.h), not from the kernels.

The vector side is not restated here.  Which jobs are usable, the small fields, field_shift, the upsizer, the fetch positions, the shift's
destinations and winners, the tap counts and the tap positions all come out of tests/flowmc_ref.py, which is run on STAND-INS for the Finest
planes instead of on samples:
  Positions   a plane whose "sample" at (row, column) is its own flat position.  flowmc_ref.fetch then returns, per output sample, the position
              it would have read; flowmc_ref.shift, per destination, the position of the winning source -- or its "pixel_max", which the
              restatement is created with 62 bits for, above every position
  Taps        a plane that records the (rows, columns) of every read that flowmc_ref.blur makes: the sample itself, then the F taps, then the
              B taps, one read per tap number.  blur parks the lanes that have run out of taps at (0, 0); the stand-in is one luma sample of
              padding wider than the real plane on every side, so (0, 0) is no position a tap can take (taps stay inside the frame)
Only what a float sample undergoes is stated here:
  fetch       the 32 bits at the position, as they are
  shift       the 32 bits of the winner; where no source landed 1.0f on luma and 0.5f on chroma
  blur        sum = s; sum = sum + tap for the F taps, then the B taps (np.float32, one addition per tap, each rounded on its own);
              sum / np.float32(mF + mB + 1)
  copy        the clip frame's bits
The float Finest plane is the float super frame of tests/super_float_ref.py with its pel x pel sub-planes interleaved (finest).
tests/test_flowmc_float_ref.py anchors all of it to tests/flowmc_ref.py on integer-valued clips."""
import numpy as np

import flowmc_ref
import super_float_ref as sf

F = np.float32
HOLE = (F(1.0), F(0.5), F(0.5))       # the top of a float plane's nominal range: luma 0 .. 1, chroma -0.5 .. 0.5
POSITION_BITS = 62                    # the integer restatement's pixel_max = 2^62 - 1 marks a hole among positions


def bits(a):
    """the samples of a float32 plane as uint32: comparisons on these count NaN payloads and signed zeros"""
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def finest(sup_frame, width, height, sub=(1, 1), gray=False, hpad=16, vpad=16, pel=2):
    """the Finest frame of a float super frame (planes as super_float_ref.frame lays them out: sub-pel plane k = sx | sy << log2(pel) in rows
    k * rows .. (k + 1) * rows): Finest[y * pel + sy][x * pel + sx] = plane k [y][x], padding included"""
    planes, _ = sf.geometry(width, height, sub, gray, hpad, vpad, pel)
    lp = {1: 0, 2: 1, 4: 2}[pel]
    out = []
    for (w, h, hp, vp), s in zip(planes, sup_frame):
        rows, cols = h + 2 * vp, w + 2 * hp
        fin = np.zeros((rows * pel, cols * pel), np.uint32)
        for k in range(pel * pel):
            fin[k >> lp::pel, k & (pel - 1)::pel] = bits(s[k * rows:(k + 1) * rows, :cols])
        out.append(fin.view(F))
    return out


class Positions:
    """stands for a Finest plane of `shape`: reading (rows, columns) gives rows * width + columns"""

    def __init__(self, shape):
        self.shape = tuple(shape)

    def __getitem__(self, rc):
        return np.asarray(rc[0], np.int64) * self.shape[1] + np.asarray(rc[1], np.int64)


class Taps:
    """stands for a Finest plane of `shape`: records the (rows, columns) of every read and returns zeros"""

    def __init__(self, shape):
        self.shape, self.reads = tuple(shape), []

    def __getitem__(self, rc):
        rows, cols = np.broadcast_arrays(np.asarray(rc[0], np.int64), np.asarray(rc[1], np.int64))
        self.reads.append((rows.copy(), cols.copy()))
        return np.zeros(rows.shape, np.int64)


def gather(fin, pos, hole=None):
    """the bits of the float plane fin at flat positions pos; positions at the hole mark give `hole`"""
    flat = bits(fin).reshape(-1)
    empty = pos == (1 << POSITION_BITS) - 1
    assert hole is not None or not empty.any()
    out = flat[np.where(empty, 0, pos)]
    if hole is not None:
        out = np.where(empty, bits(np.array([hole], F))[0], out)
    return out.astype(np.uint32).view(F)


def blur_sum(fin, reads, shift):
    """the float rule over one plane: reads = Taps.reads of flowmc_ref.blur on a stand-in that is `shift` (rows, columns) wider than fin on
    the top / left -> (the output plane, mF + mB per sample)"""
    fin = np.asarray(fin, F)
    inside = lambda r, c: r.min() >= 0 and r.max() < fin.shape[0] and c.min() >= 0 and c.max() < fin.shape[1]
    r0, c0 = reads[0][0] - shift[0], reads[0][1] - shift[1]
    assert inside(r0, c0)
    total = fin[r0, c0].copy()
    count = np.zeros(total.shape, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for rows, cols in reads[1:]:
            live = ~((rows == 0) & (cols == 0))
            r, c = np.where(live, rows - shift[0], r0), np.where(live, cols - shift[1], c0)
            assert inside(r, c), "a tap outside the Finest plane"
            total = np.where(live, total + fin[r, c], total)      # float32 + float32, rounded once per tap
            assert total.dtype == F
            count += live
        out = total / (count + 1).astype(F)
    assert out.dtype == F
    # x / 1.0f is x bit for bit; numpy may quieten a signalling NaN, the bits of a sample without taps are the sample's
    return np.where(count == 0, bits(fin[r0, c0]), bits(out)).view(F), count


def _dummy(frame):
    return [np.zeros(p.shape, np.int64) for p in frame]


class _Float:
    def _geometry(self, hpad, vpad):
        a = self.ref.ad
        self.geo = dict(width=a.nWidth, height=a.nHeight, sub=(a.xRatioUV >> 1, a.yRatioUV >> 1), gray=self.ref.nplanes == 1, hpad=hpad, vpad=vpad, pel=a.nPel)

    def finest(self, sup_frame):
        return finest(sup_frame, **self.geo)


class Flow(_Float):
    """Flow(sample_float=True) over vector clip analysis data ad.  frame(): clip = the float frames, sup = callable k -> float super frame k
    (planes as super_float_ref.frame gives them), blob = the vectors at n (None = copy).  stats: flowmc_ref.shift's counters, on positions:
    "collide" = destinations that two or more sources claim, "hole" = destinations nobody reaches."""

    def __init__(self, ad, num_frames, nplanes, hpad, vpad, time=100.0, mode=0, thscd1=400, thscd2=130):
        self.ref = flowmc_ref.Flow(ad, num_frames, nplanes, hpad, vpad, POSITION_BITS, time=time, mode=mode, thscd1=thscd1, thscd2=thscd2)
        self._geometry(hpad, vpad)

    def frame(self, n, clip, sup, blob, field_shift=0, stats=None):
        fins = {}

        def stand_in(k):
            fins[k] = self.finest(sup(k))
            assert all(p.size < 1 << 20 for p in fins[k])  # (flowmc_ref.shift's counters hold positions below 2^20)
            return [Positions(p.shape) for p in fins[k]]
        pos = self.ref.frame(n, {n: _dummy(clip[n])}, stand_in, blob, field_shift, stats)
        self.last_kind = self.ref.last_kind
        if self.last_kind == "copy":
            return [bits(p).copy().view(F) for p in clip[n][:self.ref.nplanes]]
        fin = fins[self.ref.ref(n)]
        return [gather(fin[p], pos[p], HOLE[p] if self.ref.mode else None) for p in range(self.ref.nplanes)]


class FlowBlur(_Float):
    """FlowBlur(sample_float=True) over analysis data ad_bw / ad_fw.  frame(): blobs_* = per input frame blobs of the two vector clips.
    stats: "taps1" / "taps8" = luma samples with mF + mB >= 1 / >= 8, "luma" = luma samples of blurred frames, "max_taps"."""
    EXTRA = 2  # luma samples of padding that the stand-in has more than the real plane (even: chroma gets half of it at a ratio of 2)

    def __init__(self, ad_bw, ad_fw, num_frames, nplanes, hpad, vpad, blur=50.0, prec=1, thscd1=400, thscd2=130):
        kw = dict(blur=blur, prec=prec, thscd1=thscd1, thscd2=thscd2)
        self.ref = flowmc_ref.FlowBlur(ad_bw, ad_fw, num_frames, nplanes, hpad + self.EXTRA, vpad + self.EXTRA, POSITION_BITS, **kw)
        self.real = flowmc_ref.FlowBlur(ad_bw, ad_fw, num_frames, nplanes, hpad, vpad, POSITION_BITS, **kw)
        self._geometry(hpad, vpad)

    def frame(self, n, clip, sup, blobs_bw, blobs_fw, stats=None):
        fins, taps = {}, {}

        def stand_in(k):
            fins[k] = self.finest(sup(k))
            shifts = [np.subtract(self.ref._planes(p)[4], self.real._planes(p)[4]) for p in range(len(fins[k]))]
            taps[k] = [Taps((f.shape[0] + 2 * s[0], f.shape[1] + 2 * s[1])) for f, s in zip(fins[k], shifts)]
            return taps[k]
        self.ref.frame(n, {n: _dummy(clip[n])}, stand_in, blobs_bw, blobs_fw)
        self.last_kind = self.ref.last_kind
        if self.last_kind == "copy":
            return [bits(p).copy().view(F) for p in clip[n][:self.ref.nplanes]]
        out = []
        for p in range(self.ref.nplanes):
            shift = np.subtract(self.ref._planes(p)[4], self.real._planes(p)[4])
            assert (shift > 0).all()
            o, count = blur_sum(fins[n][p], taps[n][p].reads, shift)
            out.append(o)
            if stats is not None and p == 0:
                stats["luma"] = stats.get("luma", 0) + count.size
                stats["taps1"] = stats.get("taps1", 0) + int(np.count_nonzero(count >= 1))
                stats["taps8"] = stats.get("taps8", 0) + int(np.count_nonzero(count >= 8))
                stats["max_taps"] = max(stats.get("max_taps", 0), int(count.max()))
        return out
