"""Numpy restatement of mv.FlowInter and mv.FlowFPS on float clips (mvx_flowinter_create_float, mvx_flowfps_create_float), test
infrastructure: written from the table in include/mvtools_amd.h, not from the kernel.

Nothing above the sample is restated here.  tests/flow_ref.py decides which jobs are usable and which formula a job takes, builds the padded
small fields and the occlusion masks, upsizes both and forms the fetch positions: its Flow.frame runs as it is, and only the one function it
calls per plane, flow_inter, is replaced while it runs (flow_ref.py itself is not edited).  The replacement gets the integer restatement's
full-resolution vectors and masks and asks the ORIGINAL flow_inter where it reads: run on planes whose "sample" at (row, column) is its own
flat position (flowmc_float_ref.Positions), its probe returns, per output sample, the positions of dF and dB -- of dFF and dBB when it is
handed the extra vectors, of dF0 and dB0 when it is handed zero vectors.  The float samples at those positions then go through the table,
np.float32 operation by operation:
  mix(m, p, q)   ((float)m * p + (float)(255 - m) * q) / 255
  time(r, l, t)  (r * (float)t + l * (float)(256 - t)) * (1 / 256)
  Simple         time(mix(mB, dF, dB), mix(mF, dB, dF), t) at every t: no special formula at 128
  Regular        a = mix(mF, mix(mB, dF0, dB), dF); b = mix(mB, mix(mF, dB0, dF), dB); time(b, a, t)
  Extra          lo = min(dB, dF), hi = max(dB, dF), medBB = max(lo, min(dBB, hi)), medFF likewise;
                 time(mix(mB, medFF, dB), mix(mF, medBB, dF), t)          (min / max: comparisons that give the second operand on a tie)
  blend          time(r, l, t) on the clip frames;  left / copy: the clip frame's bits
The float Finest plane is the float super frame of tests/super_float_ref.py with its sub-pel planes interleaved (flowmc_float_ref.finest).
tests/test_flow_float_ref.py anchors all of it to tests/flow_ref.py on integer-valued clips."""
import numpy as np

import blockfps_float_ref as bf
import flow_ref
import flowmc_float_ref as ff

F = np.float32
bits = ff.bits


def simple(t, dF, dB, mF, mB):
    return bf.time_(bf.mix(mB, dF, dB), bf.mix(mF, dB, dF), t)


def regular(t, dF, dB, dF0, dB0, mF, mB):
    a, b = bf.mix(mF, bf.mix(mB, dF0, dB), dF), bf.mix(mB, bf.mix(mF, dB0, dF), dB)
    return bf.time_(b, a, t)


def extra(t, dF, dB, dFF, dBB, mF, mB):
    lo, hi = bf.fmin(dB, dF), bf.fmax(dB, dF)
    medBB, medFF = bf.fmax(lo, bf.fmin(dBB, hi)), bf.fmax(lo, bf.fmin(dFF, hi))
    return bf.time_(bf.mix(mB, medFF, dB), bf.mix(mF, medBB, dF), t)


def blend(t, l, r):
    return bf.time_(np.asarray(r, F), np.asarray(l, F), t)


_original = flow_ref.flow_inter


def _reads(t, fin_b, fin_f, off, pel, vb, vf, mb, mf, w, h):
    """where the integer restatement reads for the vectors vb / vf: (positions in fin_f, positions in fin_b, MF, MB)"""
    probe = {}
    _original("simple", t, ff.Positions(fin_b.shape), ff.Positions(fin_f.shape), off, pel, vb, vf, mb, mf, w, h, np.int64, probe=probe)
    return probe["dF"][0], probe["dB"][0], probe["MF"][0], probe["MB"][0]


class _Inter:
    """stands in for flow_ref.flow_inter while a float frame is made: same arguments, a float32 plane out.  probe collects per plane "kind",
    "t", "MF", "MB", "dF", "dB" and, for 'extra', "dFF" / "dBB" (float32 planes)"""

    def __init__(self, probe):
        self.probe = probe

    def __call__(self, kind, t, fin_b, fin_f, off, pel, vb, vf, mb, mf, w, h, dtype, vbb=None, vff=None, probe=None):
        pF, pB, MF, MB = _reads(t, fin_b, fin_f, off, pel, vb, vf, mb, mf, w, h)
        dF, dB = ff.gather(fin_f, pF), ff.gather(fin_b, pB)
        seen = dict(kind=kind, t=t, MF=MF, MB=MB, dF=dF, dB=dB)
        with np.errstate(invalid="ignore", over="ignore"):
            if kind == "simple":
                out = simple(t, dF, dB, MF, MB)
            elif kind == "regular":
                zero = (np.zeros_like(vf[0]), np.zeros_like(vf[1]))
                p0F, p0B, _, _ = _reads(t, fin_b, fin_f, off, pel, zero, zero, mb, mf, w, h)
                out = regular(t, dF, dB, ff.gather(fin_f, p0F), ff.gather(fin_b, p0B), MF, MB)
            else:
                pFF, pBB, _, _ = _reads(t, fin_b, fin_f, off, pel, vbb, vff, mb, mf, w, h)
                dFF, dBB = ff.gather(fin_f, pFF), ff.gather(fin_b, pBB)
                seen.update(dFF=dFF, dBB=dBB)
                out = extra(t, dF, dB, dFF, dBB, MF, MB)
        assert out.dtype == F and out.shape == (h, w)
        if self.probe is not None:
            for k, v in seen.items():
                self.probe.setdefault(k, []).append(v)
        return out


class Flow:
    """FlowInter (fps=None) / FlowFPS with sample_float=True over analysis data ad_bw / ad_fw; the arguments are flow_ref.Flow's.
    frame(): clip = the float frames, sup = callable k -> float super frame k (planes as super_float_ref.frame gives them), blobs_* = per
    input frame blobs of the two vector clips.  Sets last_kind as flow_ref.Flow does."""

    def __init__(self, ad_bw, ad_fw, num_frames, nplanes, hpad, vpad, **kw):
        self.ref = flow_ref.Flow(ad_bw, ad_fw, num_frames, nplanes, hpad, vpad, **kw)
        a = self.ref.bw
        self.geo = dict(width=a.nWidth, height=a.nHeight, sub=(a.xRatioUV >> 1, a.yRatioUV >> 1), gray=nplanes == 1, hpad=hpad, vpad=vpad, pel=a.nPel)
        self.num_frames = self.ref.num_frames

    def map(self, n):
        return self.ref.map(n)

    def frame(self, n, clip, sup, blobs_bw, blobs_fw, probe=None):
        ref = self.ref
        dummy = [[np.zeros(p.shape, np.int64) for p in fr] for fr in clip]
        flow_ref.flow_inter = _Inter(probe)
        try:
            out = ref.frame(n, dummy, lambda k: ff.finest(sup(k), **self.geo), blobs_bw, blobs_fw)
        finally:
            flow_ref.flow_inter = _original
        self.last_kind = kind = ref.last_kind
        nl, nr, t = ref.map(n)
        last = ref.in_frames - 1
        L, R = clip[min(nl, last)][:ref.nplanes], clip[min(nr, last)][:ref.nplanes]
        if kind == "copy":
            return [bits(p).copy().view(F) for p in (L if t == 0 else R)]
        if kind == "left":
            return [bits(p).copy().view(F) for p in L]
        if kind == "blend":
            return [blend(t, l, r) for l, r in zip(L, R)]
        return out
