"""What an implementation of DepanEstimate's transforms is held to, shared by the CPU test of the kernels' text compiled for the host
(tests/test_depan_estimate_host.py), the GPU test (tests/test_gpu_depan_estimate.py) and tools/depan_estimate_precision.py.  Test infrastructure.

An FFT in single precision cannot equal FFTW's bit for bit, so three things replace byte parity:
  1. the spectrum against scipy.fft.rfft2 in double: relative L2 error without the DC bin at most 2^-23 * log2(winx * winy), the usual bound of
     a radix FFT in single precision; the DC bin alone within 2^-22 (two roundings);
  2. the discrete results -- imax, jmax, the scene-change decision, the good-zoom branch, the frame-0 rule -- equal the restatement with the
     double FFT exactly: the cases' margins (tests/test_depan_estimate_ref.py) exceed any such FFT's error;
  3. dx, dy, zoom, trust within 4 * D of that restatement, D being the largest difference over all cases between the restatements with scipy's
     single-precision FFT and with its double one: computed here, never taken from the code under test."""
import functools
import math

import numpy as np
import scipy.fft

import depan_estimate_cases as dc

QUANTITIES = ("dx", "dy", "zoom", "trust")


def spectrum_errors(case, frame, spec):
    """spec: float32 [windows, winy, nx, 2] of `frame` -> per window (relative L2 error without DC, relative error of DC, the L2 bound)"""
    e = case.ref()
    out = []
    for w in range(e.windows):
        want = scipy.fft.rfft2(e.window(frame, w).astype(np.float64))
        got = spec[w][..., 0].astype(np.float64) + 1j * spec[w][..., 1].astype(np.float64)
        d, ref = got - want, want.copy()
        dc_err = abs(d[0, 0]) / abs(want[0, 0])
        d[0, 0] = 0
        ref[0, 0] = 0
        out.append((float(np.sqrt((abs(d) ** 2).sum() / (abs(ref) ** 2).sum())), float(dc_err), 2.0 ** -23 * math.log2(e.winx * e.winy)))
    return out


def assert_spectrum(case, frame, spec):
    for l2, dc_err, bound in spectrum_errors(case, frame, spec):
        print("%s: spectrum relative L2 error %.3g (bound %.3g), DC %.3g (bound %.3g)" % (case.name, l2, bound, dc_err, 2.0 ** -22))
        assert l2 <= bound and dc_err <= 2.0 ** -22


@functools.lru_cache(maxsize=None)
def D():
    """per quantity: the largest distance over all cases between the single-precision and the double restatement"""
    return {q: max(abs(float(c.result(32)[q]) - float(c.result(64)[q])) for c in dc.CASES) for q in QUANTITIES}


def assert_discrete(case, scans, result):
    """scans: per window a dict with imax, jmax; result: dict(dx, dy, zoom, trust) of stage 2"""
    want = case.result(64)
    e = case.ref()
    for w in range(e.windows):
        assert (scans[w]["imax"], scans[w]["jmax"]) == (want["scans"][w]["imax"], want["scans"][w]["jmax"])
    # the scene-change decision, the good-zoom branch and the frame-0 rule show in the zeros and ones they write
    assert (result["dx"] == 0) == (want["dx"] == 0) and (result["dy"] == 0) == (want["dy"] == 0) and (result["zoom"] == 1) == (want["zoom"] == 1)
    if case.claim == "frame0":
        assert (result["dx"], result["dy"], result["zoom"], result["trust"]) == (0, 0, 1, 0)


def distances(case, result):
    want = case.result(64)
    return {q: abs(float(result[q]) - float(want[q])) for q in QUANTITIES}


def assert_close(case, result):
    d, lim = distances(case, result), D()
    print("%s: " % case.name + ", ".join("%s off by %.3g (4 D = %.3g)" % (q, d[q], 4 * lim[q]) for q in QUANTITIES))
    for q in QUANTITIES:
        assert d[q] <= 4 * lim[q], q
