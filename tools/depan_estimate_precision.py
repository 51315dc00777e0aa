"""Runs every case of tests/depan_estimate_cases.py through mv.DepanEstimate on the GPU and prints what the precision checks of
tests/depan_estimate_checks.py measure: per quantity D (the largest distance between the restatements with scipy's single-precision FFT and its
double one) and the GPU's largest distance from the double restatement; per window size the spectrum's relative L2 error against its bound.

    python tools/depan_estimate_precision.py > profiles/depan_estimate_precision.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vapoursynth-mvtools_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import mvtools_amd as mv  # noqa: E402
import depan_estimate_cases as dc  # noqa: E402
import depan_estimate_checks as ck  # noqa: E402


def main():
    D = ck.D()
    worst = {q: (0.0, "") for q in ck.QUANTITIES}
    print("spectrum: relative L2 error without the DC bin against scipy.fft.rfft2 in double (bound 2^-23 log2(winx winy)); DC bin alone (bound 2^-22 = %.3g)" % 2.0 ** -22)
    print("%-34s %10s %10s %10s %10s" % ("case", "GPU L2", "scipy f32", "bound", "GPU DC"))
    for c in dc.CASES:
        g = mv.DepanEstimate(c.width, c.height, c.bits, **c.kw)
        prev, cur = c.frames()
        sp = g.spectra([mv.plane_to_device(prev), mv.plane_to_device(cur)])
        res = g.correlate([sp[0]], [sp[1]], None if c.prop is None else [c.prop], [c.n])[0]
        e = c.ref()
        errs = ck.spectrum_errors(c, cur, sp[1].cpu().numpy())
        f32 = [np.stack([s.real, s.imag], -1) for s in e.spectra(cur, dc.er.FFT32)]
        ref = ck.spectrum_errors(c, cur, np.stack(f32))
        print("%-34s %10.3g %10.3g %10.3g %10.3g" % (c.name, max(x[0] for x in errs), max(x[0] for x in ref), errs[0][2], max(x[1] for x in errs)))
        for q, d in ck.distances(c, res).items():
            if d >= worst[q][0]:
                worst[q] = (d, c.name)
    print()
    print("dx, dy, zoom, trust: D = largest distance over all cases between the restatement with scipy's float32 FFT and with its float64 FFT;")
    print("GPU = the library's largest distance from the float64 restatement (must stay within 4 D)")
    print("%-6s %12s %12s %12s  %s" % ("", "D", "4 D", "GPU", "at"))
    for q in ck.QUANTITIES:
        print("%-6s %12.4g %12.4g %12.4g  %s" % (q, D[q], 4 * D[q], worst[q][0], worst[q][1]))


if __name__ == "__main__":
    main()
