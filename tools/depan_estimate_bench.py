"""Times mv.DepanEstimate on the GPU, frames resident: a walk over consecutive frames with one spectrum per frame (stage 1 once per frame, stage 2
once per pair), in batches of N frames.

    python tools/depan_estimate_bench.py [--frames N] [--seconds S]

Shapes: 1920 x 1080 8-bit (automatic window 1024 x 1024) and 3840 x 2160 16-bit (2048 x 2048), each without zoom and with zoommax = 1.2 (two
windows of half the width).  Per shape: milliseconds per frame and frames per second of the walk (a host clock around calls that end in a device
synchronise: stage 2 is synchronous), the same for stage 1 and stage 2 alone, the bytes each pass must move per frame -- every array it reads or
writes counted once -- and the time those bytes would take at the recorded HBM copy ceiling (6.29 TB/s) as a fraction of the measured
time.  Beside it the same pipeline on the CPU with scipy.fft in float32, workers=16, timed in the same run.  Kernel times come from a separate
rocprofv3 --kernel-trace --stats run of this script.
"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.fft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vapoursynth-mvtools_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import mvtools_amd as mv  # noqa: E402

HBM = 6.29e12
SHAPES = [("1080p 8-bit", 1920, 1080, 8, 1.0), ("1080p 8-bit zoom", 1920, 1080, 8, 1.2), ("4K 16-bit", 3840, 2160, 16, 1.0), ("4K 16-bit zoom", 3840, 2160, 16, 1.2)]


def pass_bytes(i, bits):
    """bytes per frame of each pass, all windows"""
    nx, w = i.winx // 2 + 1, i.windows
    nrows = min(i.winy, 2 * i.dymax + 3)
    area = (2 * i.dxmax + 1) * (2 * i.dymax + 1)
    spec = i.winy * nx * 8
    return [("rows forward", w * (i.winx * i.winy * (2 if bits > 8 else 1) + spec)), ("columns forward", w * 2 * spec),
            ("correlate + columns inverse", w * (2 * spec + nrows * nx * 8)), ("rows inverse", w * (nrows * nx * 8 + nrows * i.winx * 4)),
            ("peak", w * 2 * area * 4)]


def timed(fn, seconds):
    import torch
    fn()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        if t >= seconds:
            return t / n


def cpu_walk(frames, i, width):
    """the same pipeline with scipy.fft in float32: one spectrum per frame, product, inverse, the scan of the four corners"""
    lefts = [i.wleft] + ([i.wleft + width // 2] if i.windows == 2 else [])
    rows = np.r_[0:i.dymax + 1, i.winy - i.dymax:i.winy]
    cols = np.r_[0:i.dxmax + 1, i.winx - i.dxmax:i.winx]
    prev = None
    for f in frames:
        sp = [scipy.fft.rfft2(f[i.wtop:i.wtop + i.winy, l:l + i.winx].astype(np.float32), workers=16) for l in lefts]
        if prev is not None:
            for a, b in zip(sp, prev):
                s = scipy.fft.irfft2(np.conj(a) * b, s=(i.winy, i.winx), workers=16)
                area = s[np.ix_(rows, cols)]
                area.argmax(), area.sum(dtype=np.float32)
        prev = sp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=1.0)
    a = ap.parse_args()
    n = a.frames
    print("HBM ceiling: %.2f TB/s (the measured copy ceiling recorded in BASELINE.md); batches of %d frames" % (HBM / 1e12, n), flush=True)
    for name, w, h, bits, zoommax in SHAPES:
        rng = np.random.default_rng(3)
        frames = [rng.integers(0, 1 << bits, (h, w)).astype(np.uint16 if bits > 8 else np.uint8) for _ in range(n)]
        dev = [mv.plane_to_device(f) for f in frames]
        g = mv.DepanEstimate(w, h, bits, zoommax=zoommax, num_frames=1 << 20)
        i = g.info
        sp = g.spectra(dev)
        pairs = ([sp[max(0, k - 1)] for k in range(n)], sp)
        nums = list(range(1, n + 1))
        t1 = timed(lambda: g.spectra(dev), a.seconds) / n
        t2 = timed(lambda: g.correlate(pairs[0], pairs[1], None, nums), a.seconds) / n

        def walk():
            s = g.spectra(dev)
            g.correlate([s[max(0, k - 1)] for k in range(n)], s, None, nums)
        tw = timed(walk, a.seconds) / n
        t0 = time.perf_counter()
        cpu_walk(frames, i, w)
        reps = max(1, int(a.seconds / max(time.perf_counter() - t0, 1e-3)))
        t0 = time.perf_counter()
        for _ in range(reps):
            cpu_walk(frames, i, w)
        tc = (time.perf_counter() - t0) / reps / n
        pb = pass_bytes(i, bits)
        b1, b2 = sum(b for _, b in pb[:2]), sum(b for _, b in pb[2:])
        print("\n%s: %d window(s) of %d x %d, search area +-%d x +-%d" % (name, i.windows, i.winx, i.winy, i.dxmax, i.dymax))
        print("  walk   : %8.3f ms/frame  %9.1f frames/s   (CPU, scipy.fft float32, workers=16: %8.3f ms/frame  %8.1f frames/s)" % (tw * 1e3, 1 / tw, tc * 1e3, 1 / tc))
        print("  stage 1: %8.3f ms/frame  %6.1f MB/frame  = %5.1f %% of the HBM ceiling" % (t1 * 1e3, b1 / 1e6, 100 * b1 / HBM / t1))
        print("  stage 2: %8.3f ms/frame  %6.1f MB/frame  = %5.1f %% of the HBM ceiling" % (t2 * 1e3, b2 / 1e6, 100 * b2 / HBM / t2))
        for what, b in pb:
            print("    %-28s %8.2f MB/frame = %7.2f us at the ceiling" % (what, b / 1e6, b / HBM * 1e6))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
