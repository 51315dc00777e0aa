"""Times mvx_depan_compensate_frames (mv.DepanCompensate) on the GPU with device events, the source and output frames resident, and the
host estimator of mv.DepanAnalyse with a wall clock.

    python tools/depan_bench.py [--jobs N] [--seconds S] [--write-bw FILE] [--shapes 1080p8,4k16]

Workload: 4:2:0 at 1920 x 1080 8-bit and 3840 x 2160 16-bit, a batch of N = 16 jobs per mvx_depan_compensate_frames call, every job reading
the same source frame and writing its own output frame, mirror 15.  The call is repeated until about S seconds have passed between the two
events.  Per interpolator (nearest, bilinear, bicubic) x form (translation, zoom, rotation): output frames per second, ms per call, bytes
moved per second -- one read and one write of every plane, nothing else counted -- and that rate as a fraction of a write-bandwidth ceiling:
the "fill, linear 16 B/thread" line of tools/micro/write_bw.hip's output in FILE when given (run it in the same session), else the figure
recorded in profiles/r2_write_bw_microbench.txt.  The rotation form of nearest and bilinear includes its pre-pass.
The estimator: milliseconds per frame of mvx_depan_analyse_host (no device) on real vectors of the 1080p clip at 8/4 and 16/8 blocks.
Kernel times come from a separate rocprofv3 --kernel-trace --stats run of this script.

    python tools/depan_bench.py --float [--jobs N] [--seconds S] [--rounds R] [--out FILE]

The float path (sample_float=True) beside the 16-bit path at 1920 x 1080 4:2:0, in one process on the same transforms -- rotation for nearest
and bilinear, zoom for bicubic -- alternating the two filters round by round: ms per frame and GB/s of the algorithm's bytes (one read and
one write of every plane; the float path moves twice the 16-bit path's), median with the smallest and largest round.
"""
import argparse
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vapoursynth-mvtools_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import mvtools_amd as mv  # noqa: E402
import pipeline as pl  # noqa: E402

RECORDED = os.path.join(ROOT, "profiles", "r2_write_bw_microbench.txt")
SHAPES = {"1080p8": (1920, 1080, 8), "4k16": (3840, 2160, 16)}
FORMS = {"translation": [3.3, 1.0, 0.0, -2.7, 0.0, 1.0], "zoom": [3.3, 1.004, 0.0, -2.7, 0.0, 1.004],
         "rotation": [4.2, 1.0029, -0.0123, -3.3, 0.0123, 1.0029]}


def ceiling(path):
    """(bytes per second, where it came from) of the linear 16-byte fill"""
    src = path or RECORDED
    with open(src) as f:
        for line in f:
            m = re.match(r"fill, linear 16 B/thread.*?([0-9.]+) TB/s", line)
            if m:
                return float(m.group(1)) * 1e12, os.path.relpath(src, ROOT)
    raise SystemExit("no 'fill, linear 16 B/thread' line in " + src)


def timed(launch, seconds):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    torch.cuda.synchronize()
    reps = max(5, int(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)))
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def float_beside_16(a):
    """mvx_depan_compensate_frames on a float clip and on a 16-bit clip, alternating"""
    import torch
    w, h = 1920, 1080
    rng = np.random.default_rng(5)
    shapes = ((h, w), (h // 2, w // 2), (h // 2, w // 2))
    clips = {"16-bit": (mv.frame_to_device([rng.integers(0, 1 << 16, s).astype(np.uint16) for s in shapes]), dict(bits=16), 2),
             "float ": (mv.frame_to_device([(rng.random(s, dtype=np.float32) * 1.5 - 0.25).astype(np.float32) for s in shapes]), dict(bits=32, sample_float=True), 4)}
    lines = []
    for sub, name, form in ((0, "nearest", "rotation"), (1, "bilinear", "rotation"), (2, "bicubic", "zoom")):
        side = {}
        for key, (src, kw, bps) in clips.items():
            g = mv.DepanCompensate(w, h, src_pitch=[t.stride(0) for t in src], offset=1.0, subpixel=sub, mirror=15, **kw)
            arr, out = g.jobs([src] * a.jobs, [FORMS[form]] * a.jobs)
            g.launch(arr)  # warm-up of the timed shape: code objects and the handle's buffers
            torch.cuda.synchronize()
            side[key] = (g, arr, out, 2 * (w * h * 3 // 2) * bps, [])
        for _ in range(a.rounds):
            for key, (g, arr, out, moved, ms) in side.items():
                ms.append(timed(lambda: g.launch(arr), a.seconds) / a.jobs)
        for key, (g, arr, out, moved, ms) in side.items():
            lo, med, hi = min(ms), float(np.median(ms)), max(ms)
            lines.append("depan %-8s %-8s %s %dx%d 4:2:0  jobs/call=%d rounds=%d  %.4f ms/frame (%.4f .. %.4f)  moved=%d B/frame  %.1f GB/s (%.1f .. %.1f)" % (
                name, form, key, w, h, a.jobs, a.rounds, med, lo, hi, moved, moved / med / 1e6, moved / hi / 1e6, moved / lo / 1e6))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--float", dest="float_", action="store_true", help="the float path beside the 16-bit path at 1080p, alternating")
    ap.add_argument("--rounds", type=int, default=5, help="--float: rounds per filter")
    ap.add_argument("--out", default=None, help="--float: also write the lines to this file")
    ap.add_argument("--write-bw", default=None, help="output of tools/micro/write_bw.hip from the same session")
    ap.add_argument("--shapes", default="1080p8,4k16")
    a = ap.parse_args()
    if a.float_:
        return float_beside_16(a)
    peak, origin = ceiling(a.write_bw)
    print("ceiling: %.2f TB/s (linear 16-byte fill, %s)" % (peak / 1e12, origin), flush=True)
    for shape in a.shapes.split(","):
        w, h, bits = SHAPES[shape]
        rng = np.random.default_rng(5)
        dt = np.uint16 if bits > 8 else np.uint8
        frame = [rng.integers(0, 1 << bits, s).astype(dt) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
        src = mv.frame_to_device(frame)
        moved = 2 * (w * h * 3 // 2) * (2 if bits > 8 else 1)
        for sub, name in enumerate(("nearest", "bilinear", "bicubic")):
            g = mv.DepanCompensate(w, h, bits, src_pitch=[t.stride(0) for t in src], offset=1.0, subpixel=sub, mirror=15)
            for form, tr in FORMS.items():
                arr, out = g.jobs([src] * a.jobs, [tr] * a.jobs)
                g.launch(arr)  # warm-up of the timed shape: code objects and the handle's buffers
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.launch(arr)
                e1.record()
                torch.cuda.synchronize()
                reps = max(5, int(a.seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)))
                e0.record()
                for _ in range(reps):
                    g.launch(arr)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / reps
                rate = moved * a.jobs / (ms * 1e-3)
                print("depan %-8s %-11s %dx%d %d-bit 4:2:0  jobs/call=%d calls=%d  %.0f fps  %.4f ms/call  moved=%d B/frame  %.3f TB/s  frac=%.3f" % (
                    name, form, w, h, bits, a.jobs, reps, a.jobs * 1000.0 / ms, ms, moved, rate / 1e12, rate / peak), flush=True)
            del g, out
    # the estimator on the host
    nin = 3
    clip = pl.moving_clip(1920, 1080, 8, nin, seed=5)
    sup = mv.Super(1920, 1080, 8)
    sf = sup.build([mv.frame_to_device(f) for f in clip])
    for blk, ov in ((8, 4), (16, 8)):
        an = mv.Analyse(sup, num_frames=nin, isb=0, delta=1, blksize=blk, overlap=ov)
        blobs = [b.cpu().numpy() for b in an.run([(sf[n], sf[n - 1]) for n in range(1, nin)])]
        g = mv.DepanAnalyse(an.ad, 1920, 1080)
        g.run_host(blobs)
        reps = 5
        t = time.perf_counter()
        for _ in range(reps):
            res = g.run_host(blobs)
        ms = (time.perf_counter() - t) * 1e3 / (reps * len(blobs))
        print("depan estimator 1920x1080 blocks %d/%d (%d x %d)  %.3f ms/frame on the host  iter=%s dx=%.3f dy=%.3f" % (
            blk, ov, an.ad.nBlkX, an.ad.nBlkY, ms, [r["iter"] for r in res], res[0]["dx"], res[0]["dy"]), flush=True)


if __name__ == "__main__":
    main()
