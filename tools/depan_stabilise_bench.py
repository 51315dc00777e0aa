"""Times mvx_depan_stabilise_frames (mv.DepanStabilise) on the GPU with device events, the source and output frames resident, beside
mvx_depan_compensate_frames (mv.DepanCompensate) for the same form in the same run, and the host planner with a wall clock.

    python tools/depan_stabilise_bench.py [--jobs N] [--seconds S] [--shapes 1080p8,4k16] [--out FILE]

Workload: 4:2:0 at 1920 x 1080 8-bit and 3840 x 2160 16-bit, a batch of N = 16 jobs per call, every job writing its own output frame,
mirror 15.  Two modes per interpolator (nearest, bilinear, bicubic) x form (translation, zoom, rotation):
  prev=next=0   the job is DepanCompensate's pass with the same transform; the DepanCompensate line is that filter on the same transform
  prev=next=1   the current frame's transform leaves a border of a few per cent (a shift of 1.5 % of the width and 2 % of the height on top of
                the form), filled from a next and a prev source, each another resident frame under a transform of its own
Per line: output frames per second, ms per call, and the share of output samples that the current frame does not cover.  The call is
repeated until about S seconds have passed between the two events.  The rotation form includes its pre-pass.  Kernel times come from a
separate rocprofv3 --kernel-trace --stats run of this script.
The planner: microseconds per output frame of mvx_depan_stabilise_plan (no device) over a 200-frame track, both methods.

    python tools/depan_stabilise_bench.py --float [--jobs N] [--seconds S] [--rounds R] [--out FILE]

The float path (sample_float=True) beside the 16-bit path at 1920 x 1080 4:2:0 with prev = next = 1 (the border filled from both sources), in
one process on the same plans -- rotation for nearest and bilinear, zoom for bicubic -- alternating the two filters round by round: ms per
frame and GB/s of the algorithm's bytes (the current frame read once, the output written once; the fill sources' few per cent are not
counted), median with the smallest and largest round.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vapoursynth-mvtools_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import mvtools_amd as mv  # noqa: E402

SHAPES = {"1080p8": (1920, 1080, 8), "4k16": (3840, 2160, 16)}
FORMS = {"translation": [3.3, 1.0, 0.0, -2.7, 0.0, 1.0], "zoom": [3.3, 1.004, 0.0, -2.7, 0.0, 1.004],
         "rotation": [4.2, 1.0029, -0.0123, -3.3, 0.0123, 1.0029]}


def shifted(tr, dx, dy):
    t = list(tr)
    t[0] += dx
    t[3] += dy
    return t


def timed(launch, seconds):
    import torch
    launch()  # warm-up of the timed shape: code objects and the handle's buffers
    torch.cuda.synchronize()
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
    return e0.elapsed_time(e1) / reps, reps


def float_beside_16(a):
    import torch
    w, h = 1920, 1080
    rng = np.random.default_rng(5)
    shapes = ((h, w), (h // 2, w // 2), (h // 2, w // 2))
    clips = {"16-bit": ([mv.frame_to_device([rng.integers(0, 1 << 16, s).astype(np.uint16) for s in shapes]) for _ in range(3)], dict(bits=16), 2),
             "float ": ([mv.frame_to_device([(rng.random(s, dtype=np.float32) * 1.5 - 0.25).astype(np.float32) for s in shapes]) for _ in range(3)],
                        dict(bits=32, sample_float=True), 4)}
    lines = []
    for sub, name, form in ((0, "nearest", "rotation"), (1, "bilinear", "rotation"), (2, "bicubic", "zoom")):
        base = FORMS[form]
        plan = mv.DepanStabilisePlan()
        plan.tr[:] = shifted(base, 0.015 * w, 0.02 * h)
        plan.next.used, plan.next.frame = 1, 1
        plan.next.tr[:] = shifted(base, -0.01 * w, 0.01 * h)
        plan.prev.used, plan.prev.frame = 1, 2
        plan.prev.tr[:] = shifted(base, 0.0, -0.01 * h)
        side = {}
        for key, (src, kw, bps) in clips.items():
            g = mv.DepanStabilise(w, h, src_pitch=[t.stride(0) for t in src[0]], subpixel=sub, mirror=15, prev=1, next=1, num_frames=3, **kw)
            arr, out = g.jobs([plan] * a.jobs, [src[0]] * a.jobs, [src[2]] * a.jobs, [src[1]] * a.jobs)
            g.launch(arr)  # warm-up of the timed shape
            torch.cuda.synchronize()
            side[key] = (g, arr, out, 2 * (w * h * 3 // 2) * bps, [])
        for _ in range(a.rounds):
            for key, (g, arr, out, moved, ms) in side.items():
                ms.append(timed(lambda: g.launch(arr), a.seconds)[0] / a.jobs)
        for key, (g, arr, out, moved, ms) in side.items():
            lo, med, hi = min(ms), float(np.median(ms)), max(ms)
            lines.append("stabilise %-8s %-8s prev=next=1 %s %dx%d 4:2:0  jobs/call=%d rounds=%d  %.4f ms/frame (%.4f .. %.4f)  moved=%d B/frame  %.1f GB/s (%.1f .. %.1f)" % (
                name, form, key, w, h, a.jobs, a.rounds, med, lo, hi, moved, moved / med / 1e6, moved / hi / 1e6, moved / lo / 1e6))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--shapes", default="1080p8,4k16")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--float", dest="float_", action="store_true", help="the float path beside the 16-bit path at 1080p, alternating")
    ap.add_argument("--rounds", type=int, default=5, help="--float: rounds per filter")
    a = ap.parse_args()
    if a.float_:
        return float_beside_16(a)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for shape in a.shapes.split(","):
        w, h, bits = SHAPES[shape]
        rng = np.random.default_rng(5)
        dt = np.uint16 if bits > 8 else np.uint8
        src = [mv.frame_to_device([rng.integers(0, 1 << bits, s).astype(dt) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]) for _ in range(3)]
        pitch = [t.stride(0) for t in src[0]]
        for sub, name in enumerate(("nearest", "bilinear", "bicubic")):
            comp = mv.DepanCompensate(w, h, bits, src_pitch=pitch, offset=1.0, subpixel=sub, mirror=15)
            for fill in (0, 1):
                g = mv.DepanStabilise(w, h, bits, src_pitch=pitch, subpixel=sub, mirror=15, prev=fill, next=fill, num_frames=3)
                for form, base in FORMS.items():
                    tr = shifted(base, 0.015 * w, 0.02 * h) if fill else base
                    plan = mv.DepanStabilisePlan()
                    plan.tr[:] = tr
                    if fill:
                        plan.next.used, plan.next.frame = 1, 1
                        plan.next.tr[:] = shifted(base, -0.01 * w, 0.01 * h)
                        plan.prev.used, plan.prev.frame = 1, 2
                        plan.prev.tr[:] = shifted(base, 0.0, -0.01 * h)
                    arr, out = g.jobs([plan] * a.jobs, [src[0]] * a.jobs, [src[2]] * a.jobs, [src[1]] * a.jobs)
                    ms, reps = timed(lambda: g.launch(arr), a.seconds)
                    carr, cout = comp.jobs([src[0]] * a.jobs, [tr] * a.jobs)
                    cms, _ = timed(lambda: comp.launch(carr), a.seconds)
                    border = 1.0 - max(0.0, 1 - abs(tr[0]) / w) * max(0.0, 1 - abs(tr[3]) / h)
                    say("stabilise %-8s %-11s prev=next=%d %dx%d %d-bit 4:2:0  jobs/call=%d calls=%d  %.0f fps  %.4f ms/call  border=%.1f%%  | DepanCompensate, same transform: %.0f fps  %.4f ms/call  ratio=%.3f" % (
                        name, form, fill, w, h, bits, a.jobs, reps, a.jobs * 1000.0 / ms, ms, border * 100, a.jobs * 1000.0 / cms, cms, cms / ms))
                    del out, cout
                del g
            del comp
    # the planner on the host
    n = 200
    rng = np.random.default_rng(7)
    motions = [(float(rng.normal(0, 3)), float(rng.normal(0, 3)), float(1 + rng.normal(0, 0.004)), float(rng.normal(0, 0.3))) for _ in range(n)]
    for method in (0, 1):
        for addzoom in (0, 1):
            g = mv.DepanStabilise(1920, 1080, num_frames=n, method=method, addzoom=addzoom, prev=2, next=2)
            windows = [g.window(k) for k in range(n)]
            t = time.perf_counter()
            for k in range(n):
                g.plan(k, motions[windows[k][0]:windows[k][1] + 1])
            us = (time.perf_counter() - t) * 1e6 / n
            say("stabilise planner method=%d addzoom=%d fps=25 cutoff=1.0: %.1f us/frame through the Python binding (window of up to %d data frames)" % (
                method, addzoom, us, max(b - f + 1 for f, b, _, _ in windows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
