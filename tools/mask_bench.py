"""Times mvx_mask_frames (mv.Mask) on the GPU with device events, the vector blobs and the output frames resident.

    python tools/mask_bench.py [--jobs N] [--kinds 0,1,2,5] [--bits 8,16] [--seconds S] [--write-bw FILE]

Workload: 1920 x 1080 4:2:0 at each depth of --bits (8: mvx_mask_create; 9 to 16: the deep entry, mvx_mask_create_deep, on a clip of that depth,
two bytes a sample), vectors of 8/4 blocks (479 x 269), a batch of N = 64 jobs per mvx_mask_frames call, every job usable and
writing its own output frame.  The call is repeated until about S seconds have passed between the two events (one launch of 64 frames
lasts well under a millisecond, too short to time on its own).  Per kind: output frames per second, ms per call, bytes written per second
(the three output planes, width x height, nothing else counted; kind 5 also reads the clip's luma) and that rate as a fraction of a
write-bandwidth ceiling: the "fill, linear 16 B/thread" line of tools/micro/write_bw.hip's output in FILE when given (run it in the same
session), else the figure recorded in profiles/r2_write_bw_microbench.txt.  Kernel times come from a separate
rocprofv3 --kernel-trace --stats run of this script.
"""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vapoursynth-mvtools_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import mvtools_amd as mv  # noqa: E402
import pipeline as pl  # noqa: E402

W, H = 1920, 1080
RECORDED = os.path.join(ROOT, "profiles", "r2_write_bw_microbench.txt")


def ceiling(path):
    """(bytes per second, where it came from) of the linear 16-byte fill"""
    src = path or RECORDED
    with open(src) as f:
        for line in f:
            m = re.match(r"fill, linear 16 B/thread.*?([0-9.]+) TB/s", line)
            if m:
                return float(m.group(1)) * 1e12, os.path.relpath(src, ROOT)
    raise SystemExit("no 'fill, linear 16 B/thread' line in " + src)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=64)
    ap.add_argument("--kinds", default="0,1,2,5")
    ap.add_argument("--bits", default="8", help="clip depths, e.g. 8,16; above 8 through the deep entry")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--write-bw", default=None, help="output of tools/micro/write_bw.hip from the same session")
    a = ap.parse_args()
    peak, origin = ceiling(a.write_bw)
    print("ceiling: %.2f TB/s (linear 16-byte fill, %s)" % (peak / 1e12, origin), flush=True)
    for bits in [int(b) for b in a.bits.split(",")]:
        bench(torch, a, bits, peak)


def bench(torch, a, bits, peak):
    nin = 4
    clip = pl.moving_clip(W, H, bits, nin, seed=5)
    sup = mv.Super(W, H, bits)
    src = [mv.frame_to_device(f) for f in clip]
    sf = sup.build(src)
    an = mv.Analyse(sup, num_frames=nin, isb=1, blksize=8, overlap=4)
    blobs = an.run([(sf[n], sf[n + 1]) for n in range(nin - 1)])
    written = W * H * 3 // 2 * (2 if bits > 8 else 1)
    for kind in [int(k) for k in a.kinds.split(",")]:
        g = mv.Mask(an.ad, W, H, kind=kind, clip_pitch=[src[0][0].stride(0)], bits=bits, deep=bits > 8)
        ks = [k % (nin - 1) for k in range(a.jobs)]
        arr, out = g.jobs([blobs[k] for k in ks], [src[k] for k in ks] if kind == 5 else None)
        g.launch(arr)  # warm-up of the timed shape: code objects, the handle's buffers and tables
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.launch(arr)
        e1.record()
        torch.cuda.synchronize()
        reps = max(10, int(a.seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)))
        e0.record()
        for _ in range(reps):
            g.launch(arr)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        rate = written * a.jobs / (ms * 1e-3)
        print("mask kind=%d %dx%d %d-bit 4:2:0  jobs/call=%d calls=%d  %.0f fps  %.4f ms/call  written=%d B/frame  %.3f TB/s written  frac=%.3f" % (
            kind, W, H, bits, a.jobs, reps, a.jobs * 1000.0 / ms, ms, written, rate / 1e12, rate / peak), flush=True)


if __name__ == "__main__":
    main()
