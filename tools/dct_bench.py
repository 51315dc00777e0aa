"""Times mv.Analyse under three luma costs on the same clip: dct=0 (SAD, the default search's kernels), dct=5 (SATD, the generic SATD build) and
dct=1 (the float block DCT of csrc/mvx_dct_block.h, the generic dct 1..4 build).

    python tools/dct_bench.py [--jobs N] [--seconds S] [--blk 8,16] [--dcts 0,5,1]

Workload: 1920 x 1080 8-bit 4:2:0, pel 2, blocks of 8 or 16 overlapping by half, a batch of N chains (frame pairs) per mvx_analyse_frames call with the
super frames resident.  Device events around whole calls; every configuration is first launched on a batch of four chains (code objects, tables),
then once at full size, timed -- that launch decides how many more fit S seconds; a configuration whose single launch is longer than S is reported
from that one launch.  fps = chains per second.  dct 1..4 are opt-in: the tool switches them on (mv.enable_dct_float)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vapoursynth-mvtools_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import mvtools_amd as mv  # noqa: E402
import pipeline as pl  # noqa: E402

W, H = 1920, 1080


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--blk", default="8,16")
    ap.add_argument("--dcts", default="0,5,1")
    a = ap.parse_args()
    mv.enable_dct_float(True)
    nin = 5
    clip = pl.moving_clip(W, H, 8, nin, seed=5)
    sup = mv.Super(W, H, 8)
    sf = sup.build([mv.frame_to_device(f) for f in clip])
    pairs = [(sf[k % (nin - 1)], sf[k % (nin - 1) + 1]) for k in range(a.jobs)]
    print("Analyse %dx%d 8-bit 4:2:0 pel=2, %d chains per call" % (W, H, a.jobs), flush=True)
    for blk in [int(b) for b in a.blk.split(",")]:
        base = None
        for dct in [int(d) for d in a.dcts.split(",")]:
            an = mv.Analyse(sup, blksize=blk, overlap=blk // 2, dct=dct)
            blobs = an.alloc_blobs(a.jobs)
            an.run(pairs[:4], blobs[:4])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            an.run(pairs, blobs)
            e1.record()
            torch.cuda.synchronize()
            first = e0.elapsed_time(e1)
            reps = int(a.seconds * 1e3 / first)
            ms = first
            if reps >= 2:
                e0.record()
                for _ in range(reps):
                    an.run(pairs, blobs)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / reps
            fps = a.jobs * 1000.0 / ms
            base = base or fps
            print("blksize=%-2d overlap=%-2d dct=%d  %9.1f fps  %10.2f ms/call  calls timed=%d  x%.4f of the first row" % (blk, blk // 2, dct, fps, ms, max(reps, 1), fps / base), flush=True)


if __name__ == "__main__":
    main()
