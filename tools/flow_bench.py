"""Times mvx_flow_frames (mv.FlowFPS) on the GPU with device events, the super frames and vector blobs resident.

    python tools/flow_bench.py [--frames N] [--warmup W]

Workloads: FlowFPS 2x and 24 -> 60, mask=2, at 1080p 8-bit and 4K 16-bit 4:2:0.  Per workload: output fps, ms per output frame,
algorithmic bytes per output frame (3 x the output frame: its write plus one read of each of the two input frames it lies between) and
frac = those bytes per second over 8.0 TB/s.  Kernel times come from a separate rocprofv3 --kernel-trace --stats run of this script.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vapoursynth-mvtools_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import mvtools_amd as mv  # noqa: E402
import pipeline as pl  # noqa: E402

PEAK = 8.0e12


def workload(w, h, bits, num, frames, warmup, nin=4):
    import torch
    clip = pl.moving_clip(w, h, bits, nin, seed=5)
    sup = mv.Super(w, h, bits)
    src = [mv.frame_to_device(f) for f in clip]
    sf = sup.build(src)
    akw = dict(blksize=16, overlap=8) if w > 2000 else dict(blksize=8, overlap=4)
    abw, afw = mv.Analyse(sup, num_frames=nin, isb=1, **akw), mv.Analyse(sup, num_frames=nin, isb=0, **akw)
    bbw = abw.run([(sf[n], sf[n + 1] if n + 1 < nin else None) for n in range(nin)])
    bfw = afw.run([(sf[n], sf[n - 1] if n >= 1 else None) for n in range(nin)])
    fl = mv.FlowFPS(sup, abw.ad, afw.ad, nin, [p.stride(0) for p in src[0]], 24, 1, num=num, den=1, mask=2)
    # output frames strictly inside the middle input interval (1, 2): both extra blobs usable -> the Extra formula, no copies
    inner = [n for n in range(fl.num_frames) if fl.map(n)[0] == 1 and fl.map(n)[2] not in (0, 256)]
    ns = [inner[k % len(inner)] for k in range(frames)]
    out = fl.run(ns[:warmup], src, sf, bbw, bfw)
    out = mv.arena_frames(frames, [tuple(p.shape) for p in src[0]], src[0][0].device, zero=False)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    arr, out = fl.jobs(ns, src, sf, bbw, bfw, out=out)  # the job table is built on the host outside the timed interval
    fl.launch(arr)  # warm-up of the timed shape
    torch.cuda.synchronize()
    e0.record()
    fl.launch(arr)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    bps = (bits + 7) // 8
    frame_bytes = w * h * bps * 3 // 2
    alg = 3 * frame_bytes
    per = ms / frames
    frac = alg / (per * 1e-3) / PEAK
    name = "flowfps %s %dx%d %d-bit 4:2:0 mask=2" % ("2x" if num == 48 else "24->%d" % num, w, h, bits)
    print("%-44s frames=%d  %.1f fps  %.4f ms/frame  alg_bytes/frame=%d  frac=%.3f  time256=%s" % (
        name, frames, 1000.0 / per, per, alg, frac, sorted(set(fl.map(n)[2] for n in inner))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--only", default=None, help="run one workload: 1080p8 or 4k16 (counter passes)")
    a = ap.parse_args()
    for (w, h, bits, tag) in ((1920, 1080, 8, "1080p8"), (3840, 2160, 16, "4k16")):
        for num in (48, 60):
            if a.only in (None, tag) and (a.only is None or num == 48):
                workload(w, h, bits, num, a.frames, a.warmup)


if __name__ == "__main__":
    main()
