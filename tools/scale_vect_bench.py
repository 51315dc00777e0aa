"""Times mv.ScaleVect on one GPU with device events / the wall clock, everything resident:

  1. the kernel (mvx_scale_vect_frames, one launch) on the blobs of 341 4K frames of Degrain3 -- 2046 blobs of a 1080p 8-bit search with blocks of
     8 overlapping by 4, scaled by 2 to 4K 16-bit -- against a device-to-device copy of the same buffer in the same run: the yardstick of a kernel
     that only streams.  Out of place and in place.
  2. the chain  Super(1080p 8-bit) -> Analyse(blocks 8 / 4) -> ScaleVect(2, the 4K 16-bit super clip) -> Recalculate(4K 16-bit, blocks 16 / 8, thsad
     default) -> Degrain3  against the direct 4K 16-bit  Super -> Analyse(blocks 16 / 8) -> Degrain3  of bench.py's headline (bench.Pipeline, the same
     clip), both as frames per second over a resident batch with ONE batch in flight.  The chain's step includes both Super passes; the small clip
     itself (a resize of the full-size clip, which is not this library's business) is resident like the full-size one.

    python tools/scale_vect_bench.py [--batch 341] [--steps 3] [--repeats 3] [--seconds 0.5] [--no-chain]
"""
import argparse
import gc
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vapoursynth-mvtools_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import bench  # noqa: E402
import mvtools_amd as mv  # noqa: E402
import pipeline as pl  # noqa: E402
from compensate_n_bench import stream, timed  # noqa: E402

SMALL = (1920, 1080, 8, dict(blksize=8, overlap=4))
FULL = bench.CONFIGS["cfg3"]   # 3840 x 2160, 16 bit, Degrain3, blocks 16 / 8, pel 2


def kernel_part(a):
    import torch
    L = mv.lib()
    w, h, bits, akw = SMALL
    n = a.batch * 2 * FULL[3]
    ssup = mv.Super(w, h, bits)
    tsup = mv.Super(FULL[0], FULL[1], FULL[2], **FULL[5])
    sf = ssup.build([mv.frame_to_device(f) for f in pl.moving_clip(w, h, bits, 3, seed=5)])
    an = mv.Analyse(ssup, isb=1, **akw)
    seed = an.run([(sf[1], sf[2]), (sf[1], sf[0])])
    sv = mv.ScaleVect(an.ad, tsup, 2)
    stride = (an.blob_size + 255) // 256 * 256
    src = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
    for i in range(2):  # real vectors, repeated: the kernel's work does not depend on the values
        src[i::2, :an.blob_size] = seed[i]
    dst, work = torch.zeros_like(src), src.clone()
    arr, arr_in = (mv.ScaleVectJob * n)(), (mv.ScaleVectJob * n)()
    for i in range(n):
        arr[i].in_, arr[i].out, arr[i].fields = src[i].data_ptr(), dst[i].data_ptr(), 1
        arr_in[i].in_ = arr_in[i].out = work[i].data_ptr()
        arr_in[i].fields = 1

    def run(table):
        def go():
            if L.mvx_scale_vect_frames(sv.h, n, table, stream()):
                raise SystemExit(L.mvx_last_error().decode())
        return go

    lines = [("(a) device-to-device copy of the buffer", lambda: dst.copy_(src)), ("(b) mvx_scale_vect_frames, out of place", run(arr)),
             ("(c) mvx_scale_vect_frames, in place", run(arr_in))]
    moved = 2.0 * n * an.blob_size
    print("kernel: %d blobs of %d bytes (%d x %d %d-bit, blocks %d/%d, %d levels; the blobs of %d 4K frames of Degrain%d), scale 2 to %d x %d %d-bit; "
          "%.2f GB read + written per call; %d repeats in turn; ms per call" % (
              n, an.blob_size, w, h, bits, akw["blksize"], akw["overlap"], an.ad.nLvCount, a.batch, FULL[3], FULL[0], FULL[1], FULL[2], moved / 1e9, a.repeats), flush=True)
    ms = [[] for _ in lines]
    for _ in range(a.repeats):
        for k, (_, fn) in enumerate(lines):
            ms[k].append(timed(fn, a.seconds))
    for (name, _), m in zip(lines, ms):
        print("  %-44s %s  min %.3f  spread %.3f  %.0f GB/s at the minimum" % (name, "  ".join("%.3f" % v for v in m), min(m), max(m) - min(m), moved / min(m) / 1e6), flush=True)
    print("  (b) / (a) = %.2f, (c) / (a) = %.2f at the minima" % (min(ms[1]) / min(ms[0]), min(ms[2]) / min(ms[0])), flush=True)


class Chain:
    """search on the small clip, ScaleVect, Recalculate and Degrain at full size, over the frames of a bench.Pipeline's plan"""

    def __init__(self, torch, direct, small_src):
        self.torch, self.d = torch, direct
        w, h, bits, akw = SMALL
        dev = direct.device
        self.small_src = small_src
        self.ssup = mv.Super(w, h, bits)
        self.ssupers = self.ssup.alloc(direct.n, device=dev)
        self.san = mv.Analyse(self.ssup, isb=1, **akw)
        self.sv = mv.ScaleVect(self.san.ad, direct.sup, 2)
        self.rc = mv.Recalculate(direct.sup, self.sv.ad, blksize=FULL[4]["blksize"], overlap=FULL[4]["overlap"])
        self.dg = mv.Degrain(direct.tr, direct.sup, self.rc.ad, [p.stride(0) for p in direct.src[0]])
        nb = len(direct.plan.clips) * direct.B
        self.small_blobs, self.scaled = self.san.alloc_blobs(nb, device=dev), self.san.alloc_blobs(nb, device=dev)
        stride = (self.rc.blob_size + 255) // 256 * 256
        buf = torch.zeros((nb, stride), dtype=torch.uint8, device=dev)
        self.blobs = [buf[i, :self.rc.blob_size] for i in range(nb)]

    def step(self):
        d = self.d
        bench._order_behind_caller(self.torch, d.stream, d.device)
        with self.torch.cuda.stream(d.stream):
            self.ssup.build(self.small_src, out=self.ssupers)
            d.sup.build(d.src, out=d.supers)
            pairs = [pr for key in d.plan.clips for pr in d.plan.searches()[key]]
            self.san.run([(self.ssupers[n], self.ssupers[r] if r is not None else None) for n, r in pairs], blobs=self.small_blobs)
            self.sv.run(self.small_blobs, out=self.scaled)
            self.rc.run([(d.supers[n], d.supers[r] if r is not None else None, b) for (n, r), b in zip(pairs, self.scaled)], blobs=self.blobs)
            B = d.B
            djobs = [(d.src[n], [d.supers[r] if r is not None else None for r in refs], [self.blobs[k * B + i] for k in range(len(d.plan.clips))])
                     for n, refs, i in d.plan.degrains()]
            self.dg.run(djobs, out=d.out)


def fps(torch, step, steps, frames):
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return frames * steps / (time.perf_counter() - t0)


def chain_part(a):
    import torch
    device = torch.device("cuda", 0)
    direct = bench.Pipeline(mv, torch, FULL, a.batch, device, seed=1000)
    w, h, bits, _ = SMALL
    small_src = bench.synth_clip_device(torch, w, h, bits, direct.n, 1000, device)
    chain = Chain(torch, direct, small_src)
    torch.cuda.synchronize()
    print("chain: %s, batch %d resident, one batch in flight, %d timed steps after one warm-up, %d repeats in turn; frames per second" % (FULL[7], a.batch, a.steps, a.repeats), flush=True)
    lines = [("(d) direct: Super -> Analyse 16/8 -> Degrain3 at 4K 16-bit", direct.step),
             ("(e) chain: Super x 2 -> Analyse 8/4 at 1080p 8-bit -> ScaleVect -> Recalculate 16/8 -> Degrain3", chain.step)]
    v = [[] for _ in lines]
    for _ in range(a.repeats):
        for k, (_, fn) in enumerate(lines):
            v[k].append(fps(torch, fn, a.steps, a.batch))
    for (name, _), m in zip(lines, v):
        print("  %-100s %s  max %.1f  spread %.1f" % (name, "  ".join("%.1f" % x for x in m), max(m), max(m) - min(m)), flush=True)
    print("  (e) / (d) = %.2f at the maxima" % (max(v[1]) / max(v[0])), flush=True)
    # where the chain's step goes: each stage alone, by device events
    d = direct
    pairs = [pr for key in d.plan.clips for pr in d.plan.searches()[key]]
    sjobs = [(chain.ssupers[n], chain.ssupers[r] if r is not None else None) for n, r in pairs]
    rjobs = [(d.supers[n], d.supers[r] if r is not None else None, b) for (n, r), b in zip(pairs, chain.scaled)]
    stages = [("Super 1080p 8-bit", lambda: chain.ssup.build(small_src, out=chain.ssupers)), ("Super 4K 16-bit", lambda: d.sup.build(d.src, out=d.supers)),
              ("Analyse 8/4 at 1080p 8-bit, %d chains" % len(pairs), lambda: chain.san.run(sjobs, blobs=chain.small_blobs)),
              ("ScaleVect, %d blobs" % len(pairs), lambda: chain.sv.run(chain.small_blobs, out=chain.scaled)),
              ("Recalculate 16/8 at 4K 16-bit, %d blobs" % len(pairs), lambda: chain.rc.run(rjobs, blobs=chain.blobs)),
              ("direct Analyse 16/8 at 4K 16-bit, %d chains" % len(pairs), lambda: d.an[(1, 1)].run(*d._search_jobs()))]
    with torch.cuda.stream(d.stream):
        for name, fn in stages:
            print("  stage alone: %-52s %.2f ms" % (name, timed(fn, 0.2)), flush=True)
    del chain, direct
    gc.collect()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=FULL[6])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--no-chain", action="store_true")
    a = ap.parse_args()
    kernel_part(a)
    if not a.no_chain:
        chain_part(a)


if __name__ == "__main__":
    main()
