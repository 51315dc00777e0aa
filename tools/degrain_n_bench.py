"""Times the Degrain step alone -- mvx_degrain_frames (mv.Degrain) and mvx_degrain_n_frames (mv.DegrainN) -- on the GPU with device events, every
input resident: clip frames, super frames, vector blobs and the output frames.

    python tools/degrain_n_bench.py [--configs 1080p8,4k16] [--seconds S] [--jobs N]
    python tools/degrain_n_bench.py --out16 [--radii 3,8] [--repeats 3] [--seconds S] [--jobs N]

Workloads: 1920 x 1080 8-bit and 3840 x 2160 16-bit, 4:2:0, blocks of 16 overlapping by 8, pel 2.  Rows: Degrain at radius 3 and 6 (the existing kernels,
whose code this tool leaves alone: what the new ones are read against) and DegrainN at radius 3, 6, 12 and 24, defaults otherwise (thsad 400, no fall-off).

The clip has seven frames moving by one sample per frame; the job is frame 3, and the references at distance d are frames 3 +- ((d - 1) % 3 + 1) with the
vectors the search finds for them -- so beyond distance 3 the near frames are used again.  Nearly every weight is then above 0, at every radius: the lists of
DegrainN are as long as they get, and the times are its worst case (on real footage the far lists are shorter).  A call takes --jobs copies of that job, each
writing its own output frame; the job tables are built once and the C entry point is called directly, so the host's share of a call is the library's
own (DegrainN copies its reference tables per call).  The call is repeated until about S seconds lie between the two events, after a warm-up call of the
same shape.  Reported: ms per frame = ms per call / jobs, and the mean number of references with a weight per block.  Kernel times and counters come from
separate profiler runs.

--out16: the 1080p 8-bit clip only, DegrainN at each of --radii, --repeats timings of each of three lines: (a) the 8-bit DegrainN, (b) DegrainN with out16
(8-bit clip, super frames and vectors, 16-bit output planes), (c) what gives 16-bit output without out16 -- the same clip shifted left by 8 as a 16-bit clip,
its own 16-bit super frames and vectors, the 16-bit DegrainN.  The repeats of a line are taken in turn with the other lines (a, b, c, a, b, c, ...), so a drift
of the clock reaches all three alike; the spread of a line is max - min over its repeats."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vapoursynth-mvtools_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import mvtools_amd as mv  # noqa: E402
import pipeline as pl  # noqa: E402
import vector_fields  # noqa: E402

CONFIGS = {"1080p8": (1920, 1080, 8), "4k16": (3840, 2160, 16)}
ROWS = [("Degrain", 3), ("Degrain", 6), ("DegrainN", 3), ("DegrainN", 6), ("DegrainN", 12), ("DegrainN", 24)]
AKW = dict(blksize=16, overlap=8)
POOL, TARGET = 7, 3


def timed(run, seconds):
    import torch
    run()  # warm-up of the timed shape: code objects, the handle's buffers
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    reps = max(5, int(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)))
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, reps


def call_of(kind, g, src, refs, blobs, out):
    """-> a function that enqueues one call of len(out) jobs (the arrays it passes stay alive in its closure)"""
    n, nr, L = len(out), len(refs), mv.lib()
    rt = bt = None
    if kind == "Degrain":
        arr = (mv.DegrainJob * n)()
    else:
        arr = (mv.DegrainNJob * n)()
        rt, bt = ((C.c_void_p * 3) * nr)(), (C.c_void_p * nr)()
        for r in range(nr):
            for p in range(3):
                rt[r][p] = refs[r][p].data_ptr()
            bt[r] = blobs[r].data_ptr()
    for i in range(n):
        for p in range(3):
            arr[i].src[p] = src[p].data_ptr()
            arr[i].dst[p] = out[i][p].data_ptr()
        if kind == "Degrain":
            for r in range(nr):
                for p in range(3):
                    arr[i].refs[r][p] = refs[r][p].data_ptr()
                arr[i].blobs[r] = blobs[r].data_ptr()
        else:
            arr[i].refs = C.cast(rt, C.POINTER(C.c_void_p * 3))
            arr[i].blobs = C.cast(bt, C.POINTER(C.c_void_p))
    fn = L.mvx_degrain_frames if kind == "Degrain" else L.mvx_degrain_n_frames

    def run(keep=(arr, rt, bt, refs, blobs, out)):
        import torch
        if fn(g.h, n, arr, C.c_void_p(torch.cuda.current_stream().cuda_stream)):
            raise SystemExit(L.mvx_last_error().decode())
    return run


def prepared(w, h, bits, clip):
    """-> (device frames, super clip, analysis data, {(isb, delta 1..3): (reference super frame, blob)}) for the job TARGET"""
    sup = mv.Super(w, h, bits)
    src = [mv.frame_to_device(f) for f in clip]
    sf = sup.build(src)
    near = {}
    for d in (1, 2, 3):
        for isb in (1, 0):
            an = mv.Analyse(sup, num_frames=POOL, isb=isb, delta=d, **AKW)
            nref = TARGET + (d if isb else -d)
            near[(isb, d)] = (sf[nref], an.run([(sf[TARGET], sf[nref])])[0])
    return src, sup, an.ad, near


def main_out16(a):
    import torch
    w, h, _ = CONFIGS["1080p8"]
    njobs = a.jobs or 64
    clip8 = pl.moving_clip(w, h, 8, POOL, seed=5, motion=(1, 0))
    clip16 = [[p.astype(np.uint16) << 8 for p in f] for f in clip8]
    src8, sup8, ad8, near8 = prepared(w, h, 8, clip8)
    src16, sup16, ad16, near16 = prepared(w, h, 16, clip16)
    pitch8, pitch16 = [p.stride(0) for p in src8[0]], [p.stride(0) for p in src16[0]]
    out8 = [[torch.empty_like(p) for p in src8[TARGET]] for _ in range(njobs)]
    out16 = [[torch.empty_like(p) for p in src16[TARGET]] for _ in range(njobs)]
    print("out16: %dx%d 4:2:0, blocks 16/8 (%d x %d), pel 2, %d jobs per call, %d repeats in turn; ms per frame" % (w, h, ad8.nBlkX, ad8.nBlkY, njobs, a.repeats), flush=True)
    for radius in [int(r) for r in a.radii.split(",")]:
        def listed(near):
            picks = [near[(isb, (d - 1) % 3 + 1)] for d in range(1, radius + 1) for isb in (1, 0)]
            return [r for r, _ in picks], [b for _, b in picks]
        refs8, blobs8 = listed(near8)
        refs16, blobs16 = listed(near16)
        ga = mv.DegrainN(radius, sup8, ad8, pitch8)
        gb = mv.DegrainN(radius, sup8, ad8, pitch8, dst_pitch=pitch16, out16=True)
        gc = mv.DegrainN(radius, sup16, ad16, pitch16)
        assert (ga.out_bits, gb.out_bits, gc.out_bits) == (8, 16, 16)
        lines = [("(a) 8-bit clip, 8-bit output", call_of("DegrainN", ga, src8[TARGET], refs8, blobs8, out8)),
                 ("(b) 8-bit clip, out16", call_of("DegrainN", gb, src8[TARGET], refs8, blobs8, out16)),
                 ("(c) clip shifted to 16 bits, 16-bit DegrainN", call_of("DegrainN", gc, src16[TARGET], refs16, blobs16, out16))]
        ms = [[] for _ in lines]
        for _ in range(a.repeats):
            for i, (_, run) in enumerate(lines):
                ms[i].append(timed(run, a.seconds)[0] / njobs)
        for (name, _), m in zip(lines, ms):
            print("  radius %2d  %-46s %s  min %.4f  spread %.4f  (%.0f fps)" % (radius, name, "  ".join("%.4f" % v for v in m), min(m), max(m) - min(m), 1e3 / min(m)), flush=True)
        b, c = ms[1], ms[2]
        print("  radius %2d  (b) - (c) = %+.4f ms per frame at the minima; spread of (c) %.4f: %s" % (
            radius, min(b) - min(c), max(c) - min(c), "(b) is not slower than (c) by more than (c)'s spread" if min(b) - min(c) <= max(c) - min(c) else "(b) IS SLOWER than (c) by more than (c)'s spread"),
            flush=True)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1080p8,4k16")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--jobs", type=int, default=0, help="jobs per call (default: 64 at 1080p, 16 at 4K)")
    ap.add_argument("--out16", action="store_true", help="1080p 8-bit: DegrainN, DegrainN with out16, and the 16-bit DegrainN on the clip shifted up")
    ap.add_argument("--radii", default="3,8", help="with --out16")
    ap.add_argument("--repeats", type=int, default=3, help="with --out16")
    a = ap.parse_args()
    if a.out16:
        return main_out16(a)
    for name in a.configs.split(","):
        w, h, bits = CONFIGS[name]
        njobs = a.jobs or (64 if w < 3000 else 16)
        clip = pl.moving_clip(w, h, bits, POOL, seed=5, motion=(1, 0))
        sup = mv.Super(w, h, bits)
        src = [mv.frame_to_device(f) for f in clip]
        sf = sup.build(src)
        near = {}  # (isb, delta 1..3) -> (reference super frame, blob)
        for d in (1, 2, 3):
            for isb in (1, 0):
                an = mv.Analyse(sup, num_frames=POOL, isb=isb, delta=d, **AKW)
                nref = TARGET + (d if isb else -d)
                near[(isb, d)] = (sf[nref], an.run([(sf[TARGET], sf[nref])])[0])
        ad = an.ad
        pitch = [p.stride(0) for p in src[0]]
        out = [[torch.empty_like(p) for p in src[TARGET]] for _ in range(njobs)]
        print("%s: %dx%d %d-bit 4:2:0, blocks 16/8 (%d x %d), pel 2, %d jobs per call" % (name, w, h, bits, ad.nBlkX, ad.nBlkY, njobs), flush=True)
        for kind, radius in ROWS:
            refs, blobs = [], []
            for d in range(1, radius + 1):
                for isb in (1, 0):
                    r, b = near[(isb, (d - 1) % 3 + 1)]
                    refs.append(r)
                    blobs.append(b)
            g = (mv.Degrain if kind == "Degrain" else mv.DegrainN)(radius, sup, ad, pitch)
            ms, reps = timed(call_of(kind, g, src[TARGET], refs, blobs, out), a.seconds)
            sads = np.stack([pl.blob_vectors(b.cpu().numpy(), ad)[2].reshape(-1) for b in blobs])
            th = vector_fields.scaled_thresholds(ad, 400)[0]
            mean_list = float(np.mean(np.sum(sads < th, axis=0)))
            print("  %-8s radius %2d (%2d references)  %8.4f ms/frame  %9.4f ms/call  calls=%d  mean references with a weight per block=%.1f" % (
                kind, radius, 2 * radius, ms / njobs, ms, reps, mean_list), flush=True)


if __name__ == "__main__":
    main()
