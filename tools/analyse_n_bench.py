"""Times mvx_analyse_n_frames (mv.AnalyseN: all 2 * radius fields of the source frames of a call as ONE search batch) against what gives the same
fields without it -- 2 * radius separate mvx_analyse_frames calls, one per (isb, delta), each over the same source frames -- on the GPU with device
events, every super frame and blob resident.

    python tools/analyse_n_bench.py [--radii 3,8] [--sources 1,8] [--repeats 3] [--seconds S]

Workload: 1920 x 1080 8-bit 4:2:0, blocks of 16 overlapping by 8, pel 2, defaults otherwise.  The clip has sources + 2 * radius frames moving by one
sample per frame, so every reference of every source frame lies inside the clip.  The job tables are built once and the C entry points are called
directly.  Each line is timed --repeats times in turn with the other (a, b, a, b, ...), a call sequence repeated until about S seconds lie between the
two events after a warm-up; the spread of a line is max - min over its repeats.  Reported: ms per source frame (2 * radius fields)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vapoursynth-mvtools_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import mvtools_amd as mv  # noqa: E402
import pipeline as pl  # noqa: E402
from compensate_n_bench import stream, timed  # noqa: E402

W, H, BITS = 1920, 1080, 8
AKW = dict(blksize=16, overlap=8)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--radii", default="3,8")
    ap.add_argument("--sources", default="1,8", help="source frames per call")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5)
    a = ap.parse_args()
    L = mv.lib()
    radii, sources = [int(v) for v in a.radii.split(",")], [int(v) for v in a.sources.split(",")]
    nfr = max(sources) + 2 * max(radii)
    sup = mv.Super(W, H, BITS)
    sf = sup.build([mv.frame_to_device(f) for f in pl.moving_clip(W, H, BITS, nfr, seed=5, motion=(1, 0))])
    for radius in radii:
        nr = 2 * radius
        an = mv.AnalyseN(sup, radius, num_frames=nfr, **AKW)
        ones = [mv.Analyse(sup, num_frames=nfr, isb=int(r % 2 == 0), delta=r // 2 + 1, **AKW) for r in range(nr)]
        for ns in sources:
            first = max(radii)
            frames = list(range(first, first + ns))
            multi = an.alloc_blobs(ns)
            single = [o.alloc_blobs(ns) for o in ones]
            table, arr = ((C.c_void_p * 3) * (nr * ns))(), (mv.AnalyseNJob * ns)()
            old = [(mv.AnalyseJob * ns)() for _ in range(nr)]
            for j, n in enumerate(frames):
                for r, m in enumerate(mv.multi_refs(n, radius, nfr)):
                    for p in range(3):
                        table[j * nr + r][p] = sf[m][p].data_ptr()
                        old[r][j].src[p], old[r][j].ref[p] = sf[n][p].data_ptr(), sf[m][p].data_ptr()
                    old[r][j].blob = single[r][j].data_ptr()
                for p in range(3):
                    arr[j].src[p] = sf[n][p].data_ptr()
                arr[j].refs = C.cast(C.byref(table, j * nr * C.sizeof(C.c_void_p * 3)), C.POINTER(C.c_void_p * 3))
                arr[j].blob = multi[j].data_ptr()

            def run_new():
                if L.mvx_analyse_n_frames(an.h, ns, arr, stream()):
                    raise SystemExit(L.mvx_last_error().decode())

            def run_old():
                for r in range(nr):
                    if L.mvx_analyse_frames(ones[r].h, ns, old[r], stream()):
                        raise SystemExit(L.mvx_last_error().decode())

            run_new(); run_old()
            torch.cuda.synchronize()
            same = all(torch.equal(an.fields(multi[j])[r], single[r][j]) for j in range(ns) for r in range(nr))
            ad = an.ad(0)
            print("radius %d, %d source frames per call (%d chains): %dx%d %d-bit 4:2:0, blocks 16/8 (%d x %d), pel 2, %d repeats in turn; ms per source frame; fields %s" % (
                radius, ns, nr * ns, W, H, BITS, ad.nBlkX, ad.nBlkY, a.repeats, "identical" if same else "DIFFER"), flush=True)
            lines = [("(a) %d mvx_analyse_frames calls of %d jobs" % (nr, ns), run_old), ("(b) one mvx_analyse_n_frames call", run_new)]
            ms = [[] for _ in lines]
            for _ in range(a.repeats):
                for k, (_, run) in enumerate(lines):
                    ms[k].append(timed(run, a.seconds) / ns)
            for (name, _), m in zip(lines, ms):
                print("  %-44s %s  min %.3f  spread %.3f" % (name, "  ".join("%.3f" % v for v in m), min(m), max(m) - min(m)), flush=True)
            d, spread = min(ms[1]) - min(ms[0]), max(ms[0]) - min(ms[0])
            print("  (b) - (a) = %+.3f ms per source frame at the minima (%.2fx); spread of (a) %.3f: %s" % (
                d, min(ms[0]) / min(ms[1]), spread, "(b) is not slower than (a) by more than (a)'s spread" if d <= spread else "(b) IS SLOWER than (a) by more than (a)'s spread"),
                flush=True)


if __name__ == "__main__":
    main()
