"""Times the float path beside the 16-bit path it replaces, in one session and on the same vectors: DegrainN and Super on a float32 clip against
DegrainN and Super on its 16-bit quantised copy.  Device events around resident inputs, a warm-up call of every timed shape, the four lines taken
in turn over --repeats rounds (tools/degrain_n_bench.py has the timing and the job tables).

    python tools/degrain_float_bench.py [--seconds S] [--repeats N] [--jobs N] [--out profiles/degrain_float_bench.txt]

Workload: 1920 x 1080 4:2:0, radius 3, blocks of 16 overlapping by 8, pel 2.  The vectors are searched once, on the 16-bit copy, and both DegrainN
objects read the same blobs.  Both Supers have one level (the render super of a script that searches elsewhere) and no shadow planes.

Reported per line: ms per frame, frames/s, and bytes/s over the bytes the algorithm needs, computed here from the shapes:
    DegrainN  (1 source + 1 output + 2 * radius references) x the clip frame's samples x bytes per sample
    Super     the clip frame's samples + pel^2 x the padded frame's samples, x bytes per sample
No rate is promised for the float path: it moves twice the bytes of the 16-bit path.  The figure to read is its byte rate beside the 16-bit path's."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import degrain_n_bench as dnb  # noqa: E402  (puts the package and tests/ on the path)
import numpy as np  # noqa: E402

mv, pl = dnb.mv, dnb.pl
W, H, RADIUS = 1920, 1080, 3
POOL, TARGET = dnb.POOL, dnb.TARGET


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--jobs", type=int, default=32, help="frames per call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "degrain_float_bench.txt"))
    a = ap.parse_args()
    njobs = a.jobs
    clip16 = pl.moving_clip(W, H, 16, POOL, seed=5, motion=(1, 0))
    clipf = [[(p.astype(np.float64) / 65535.0 - (0.5 if i else 0.0)).astype(np.float32) for i, p in enumerate(f)] for f in clip16]
    # the search, once, on the 16-bit copy
    src16, sup16, ad, near = dnb.prepared(W, H, 16, clip16)
    order = [(isb, d) for d in range(1, RADIUS + 1) for isb in (1, 0)]
    blobs = [near[k][1] for k in order]
    nref = [TARGET + (d if isb else -d) for isb, d in order]
    # the render supers: one level, no shadow planes
    rsup16 = mv.Super(W, H, 16, levels=1, shadow=False)
    rsf16 = rsup16.build(src16)
    fsup = mv.Super(W, H, 32, sample_float=True)
    srcf = [mv.frame_to_device(f) for f in clipf]
    fsf = fsup.build(srcf)
    pitch16, pitchf = [p.stride(0) for p in src16[0]], [p.stride(0) for p in srcf[0]]
    g16 = mv.DegrainN(RADIUS, rsup16, ad, pitch16)
    gf = mv.DegrainN(RADIUS, fsup, ad, pitchf)
    assert (g16.out_bits, gf.out_bits) == (16, 32)
    out16 = [[torch.empty_like(p) for p in src16[TARGET]] for _ in range(njobs)]
    outf = [[torch.empty_like(p) for p in srcf[TARGET]] for _ in range(njobs)]
    sup_in16, sup_inf = [src16[i % POOL] for i in range(njobs)], [srcf[i % POOL] for i in range(njobs)]
    sup_out16, sup_outf = rsup16.alloc(njobs), fsup.alloc(njobs)
    samples = W * H * 3 // 2
    padded = sum(fsup.info.pel ** 2 * (W // s + 2 * (fsup.info.hpad // s)) * (H // s + 2 * (fsup.info.vpad // s)) for s in (1, 2, 2))
    lines = [("DegrainN 16-bit", dnb.call_of("DegrainN", g16, src16[TARGET], [rsf16[m] for m in nref], blobs, out16), (2 + 2 * RADIUS) * samples * 2),
             ("DegrainN float", dnb.call_of("DegrainN", gf, srcf[TARGET], [fsf[m] for m in nref], blobs, outf), (2 + 2 * RADIUS) * samples * 4),
             ("Super 16-bit", lambda: rsup16.build(sup_in16, out=sup_out16), (samples + padded) * 2),
             ("Super float", lambda: fsup.build(sup_inf, out=sup_outf), (samples + padded) * 4)]
    ms = [[] for _ in lines]
    for _ in range(a.repeats):
        for i, (_, run, _) in enumerate(lines):
            ms[i].append(dnb.timed(run, a.seconds)[0] / njobs)
    text = ["float DegrainN and Super beside the 16-bit path (DESIGN.md 4.3.4): python tools/degrain_float_bench.py",
            "%s, %dx%d 4:2:0, radius %d, blocks 16/8 (%d x %d), pel 2, one-level supers, %d frames per call, %d repeats in turn, same session, same vectors" % (
                torch.cuda.get_device_name(0), W, H, RADIUS, ad.nBlkX, ad.nBlkY, njobs, a.repeats),
            "bytes: the algorithm's (DegrainN: source + output + %d references; Super: clip frame + level 0), not the memory system's" % (2 * RADIUS), ""]
    for (name, _, nbytes), m in zip(lines, ms):
        best = min(m)
        text.append("  %-16s ms/frame %s  min %.4f  spread %.4f  %8.0f frames/s  %7.1f GB/s  (%.1f MB per frame)" % (
            name, "  ".join("%.4f" % v for v in m), best, max(m) - best, 1e3 / best, nbytes / best / 1e6, nbytes / 1e6))
    for k in (0, 2):
        b16, bf = lines[k][2] / min(ms[k]), lines[k + 1][2] / min(ms[k + 1])
        text.append("  %s: the float path's byte rate is %.2f of the 16-bit path's, its frame rate %.2f" % (lines[k][0].split()[0], bf / b16, min(ms[k]) / min(ms[k + 1])))
    print("\n".join(text), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
