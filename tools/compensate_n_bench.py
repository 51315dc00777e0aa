"""Times mvx_compensate_n_frames (mv.CompensateN) against what gives the same 2 * tr + 1 frames without it -- 2 * tr jobs through
mvx_compensate_frames (mv.Compensate, whose kernels this tool leaves alone) plus a copy of the source -- on the GPU with device events, every
input resident: super frames, the multi blob and the output frames.

    python tools/compensate_n_bench.py [--trs 3,8] [--repeats 3] [--seconds S] [--jobs N] [--overlap 8]
    python tools/compensate_n_bench.py --float [--trs 3] [--repeats 3] [--seconds S] [--jobs N]
    python tools/compensate_n_bench.py --single [--repeats 3] [--seconds S] [--jobs 8,256] [--shapes 8:8:0,8:16:8,16:16:8]

Workload: 1920 x 1080 8-bit 4:2:0, blocks of 16 overlapping by 8 (--overlap 0: side by side), pel 2, defaults otherwise.  The clip has 2 * tr + 1 frames
moving by one sample per frame; the job is the middle frame against all the others, with the vectors AnalyseN finds.  A call takes --jobs copies of that
job, each writing its own 2 * tr + 1 output frames; the job tables are built once and the C entry points are called directly.  The baseline's copy of
the source is three strided device copies per job (the pel-0 window of each plane of the super frame).  Each line is timed --repeats times in turn with
the other (a, b, a, b, ...), a call repeated until about S seconds lie between the two events after a warm-up call; the spread of a line is max - min over
its repeats.  Reported: ms per job (2 * tr + 1 frames).

--float: the float CompensateN (mvx_compensate_n_create_float) beside the 16-bit CompensateN in one session, on the SAME vectors (AnalyseN on the
16-bit clip; the float clip is that clip scaled to 0..1): 1920 x 1080 4:2:0, pel 2, blocks 16/8 and 16/0, the lines timed in turn as above.  Reported
per line: ms per job and the rate of the algorithm's bytes -- every output sample written once and one sample read for it, 2 * (2 * tr + 1) frames of
1.5 * 1920 * 1080 samples of 2 or 4 bytes per job (overlapped blocks read up to four samples and window weights per output sample: those extra
reads are the implementation's, not the algorithm's, and are not counted).

--single: mvx_compensate_frames by itself -- no CompensateN line, no copy of the source -- at 1920 x 1080 4:2:0, pel 2: 8-bit blocks 8/0, 8-bit 16/8 and
16-bit 16/8, each at every --jobs count (at 256 jobs the outputs of a call exceed the last-level cache).  A job is the middle frame of three against
the frame after it or, every other job, the frame before it, with the vectors Analyse finds; every job writes its own output frame.  Reported: ms per
job (one frame), --repeats times; to compare two builds of the library run one process per build (MVX_LIB selects the library) in turn."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vapoursynth-mvtools_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import mvtools_amd as mv  # noqa: E402
import pipeline as pl  # noqa: E402

W, H, BITS = 1920, 1080, 8


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
    return e0.elapsed_time(e1) / reps


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def n_call(L, cn, sf, refs, multi, stride, n, jobs, outs):
    """-> run(): one mvx_compensate_n_frames call of `jobs` copies of the job (frame n against refs), each into its own outs[j]"""
    no, nr = len(outs[0]), len(refs)
    table, arr = ((C.c_void_p * 3) * nr)(), (mv.CompensateNJob * jobs)()
    for r in range(nr):
        for p in range(3):
            table[r][p] = refs[r][p].data_ptr()
    dst = ((C.c_void_p * 3) * (no * jobs))()
    for j in range(jobs):
        for p in range(3):
            arr[j].src_super[p] = sf[n][p].data_ptr()
            for k in range(no):
                dst[j * no + k][p] = outs[j][k][p].data_ptr()
        arr[j].refs = C.cast(table, C.POINTER(C.c_void_p * 3))
        arr[j].dst = C.cast(C.byref(dst, j * no * C.sizeof(C.c_void_p * 3)), C.POINTER(C.c_void_p * 3))
        arr[j].blob, arr[j].field_stride = multi.data_ptr(), stride

    def run():
        if L.mvx_compensate_n_frames(cn.h, jobs, arr, stream()):
            raise SystemExit(L.mvx_last_error().decode())
    run.keep = (table, arr, dst)
    return run


def main_float(a):
    import numpy as np
    import torch
    L = mv.lib()
    for tr in [int(t) for t in a.trs.split(",")]:
        nfr, n, no = 2 * tr + 1, tr, 2 * tr + 1
        q = pl.moving_clip(W, H, 16, nfr, seed=5, motion=(1, 0))
        isup = mv.Super(W, H, 16)
        isf = isup.build([mv.frame_to_device(f) for f in q])
        fsup = mv.Super(W, H, 32, sample_float=True)
        fsf = fsup.build([mv.frame_to_device([(pl_.astype(np.float32) / np.float32(65535) - np.float32(0.5 if p else 0.0)) for p, pl_ in enumerate(f)]) for f in q])
        for overlap in (8, 0):
            an = mv.AnalyseN(isup, tr, num_frames=nfr, blksize=16, overlap=overlap)
            multi = an.run([(isf[n], [isf[m] for m in mv.multi_refs(n, tr, nfr)])])[0]
            ad = an.ad(0)
            lines, ms, rate = [], [], []
            for name, sup, sfr, kw in (("16-bit mvx_compensate_n_frames", isup, isf, {}), ("float  mvx_compensate_n_frames", fsup, fsf, dict(sample_float=True))):
                cn = mv.CompensateN(tr, sup, ad, **kw)
                i = sup.info
                hs = [i.height] + [i.height // i.yRatioUV] * 2
                outs = [[[torch.zeros((hs[p], cn.dst_pitch[p]), dtype=torch.uint8, device="cuda") for p in range(3)] for _ in range(no)] for _ in range(a.jobs)]
                lines.append((name, n_call(L, cn, sfr, [sfr[m] for m in mv.multi_refs(n, tr, nfr)], multi, an.field_stride, n, a.jobs, outs), cn, outs))
                ms.append([])
                rate.append(2 * no * (W * H * 3 // 2) * sup.bps)
            print("tr %d: %dx%d 4:2:0, blocks %d/%d (%d x %d), pel 2, vectors of the 16-bit search, %d jobs per call, %d repeats in turn; a job is %d frames" % (
                tr, W, H, ad.nBlkSizeX, ad.nOverlapX, ad.nBlkX, ad.nBlkY, a.jobs, a.repeats, no), flush=True)
            for _ in range(a.repeats):
                for k, line in enumerate(lines):
                    ms[k].append(timed(line[1], a.seconds) / a.jobs)
            gbs = []
            for line, m, b in zip(lines, ms, rate):
                gbs.append(b / (min(m) * 1e-3) / 1e9)
                print("  tr %d  ov %d  %-32s %s  min %.4f ms  spread %.4f ms  %.1f MB per job  %.0f GB/s (at the slowest repeat %.0f)" % (
                    tr, overlap, line[0], "  ".join("%.4f" % v for v in m), min(m), max(m) - min(m), b / 1e6, gbs[-1], b / (max(m) * 1e-3) / 1e9), flush=True)
            rel = max((max(m) - min(m)) / min(m) for m in ms)
            print("  tr %d  ov %d  byte rate float / 16-bit = %.3f (ms per job %.2fx); the larger relative spread of the two lines is %.3f: %s" % (
                tr, overlap, gbs[1] / gbs[0], min(ms[1]) / min(ms[0]), rel,
                "the float path's byte rate is LOWER by more than the spread" if gbs[1] / gbs[0] < 1 - rel else "the float path's byte rate is not lower by more than the spread"), flush=True)


def main_single(a):
    import torch
    L = mv.lib()
    for bits, blk, overlap in [tuple(int(v) for v in t.split(":")) for t in a.shapes.split(",")]:
        sup = mv.Super(W, H, bits)
        sf = sup.build([mv.frame_to_device(f) for f in pl.moving_clip(W, H, bits, 3, seed=5, motion=(1, 0))])
        blobs, ad = [], None
        for isb, ref in ((1, 2), (0, 0)):
            an = mv.Analyse(sup, isb=isb, blksize=blk, overlap=overlap)
            blobs.append(an.run([(sf[1], sf[ref])])[0])
            ad = an.ad
        refs = [sf[2], sf[0]]
        comp = mv.Compensate(sup, ad)
        i = sup.info
        hs = [i.height] + [i.height // i.yRatioUV] * 2
        for jobs in [int(j) for j in a.jobs.split(",")]:
            outs = [[torch.zeros((hs[p], comp.dst_pitch[p]), dtype=torch.uint8, device="cuda") for p in range(3)] for _ in range(jobs)]
            arr = (mv.CompensateJob * jobs)()
            for j in range(jobs):
                for p in range(3):
                    arr[j].src_super[p], arr[j].ref_super[p], arr[j].dst[p] = sf[1][p].data_ptr(), refs[j & 1][p].data_ptr(), outs[j][p].data_ptr()
                arr[j].blob = blobs[j & 1].data_ptr()

            def run():
                if L.mvx_compensate_frames(comp.h, jobs, arr, stream()):
                    raise SystemExit(L.mvx_last_error().decode())
            ms = [timed(run, a.seconds) / jobs for _ in range(a.repeats)]
            print("single  %2d-bit blocks %2d/%d (%d x %d)  %3d jobs per call  ms per job  %s  min %.4f  spread %.4f" % (
                bits, blk, overlap, ad.nBlkX, ad.nBlkY, jobs, "  ".join("%.4f" % v for v in ms), min(ms), max(ms) - min(ms)), flush=True)
            del outs, arr


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", action="store_true", help="mvx_compensate_frames by itself (see the head of this file)")
    ap.add_argument("--shapes", default="8:8:0,8:16:8,16:16:8", help="--single: bits:blksize:overlap of every shape")
    ap.add_argument("--float", dest="flt", action="store_true", help="the float CompensateN beside the 16-bit one (see the head of this file)")
    ap.add_argument("--trs", default="3,8")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--jobs", default="8", help="jobs (source frames) per call; --single: a list, e.g. 8,256")
    ap.add_argument("--overlap", type=int, default=8)
    a = ap.parse_args()
    if a.single:
        return main_single(a)
    a.jobs = int(a.jobs)
    if a.flt:
        if a.trs == "3,8":
            a.trs = "3"
        return main_float(a)
    L = mv.lib()
    for tr in [int(t) for t in a.trs.split(",")]:
        nfr, n, no, nr = 2 * tr + 1, tr, 2 * tr + 1, 2 * tr
        sup = mv.Super(W, H, BITS)
        sf = sup.build([mv.frame_to_device(f) for f in pl.moving_clip(W, H, BITS, nfr, seed=5, motion=(1, 0))])
        an = mv.AnalyseN(sup, tr, num_frames=nfr, blksize=16, overlap=a.overlap)
        refs = [sf[m] for m in mv.multi_refs(n, tr, nfr)]
        multi = an.run([(sf[n], refs)])[0]
        cn = mv.CompensateN(tr, sup, an.ad(0))
        comp = mv.Compensate(sup, an.ad(0))
        i = sup.info
        hs, ws = [i.height] + [i.height // i.yRatioUV] * 2, [i.width] + [i.width // i.xRatioUV] * 2
        pads = [(i.vpad, i.hpad)] + [(i.vpad // i.yRatioUV, i.hpad // i.xRatioUV)] * 2
        frame = lambda: [torch.zeros((hs[p], cn.dst_pitch[p]), dtype=torch.uint8, device="cuda") for p in range(3)]
        out_new = [[frame() for _ in range(no)] for _ in range(a.jobs)]
        out_old = [[frame() for _ in range(no)] for _ in range(a.jobs)]

        # CompensateN: a.jobs jobs, one call
        table, arr = ((C.c_void_p * 3) * nr)(), (mv.CompensateNJob * a.jobs)()
        for r in range(nr):
            for p in range(3):
                table[r][p] = refs[r][p].data_ptr()
        dst = ((C.c_void_p * 3) * (no * a.jobs))()
        for j in range(a.jobs):
            for p in range(3):
                arr[j].src_super[p] = sf[n][p].data_ptr()
                for k in range(no):
                    dst[j * no + k][p] = out_new[j][k][p].data_ptr()
            arr[j].refs = C.cast(table, C.POINTER(C.c_void_p * 3))
            arr[j].dst = C.cast(C.byref(dst, j * no * C.sizeof(C.c_void_p * 3)), C.POINTER(C.c_void_p * 3))
            arr[j].blob, arr[j].field_stride = multi.data_ptr(), an.field_stride

        def run_new():
            if L.mvx_compensate_n_frames(cn.h, a.jobs, arr, stream()):
                raise SystemExit(L.mvx_last_error().decode())

        # the baseline: 2 * tr Compensate jobs per source frame in one call, and the copy of the source
        old = (mv.CompensateJob * (nr * a.jobs))()
        fields = an.fields(multi)
        for j in range(a.jobs):
            for k in range(no):
                _, field = cn.map(k)
                if field < 0:
                    continue
                o = old[j * nr + field]
                for p in range(3):
                    o.src_super[p], o.ref_super[p], o.dst[p] = sf[n][p].data_ptr(), refs[field][p].data_ptr(), out_old[j][k][p].data_ptr()
                o.blob = fields[field].data_ptr()
        centre = [sf[n][p][pads[p][0]:pads[p][0] + hs[p], pads[p][1]:pads[p][1] + ws[p]] for p in range(3)]

        def run_old():
            if L.mvx_compensate_frames(comp.h, nr * a.jobs, old, stream()):
                raise SystemExit(L.mvx_last_error().decode())
            for j in range(a.jobs):
                for p in range(3):
                    out_old[j][tr][p][:, :ws[p]].copy_(centre[p])

        run_new(); run_old()
        torch.cuda.synchronize()
        same = all(torch.equal(out_new[j][k][p], out_old[j][k][p]) for j in (0, a.jobs - 1) for k in range(no) for p in range(3))
        ad = an.ad(0)
        print("tr %d: %dx%d %d-bit 4:2:0, blocks %d/%d (%d x %d), pel 2, %d jobs per call, %d repeats in turn; ms per job of %d frames; outputs %s" % (
            tr, W, H, BITS, ad.nBlkSizeX, ad.nOverlapX, ad.nBlkX, ad.nBlkY, a.jobs, a.repeats, no, "identical" if same else "DIFFER"), flush=True)
        lines = [("(a) %d x mvx_compensate_frames jobs + source copy" % nr, run_old), ("(b) mvx_compensate_n_frames", run_new)]
        ms = [[] for _ in lines]
        for _ in range(a.repeats):
            for k, (_, run) in enumerate(lines):
                ms[k].append(timed(run, a.seconds) / a.jobs)
        for (name, _), m in zip(lines, ms):
            print("  tr %d  %-50s %s  min %.4f  spread %.4f" % (tr, name, "  ".join("%.4f" % v for v in m), min(m), max(m) - min(m)), flush=True)
        d, spread = min(ms[1]) - min(ms[0]), max(ms[0]) - min(ms[0])
        print("  tr %d  (b) - (a) = %+.4f ms per job at the minima (%.2fx); spread of (a) %.4f: %s" % (
            tr, d, min(ms[0]) / min(ms[1]), spread, "(b) is FASTER than (a) by more than (a)'s spread" if -d > spread else
            "(b) ties with (a)" if d <= spread else "(b) IS SLOWER than (a) by more than (a)'s spread"), flush=True)


if __name__ == "__main__":
    main()
