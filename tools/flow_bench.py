"""Times mvx_flow_frames (mv.FlowFPS), mvx_flowcomp_frames (mv.Flow) and mvx_flowblur_frames (mv.FlowBlur) on the GPU with device events,
the super frames and vector blobs resident.

    python tools/flow_bench.py [--frames N] [--warmup W] [--only 1080p8|4k16] [--filters flowfps,fetch,shift,blur]
    python tools/flow_bench.py --float [--frames N] [--repeats R] [--filters fetch,shift,blur,flowinter,flowfps]

Workloads at 1080p 8-bit and 4K 16-bit 4:2:0: FlowFPS 2x and 24 -> 60, mask=2; Flow fetch and Flow shift at time 100; FlowBlur at blur 50,
prec 1.  Per workload: output fps, ms per output frame, algorithmic bytes per output frame and frac = those bytes per second over 8.0 TB/s.
FlowFPS: 3 x the output frame (its write plus one read of each of the two input frames it lies between); Flow and FlowBlur: 2 x (the write
plus one read of the frame they sample).  FlowBlur also reports its mean taps per sample (F + B, all planes).  Flow shift launches at most 64
jobs at once (its winner buffer takes 8 bytes per sample and job).  Kernel times come from a separate rocprofv3 --kernel-trace --stats run
of this script.

--float: Flow fetch, Flow shift and FlowBlur (blur 50), and with --filters flowinter,flowfps FlowInter (time 50) and FlowFPS (24 -> 60, mask 2;
both on the Extra formula), at 1080p 4:2:0, pel 2, blocks 16/8, on a 16-bit clip and on its float clip (sample_float=True) with the SAME
vectors, searched once on the 16-bit clip.  The two paths alternate R times in one process; per path the median, the fastest and the slowest ms
per frame, the spread (slowest - fastest) / median, and the algorithm's bytes per second at the median (2 x the output frame, 3 x for FlowInter
and FlowFPS: 2-byte samples against 4-byte samples).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vapoursynth-mvtools_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import flow_ref  # noqa: E402
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


def _timed(launch, arr):
    """ms of one launch of the job table arr, after a warm-up launch of the same shape"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    launch(arr)
    torch.cuda.synchronize()
    e0.record()
    launch(arr)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _mean_taps(sup, ad_bw, ad_fw, blob_bw, blob_fw, blur256, prec):
    """RealFlowBlur's taps per sample (mF + mB, MVFlowBlur.c:88-118) over all planes of one frame, from its upsized vectors"""
    vb, vf = pl.blob_vectors(blob_bw.cpu().numpy(), ad_bw), pl.blob_vectors(blob_fw.cpu().numpy(), ad_fw)
    taps = samples = 0
    for p in range(sup.nplanes):
        xr, yr = (ad_bw.xRatioUV, ad_bw.yRatioUV) if p else (1, 1)
        lw, lh = ad_bw.nWidth // xr, ad_bw.nHeight // yr
        for v in (vb, vf):
            sx, sy = v[0].astype(np.int16), v[1].astype(np.int16)
            if p:
                sx, sy = flow_ref.half_uv(sx, xr), flow_ref.half_uv(sy, yr)
            fx = flow_ref.upsize_i16(sx, lw, lh, lw, lh, ad_bw.nPel, True).astype(np.int64) * blur256
            fy = flow_ref.upsize_i16(sy, lw, lh, lw, lh, ad_bw.nPel, False).astype(np.int64) * blur256
            taps += int(((np.maximum(np.abs(fx), np.abs(fy)) // prec) >> 8).sum())
        samples += lw * lh
    return taps / samples


def workload_mc(w, h, bits, kind, frames, warmup, nin=4):
    """kind: fetch / shift (mv.Flow, mvbw vectors, time 100) or blur (mv.FlowBlur, blur 50, prec 1)"""
    import torch
    clip = pl.moving_clip(w, h, bits, nin, seed=5)
    sup = mv.Super(w, h, bits)
    src = [mv.frame_to_device(f) for f in clip]
    sf = sup.build(src)
    akw = dict(blksize=16, overlap=8) if w > 2000 else dict(blksize=8, overlap=4)
    abw, afw = mv.Analyse(sup, num_frames=nin, isb=1, **akw), mv.Analyse(sup, num_frames=nin, isb=0, **akw)
    bbw = abw.run([(sf[n], sf[n + 1] if n + 1 < nin else None) for n in range(nin)])
    bfw = afw.run([(sf[n], sf[n - 1] if n >= 1 else None) for n in range(nin)])
    pitch = [p.stride(0) for p in src[0]]
    if kind == "shift":
        frames = min(frames, 64)
    out = mv.arena_frames(frames, [tuple(p.shape) for p in src[0]], src[0][0].device, zero=False)
    extra = ""
    if kind == "blur":
        fl = mv.FlowBlur(sup, abw.ad, afw.ad, nin, pitch, blur=50.0, prec=1)
        ns = [1 + k % (nin - 2) for k in range(frames)]  # frames with mvbw at n - 1 and mvfw at n + 1: no copies
        fl.run(ns[:warmup], src, sf, bbw, bfw)
        arr, out = fl.jobs(ns, src, sf, bbw, bfw, out=out)
        launch = fl.launch
        extra = "  mean_taps/sample=%.2f" % _mean_taps(sup, abw.ad, afw.ad, bbw[0], bfw[2], int(np.float32(50.0) * np.float32(256.0) / np.float32(200.0)), 1)
        name = "flowblur blur=50 prec=1 %dx%d %d-bit 4:2:0" % (w, h, bits)
    else:
        fl = mv.Flow(sup, abw.ad, nin, pitch, time=100.0, mode=1 if kind == "shift" else 0)
        ns = [k % (nin - 1) for k in range(frames)]  # nref = n + 1 inside the clip: no copies
        jobs = [(src[n], sf[n + 1], bbw[n]) for n in ns]
        fl.run(jobs[:warmup])
        arr = (mv.FlowCompJob * frames)()
        for k, (c, r, b) in enumerate(jobs):
            for p in range(sup.nplanes):
                arr[k].clip[p], arr[k].ref_super[p], arr[k].dst[p] = c[p].data_ptr(), r[p].data_ptr(), out[k][p].data_ptr()
            arr[k].blob = b.data_ptr()
        launch = fl.launch
        name = "flow %s time=100 %dx%d %d-bit 4:2:0" % ("fetch" if kind == "fetch" else "shift", w, h, bits)
    torch.cuda.synchronize()
    ms = _timed(launch, arr)
    frame_bytes = w * h * ((bits + 7) // 8) * 3 // 2
    alg = 2 * frame_bytes
    per = ms / frames
    frac = alg / (per * 1e-3) / PEAK
    print("%-44s frames=%d  %.1f fps  %.4f ms/frame  alg_bytes/frame=%d  frac=%.3f%s" % (name, frames, 1000.0 / per, per, alg, frac, extra), flush=True)


def float_workloads(kinds, frames, warmup, repeats, w=1920, h=1080, nin=4):
    """the 16-bit path and the float path of Flow fetch / Flow shift / FlowBlur / FlowInter / FlowFPS on the same vectors, alternating"""
    import torch
    import degrain_float_cases as fc
    q = pl.moving_clip(w, h, 16, nin, seed=5)
    floats = fc.float_clip(q, 16, seed=9)
    akw = dict(blksize=16, overlap=8)
    sides = {}
    isup = mv.Super(w, h, 16, pel=2)
    isrc = [mv.frame_to_device(f) for f in q]
    isf = isup.build(isrc)
    abw, afw = mv.Analyse(isup, num_frames=nin, isb=1, **akw), mv.Analyse(isup, num_frames=nin, isb=0, **akw)
    bbw = abw.run([(isf[n], isf[n + 1] if n + 1 < nin else None) for n in range(nin)])
    bfw = afw.run([(isf[n], isf[n - 1] if n >= 1 else None) for n in range(nin)])
    fsup = mv.Super(w, h, 32, pel=2, sample_float=True)
    fsrc = [mv.frame_to_device(f) for f in floats]
    sides["16-bit"] = (isup, isrc, isf, {}, 2)
    sides["float"] = (fsup, fsrc, fsup.build(fsrc), dict(sample_float=True), 4)
    for kind in kinds:
        n = min(frames, 64) if kind == "shift" else frames
        runs = {}
        for tag, (sup, src, sf, kw, bps) in sides.items():
            pitch = [p.stride(0) for p in src[0]]
            out = mv.arena_frames(n, [tuple(p.shape) for p in src[0]], src[0][0].device, zero=False)
            reads = 1
            if kind in ("flowinter", "flowfps"):
                if kind == "flowinter":
                    fl = mv.FlowInter(sup, abw.ad, afw.ad, nin, pitch, time=50.0, **kw)
                    inner = [1]
                else:
                    fl = mv.FlowFPS(sup, abw.ad, afw.ad, nin, pitch, 24, 1, num=60, den=1, mask=2, **kw)
                    inner = [k for k in range(fl.num_frames) if fl.map(k)[0] == 1 and fl.map(k)[2] not in (0, 256)]
                # output frames inside the middle input interval (1, 2): both extra blobs usable -> the Extra formula, no copies
                ns = [inner[k % len(inner)] for k in range(n)]
                fl.run(ns[:warmup], src, sf, bbw, bfw)
                arr, _ = fl.jobs(ns, src, sf, bbw, bfw, out=out)
                reads = 2
            elif kind == "blur":
                fl = mv.FlowBlur(sup, abw.ad, afw.ad, nin, pitch, blur=50.0, prec=1, **kw)
                ns = [1 + k % (nin - 2) for k in range(n)]
                fl.run(ns[:warmup], src, sf, bbw, bfw)
                arr, _ = fl.jobs(ns, src, sf, bbw, bfw, out=out)
            else:
                fl = mv.Flow(sup, abw.ad, nin, pitch, time=100.0, mode=1 if kind == "shift" else 0, **kw)
                jobs = [(src[k % (nin - 1)], sf[k % (nin - 1) + 1], bbw[k % (nin - 1)]) for k in range(n)]
                fl.run(jobs[:warmup])
                arr = (mv.FlowCompJob * n)()
                for k, (c, r, b) in enumerate(jobs):
                    for p in range(sup.nplanes):
                        arr[k].clip[p], arr[k].ref_super[p], arr[k].dst[p] = c[p].data_ptr(), r[p].data_ptr(), out[k][p].data_ptr()
                    arr[k].blob = b.data_ptr()
            runs[tag] = (fl, arr, out, (1 + reads) * (w * h * bps * 3 // 2), [])
        torch.cuda.synchronize()
        for _ in range(repeats):
            for tag in runs:  # alternating, each timed launch after a warm-up launch of its own shape
                fl, arr, _, _, ms = runs[tag]
                ms.append(_timed(fl.launch, arr) / n)
        for tag, (_, _, _, alg, ms) in runs.items():
            med, lo_, hi = float(np.median(ms)), min(ms), max(ms)
            print("%-7s %-6s 1080p 4:2:0 pel 2 16/8  frames=%d repeats=%d  median %.4f ms/frame (fastest %.4f, slowest %.4f, spread %.1f %%)  "
                  "alg_bytes/frame=%d  %.3f TB/s  frac=%.3f" % (kind, tag, n, repeats, med, lo_, hi, 100.0 * (hi - lo_) / med, alg, alg / (med * 1e-3) / 1e12,
                                                                alg / (med * 1e-3) / PEAK), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--only", default=None, help="run one workload: 1080p8 or 4k16 (counter passes)")
    ap.add_argument("--filters", default="flowfps,fetch,shift,blur", help="comma-separated subset of flowfps, fetch, shift, blur (--float: and flowinter)")
    ap.add_argument("--float", dest="float_", action="store_true", help="the float path against the 16-bit path on the same vectors (1080p, pel 2, 16/8)")
    ap.add_argument("--repeats", type=int, default=7, help="--float: timed launches per path, alternating")
    a = ap.parse_args()
    filters = a.filters.split(",")
    if a.float_:
        float_workloads([k for k in ("fetch", "shift", "blur", "flowinter", "flowfps") if k in filters], a.frames, a.warmup, a.repeats)
        return
    for (w, h, bits, tag) in ((1920, 1080, 8, "1080p8"), (3840, 2160, 16, "4k16")):
        if "flowfps" in filters:
            for num in (48, 60):
                if a.only in (None, tag) and (a.only is None or num == 48):
                    workload(w, h, bits, num, a.frames, a.warmup)
        for kind in ("fetch", "shift", "blur"):
            if kind in filters and a.only in (None, tag):
                workload_mc(w, h, bits, kind, a.frames, a.warmup)


if __name__ == "__main__":
    main()
