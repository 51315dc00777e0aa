"""Times mvx_blockfps_frames (mv.BlockFPS) on the GPU with device events, every input resident: clip frames, super frames, both vector clips and
the output frames.

    python tools/blockfps_bench.py [--bits 16] [--blksize 16] [--repeats 3] [--seconds S] [--mode 3]
    python tools/blockfps_bench.py --float [--repeats 3] [--seconds S] [--mode 3]

Workload: 1920 x 1080 4:2:0 at --bits 8 or 16, pel 2, blocks of --blksize overlapping by half and the same blocks side by side, mode 3, 24 -> 60 fps
over a clip of five frames moving by one sample per frame, with the vectors Analyse finds.  MVX_LIB selects the library (the wrapper's rule), so
two builds are compared by running the tool once per build.  A call is the eight interpolated output frames of that conversion (outputs
1-4 and 6-9: time256 102, 205, 51, 154 between frames 0-1, 1-2, 2-3, 3-4), each into its own output frame; the job table is built once and the C
entry point is called directly.  Each line is timed --repeats times in turn with the other (a, b, a, b, ...), a call repeated until about S
seconds lie between the two events after a warm-up call; the spread of a line is max - min over its repeats.  Reported: ms per output frame.

--float: the float BlockFPS (mvx_blockfps_create_float) beside the 16-bit BlockFPS in one session, on the SAME vectors (Analyse on the 16-bit
clip; the float clip is that clip scaled to 0..1, chroma centred on 0).  Reported per line: ms per frame and the rate of the algorithm's bytes --
every output sample written once and two samples read for it, one from each super frame: 3 x 1.5 x 1920 x 1080 samples of 2 or 4 bytes per frame
(the masks, the plan, and with overlap the up to four blocks and window weights per sample are the implementation's reads, not the algorithm's,
and are not counted)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vapoursynth-mvtools_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import mvtools_amd as mv  # noqa: E402
import pipeline as pl  # noqa: E402

W, H, NFRAMES = 1920, 1080, 5
OUTPUTS = [1, 2, 3, 4, 6, 7, 8, 9]


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


def call(L, b, clip, sf, bw, fw, outs):
    """-> run(): one mvx_blockfps_frames call of the OUTPUTS, each into its own outs[k]"""
    import torch
    arr = (mv.BlockFPSJob * len(OUTPUTS))()
    for k, n in enumerate(OUTPUTS):
        nl, nr, t = b.map(n)
        assert 0 < t < 256 and nr < NFRAMES
        arr[k].time256 = t
        for p in range(3):
            arr[k].clip_left[p], arr[k].clip_right[p], arr[k].dst[p] = clip[nl][p].data_ptr(), clip[nr][p].data_ptr(), outs[k][p].data_ptr()
            arr[k].src_super[p], arr[k].ref_super[p] = sf[nl][p].data_ptr(), sf[nr][p].data_ptr()
        arr[k].blob_fw, arr[k].blob_bw = fw[nr].data_ptr(), bw[nl].data_ptr()

    def run():
        if L.mvx_blockfps_frames(b.h, len(OUTPUTS), arr, C.c_void_p(torch.cuda.current_stream().cuda_stream)):
            raise SystemExit(L.mvx_last_error().decode())
    run.keep = arr
    return run


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--float", dest="flt", action="store_true", help="the float BlockFPS beside the 16-bit one (see the head of this file)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--mode", type=int, default=3)
    ap.add_argument("--bits", type=int, default=16, choices=(8, 16), help="the integer clip's depth (--float: 16, the depth of the search it shares)")
    ap.add_argument("--blksize", type=int, default=16)
    a = ap.parse_args()
    if a.flt and a.bits != 16:
        ap.error("--float compares with the 16-bit clip")
    L = mv.lib()
    q = pl.moving_clip(W, H, a.bits, NFRAMES, seed=5, motion=(1, 0))
    isup = mv.Super(W, H, a.bits)
    iclip = [mv.frame_to_device(f) for f in q]
    isf = isup.build(iclip)
    kinds = [("%d-bit mvx_blockfps_frames" % a.bits, isup, iclip, isf, {})]
    if a.flt:
        fsup = mv.Super(W, H, 32, sample_float=True)
        fclip = [mv.frame_to_device([(x.astype(np.float32) / np.float32(65535) - np.float32(0.5 if p else 0.0)) for p, x in enumerate(f)]) for f in q]
        kinds.append(("float  mvx_blockfps_frames", fsup, fclip, fsup.build(fclip), dict(sample_float=True)))
    for overlap in (a.blksize // 2, 0):
        abw = mv.Analyse(isup, num_frames=NFRAMES, isb=1, blksize=a.blksize, overlap=overlap)
        afw = mv.Analyse(isup, num_frames=NFRAMES, isb=0, blksize=a.blksize, overlap=overlap)
        bw = abw.run([(isf[m], isf[m + 1] if m + 1 < NFRAMES else None) for m in range(NFRAMES)])
        fw = afw.run([(isf[m], isf[m - 1] if m >= 1 else None) for m in range(NFRAMES)])
        ad = abw.ad
        lines, ms, nbytes = [], [], []
        for name, sup, clip, sfr, kw in kinds:
            pitch = [p.stride(0) for p in clip[0]]
            b = mv.BlockFPS(sup, abw.ad, afw.ad, NFRAMES, pitch, 24, 1, num=60, den=1, mode=a.mode, **kw)
            outs = [[torch.zeros_like(p) for p in clip[0]] for _ in OUTPUTS]
            lines.append((name, call(L, b, clip, sfr, bw, fw, outs), b, outs))
            ms.append([])
            nbytes.append(3 * (W * H * 3 // 2) * sup.bps)
        print("%dx%d 4:2:0, blocks %d/%d (%d x %d), pel 2, mode %d, 24 -> 60, vectors of the 16-bit search, %d frames per call, %d repeats in turn" % (
            W, H, ad.nBlkSizeX, ad.nOverlapX, ad.nBlkX, ad.nBlkY, a.mode, len(OUTPUTS), a.repeats), flush=True)
        for _ in range(a.repeats):
            for k, line in enumerate(lines):
                ms[k].append(timed(line[1], a.seconds) / len(OUTPUTS))
        gbs = []
        for line, m, nb in zip(lines, ms, nbytes):
            gbs.append(nb / (min(m) * 1e-3) / 1e9)
            print("  ov %d  %-28s %s  min %.4f ms  spread %.4f ms  %.1f MB per frame  %.0f GB/s (at the slowest repeat %.0f)" % (
                overlap, line[0], "  ".join("%.4f" % v for v in m), min(m), max(m) - min(m), nb / 1e6, gbs[-1], nb / (max(m) * 1e-3) / 1e9), flush=True)
        if a.flt:
            rel = max((max(m) - min(m)) / min(m) for m in ms)
            print("  ov %d  byte rate float / 16-bit = %.3f (ms per frame %.2fx); the larger relative spread of the two lines is %.3f: %s" % (
                overlap, gbs[1] / gbs[0], min(ms[1]) / min(ms[0]), rel,
                "the float path's byte rate is LOWER by more than the spread" if gbs[1] / gbs[0] < 1 - rel else "the float path's byte rate is not lower by more than the spread"), flush=True)


if __name__ == "__main__":
    main()
