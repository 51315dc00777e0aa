"""developer tool: how many blocks of the speculative search kernel (mvx_analyse_spec.h) verify, per level, from a library built with
-DMVX_SPEC_STATS (python tools/build_variant.py specstats "MVX_SPEC_STATS" mvx_analyse_spec_u16.hip):

    MVX_LIB=tools/variants/specstats.so python tools/specstats.py [cfg] [batch]

Also per level: the windows of stage 2 by form, the stage-2 passes that ran and the passes that packing saved (add MVX_SPEC_NOPACK to the switches
for the unpacked count); the windows that are not in strip form by their runs of equal centres, the run-form passes that ran and the passes run form
saved against block form (MVX_SPEC_NORUN: the histogram alone)."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import torch  # noqa: E402
import mvtools_amd as mv  # noqa: E402

cfg = bench.CONFIGS[sys.argv[1] if len(sys.argv) > 1 else "cfg3"]
batch = int(sys.argv[2]) if len(sys.argv) > 2 else 64
blk, ov = cfg[4].get("blksize", 8), cfg[4].get("overlap", 0)
nblkx0 = (cfg[0] - ov) // (blk - ov)  # blocks per row of the finest level
p = bench.Pipeline(mv, torch, cfg, batch, torch.device("cuda", 0), 1)
NCOL = 17  # (SPEC_NSTAT of mvx_analyse_spec.h)
out = (C.c_ulonglong * (24 * NCOL))()  # MVX_MAX_LEVELS x NCOL
p.step()
torch.cuda.synchronize()
assert mv.lib().mvx_debug_specstats(out, 1) == 0
p.step(time_search=True)
torch.cuda.synchronize()
assert mv.lib().mvx_debug_specstats(out, 1) == 0
print("batch %d: search launch %.1f ms (counting build)" % (batch, p.ev[0][0].elapsed_time(p.ev[0][1])))
print("level: blocks in speculated rows, searched live (share), of them flag clear (hexagon won / rescue), accepted after redoing the predictor phase with the true left / median")
for lv in range(16):
    b, live, flag, resc, ws, wb, dev, lim, p2, saved, r1, r2, r3, r4, rlim, prun, rsaved = (int(out[lv * NCOL + i]) for i in range(NCOL))
    if b:
        print("%5d: %12d %12d (%5.2f %%) %12d %10d" % (lv, b, live, 100.0 * live / b, flag, resc))
        if ws + wb:
            print("       stage-2 windows (16x16 row passes): strip form %d (%.1f %%), block form %d -- %.2f blocks per block-form window whose centre differs from the window's first block, %d block-form windows for the limits alone" % (
                ws, 100.0 * ws / (ws + wb), wb, dev / max(wb, 1), lim))
            # a group is a whole number of windows (mvx_analyse_spec.h: GT): every window but the last one of a block row is full
            bpw = b / (ws + wb)
            print("       %.2f blocks per stage-2 window" % bpw + (" = %.1f windows per block row of %d blocks" % (nblkx0 / bpw, nblkx0) if lv == 0 else ""))
            # stage 2 in packed passes (mvx_analyse_spec.h: PACK): four strip-form windows in a row take seven passes, not eight; stage 1 is one pass per window
            print("       stage-2 passes run %d, saved by packing %d (%.1f %% of stage 2, %.1f %% of all row passes)" % (
                p2, saved, 100.0 * saved / max(p2 + saved, 1), 100.0 * saved / max(p2 + saved + ws + wb, 1))
                + (" = %.1f saved per block row of %d blocks (all groups packed: %d)" % (saved * (nblkx0 / bpw) / (ws + wb), nblkx0, nblkx0 // 28) if lv == 0 and blk - ov == 8 else ""))
            # run form (mvx_analyse_spec.h: RUN): a window of two or three runs of equal centres, every block with the pattern inside its limits, is two or three strips
            if r1 + r2 + r3 + r4 + rlim:
                nn = max(r1 + r2 + r3 + r4 + rlim, 1)
                print("       windows not in strip form by runs of equal centres: one %d, two %d (%.1f %%), three %d (%.1f %%), four or more %d (%.1f %%), a run outside its limits %d (%.1f %%)" % (
                    r1, r2, 100.0 * r2 / nn, r3, 100.0 * r3 / nn, r4, 100.0 * r4 / nn, rlim, 100.0 * rlim / nn))
                print("       run-form passes run %d, saved against block form %d (%.1f %% of stage 2, %.1f %% of all row passes)" % (
                    prun, rsaved, 100.0 * rsaved / max(p2 + rsaved, 1), 100.0 * rsaved / max(p2 + rsaved + ws + wb, 1)))
