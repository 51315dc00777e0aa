"""Rates of the temporal-radius filters through the VapourSynth filter shell (libmvtools_vs.so, MVX_VS_MULTI=1) driven by the mini host: a 1080p 8-bit 4:2:0
clip, blocks of 16 stepping by 8, pel 2, T request threads asking for output frames only --

    degrain3            mv.Super -> mv.Analyse x 6 -> mv.Degrain3          (the existing pipeline, for comparison: look-ahead windows, vectors handed over on the device)
    multidegrain r3     mv.Super -> mv.AnalyseN(radius=3) -> mv.DegrainN   (one search launch per frame, the multi blob downloaded into a property and uploaded again)
    multidegrain r8     the same at radius 8
    multicompensate tr3 mv.Super -> mv.AnalyseN(radius=3) -> mv.CompensateN: 7 output frames per source frame

each REPEATS times in one session.  Reported: source frames per second from the loaded clip to the last output frame -- graph construction INCLUDED, because creating
mv.Degrain3 reads frame 0 of its vector clips and so runs the first look-ahead windows of the existing pipeline there -- median and spread, the same over the requests for
the output clip alone, and the shell's upload / download thread-seconds (MVX_VS_STATS), which hold what moving the multi blob through a frame property costs.  Recorded, not gated.

    usage (GPU box):  python tools/multi_shell_bench.py [frames] [threads] [repeats]"""
import os
import re
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vapoursynth-mvtools_amd"), os.path.join(ROOT, "tests")]
import pipeline as pl  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 160
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16
REPEATS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
w, h, bits = 1920, 1080, 8
tmp = os.environ.get("TMPDIR", "/tmp")
src, out = os.path.join(tmp, "multi_bench_in.raw"), os.path.join(tmp, "multi_bench_out.raw")
frames = pl.moving_clip(w, h, bits, N, seed=3, noise=2)
with open(src, "wb") as f:
    for fr in frames:
        for p in fr:
            f.write(np.ascontiguousarray(p).tobytes())
host, plugin = os.path.join(ROOT, "vapoursynth-mvtools_amd", "mvx_vs_host"), os.path.join(ROOT, "vapoursynth-mvtools_amd", "libmvtools_vs.so")
env = dict(os.environ, MVX_VS_STATS="1", MVX_HOST_TIMES="1", MVX_VS_MULTI="1")
BLK = ["blksize=16", "overlap=8"]
RUNS = [
    ("degrain3", "degrain3", ["a." + a for a in BLK], 1),
    ("multidegrain radius 3", "multidegrain", ["m.radius=3"] + ["m." + a for a in BLK], 1),
    ("multidegrain radius 8", "multidegrain", ["m.radius=8"] + ["m." + a for a in BLK], 1),
    ("multicompensate tr 3", "multicompensate", ["m.radius=3"] + ["m." + a for a in BLK], 7),
]
print("%dx%d P%d, %d frames, %d request threads, %d repeats; blksize 16, overlap 8, pel 2" % (w, h, bits, N, T, REPEATS), flush=True)
for name, pipeline, args, per in RUNS:
    rates, req, moved = [], [], ""
    for _ in range(REPEATS):
        r = subprocess.run([host, plugin, "run", pipeline, src, str(w), str(h), str(bits), str(N), out] + args + ["x.threads=%d" % T, "x.order=frame"],
                           capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-500:] + r.stderr[-1500:]
        loaded = float(re.search(r"clip loaded at ([0-9.]+) s", r.stderr).group(1))
        built = float(re.search(r"graph built at ([0-9.]+) s", r.stderr).group(1))
        asked = float(re.search(r"output clip \(frame order\) ([0-9.]+) s", r.stderr).group(1))
        rates.append(N / (built - loaded + asked))
        req.append(N / max(asked, 0.005))
        m = re.search(r"upload=([0-9.]+)/(\d+) download=([0-9.]+)/(\d+)", r.stderr)
        if m:
            moved = "uploads %s thread-s in %s calls, downloads %s thread-s in %s calls (last repeat)" % m.groups()
    print("%-22s %7.1f source frames/s (median; %s)%s; the output requests alone %s   %s" % (
        name, statistics.median(rates), " ".join("%.1f" % v for v in rates), "  = %.1f output frames/s" % (per * statistics.median(rates)) if per > 1 else "",
        " ".join("%.1f" % v for v in req), moved), flush=True)
