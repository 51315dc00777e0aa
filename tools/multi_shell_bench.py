"""Rates of the temporal-radius filters through the VapourSynth filter shell (libmvtools_vs.so, MVX_VS_MULTI=1) driven by the mini host: a 1080p 8-bit 4:2:0
clip, blocks of 16 stepping by 8, pel 2, T request threads asking for output frames only --

    degrain3            mv.Super -> mv.Analyse x 6 -> mv.Degrain3          (the existing pipeline, for comparison: look-ahead windows, vectors handed over on the device)
    multidegrain r3     mv.Super -> mv.AnalyseN(radius=3) -> mv.DegrainN   (look-ahead windows of MVX_VS_MULTI_LOOKAHEAD frames; the multi blob goes through a frame property)
    multidegrain r8     the same at radius 8
    multicompensate tr3 mv.Super -> mv.AnalyseN(radius=3) -> mv.CompensateN: 7 output frames per source frame
    multirecalculate r3 mv.Super -> mv.AnalyseN(radius=3) -> mv.RecalculateN to blocks of 8 stepping by 4 (one call per frame): the vector clip itself is the output

each under several settings of the environment (the column `lookahead` = MVX_VS_MULTI_LOOKAHEAD; "-" = unset: the default window length, mvx_win_default_length; 0 = one
call per frame), REPEATS times in one session.  With --against DIR every pipeline is also run, with nothing set, on the plugin
DIR/libmvtools_vs.so -- another build of the shell, e.g. the parent commit's -- turn and turn about with this tree's, so that both see the same state of the machine; the
mini host is this tree's either way.  Reported: source frames per second from the loaded clip to the last output frame -- graph construction INCLUDED, because creating
mv.Degrain3 reads frame 0 of its vector clips and so runs the first look-ahead windows of the existing pipeline there -- median and the repeats, the same over the
requests for the output clip alone, the shell's upload / download thread-seconds (MVX_VS_STATS) and its AnalyseN counters.  Every mini-host process runs under its own
time limit and the first one that fails ends the session.  Recorded, not gated.

With --float the session is another one: multidegrain at radius 3 on a 1080p 16-bit clip, and the same graph with the float switch (MVX_VS_FLOAT=1) on the float clip whose
quantised copy that 16-bit clip is -- mv.Super and mv.DegrainN on float samples, mv.AnalyseN on the 16-bit clip, so both graphs use the same vectors -- turn and turn about.
The float graph moves twice the bytes per frame over PCIe in each direction.

    usage (GPU box):  python tools/multi_shell_bench.py [frames] [threads] [repeats] [--against DIR | --float]"""
import os
import re
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vapoursynth-mvtools_amd"), os.path.join(ROOT, "tests")]
import pipeline as pl  # noqa: E402

argv = sys.argv[1:]
AGAINST = None
if "--against" in argv:
    i = argv.index("--against")
    AGAINST = os.path.abspath(argv[i + 1])
    del argv[i:i + 2]
FLOAT = "--float" in argv
if FLOAT:
    argv.remove("--float")
N = int(argv[0]) if len(argv) > 0 else 160
T = int(argv[1]) if len(argv) > 1 else 16
REPEATS = int(argv[2]) if len(argv) > 2 else 3
LIMIT = 180  # seconds a mini-host process may take
w, h, bits = 1920, 1080, 16 if FLOAT else 8
tmp = os.environ.get("TMPDIR", "/tmp")
src, out = os.path.join(tmp, "multi_bench_in.raw"), os.path.join(tmp, "multi_bench_out.raw")
frames = pl.moving_clip(w, h, bits, N, seed=3, noise=2)
with open(src, "wb") as f:
    for fr in frames:
        for p in fr:
            f.write(np.ascontiguousarray(p).tobytes())
fsrc = os.path.join(tmp, "multi_bench_in_float.raw")
if FLOAT:   # luma in [0, 1], chroma in [-0.5, 0.5]: round(x * 65535) (chroma: of x + 0.5) is the 16-bit clip
    with open(fsrc, "wb") as f:
        for fr in frames:
            for p, a in enumerate(fr):
                f.write((a.astype(np.float64) / 65535.0 - (0.5 if p else 0.0)).astype(np.float32).tobytes())
host = os.path.join(ROOT, "vapoursynth-mvtools_amd", "mvx_vs_host")
PLUGINS = {"this": os.path.join(ROOT, "vapoursynth-mvtools_amd", "libmvtools_vs.so")}
if AGAINST:
    PLUGINS["other"] = os.path.join(AGAINST, "libmvtools_vs.so")
BLK = ["blksize=16", "overlap=8"]
M3, M8 = ["m.radius=3"] + ["m." + a for a in BLK], ["m.radius=8"] + ["m." + a for a in BLK]
# name, pipeline, arguments, output frames per source frame, the default window length (for its neighbours)
PIPELINES = [
    ("degrain3", "degrain3", ["a." + a for a in BLK], 1, None),
    ("multidegrain radius 3", "multidegrain", M3, 1, 128),
    ("multidegrain radius 8", "multidegrain", M8, 1, 48),
    ("multicompensate tr 3", "multicompensate", M3, 7, 128),
    ("multirecalculate radius 3", "multirecalculate", M3 + ["r.blksize=8", "r.overlap=4", "r.thsad=200"], 1, None),
]
RUNS = []          # (plugin, name, pipeline, args, per, lookahead)
if FLOAT:
    RUNS = [("this", "multidegrain radius 3, 16-bit", "multidegrain", M3, 1, "-"), ("this", "multidegrain radius 3, float", "multidegrain", M3 + ["x.float=" + fsrc], 1, "-")]
    PIPELINES = []
for name, pipeline, args, per, default in PIPELINES:
    if AGAINST:
        RUNS.append(("other", name, pipeline, args, per, "-"))
    RUNS.append(("this", name, pipeline, args, per, "-"))
    if default:   # its neighbours, and one call per frame: the shape of the work before the windows
        RUNS += [("this", name, pipeline, args, per, la) for la in (str(default // 2), str(default * 2), "0")]

print("%dx%d P%d, %d frames, %d request threads, %d repeats; blksize 16, overlap 8, pel 2%s" % (w, h, bits, N, T, REPEATS, "; other = " + os.path.relpath(AGAINST, ROOT) if AGAINST else ""), flush=True)
results = {i: dict(rates=[], req=[], moved="", counters="") for i in range(len(RUNS))}
for _ in range(REPEATS):      # repeats outermost: the two plugins, and the settings of a pipeline, take turns
    for i, (plugin, name, pipeline, args, per, la) in enumerate(RUNS):
        env = dict(os.environ, MVX_VS_STATS="1", MVX_HOST_TIMES="1", MVX_VS_MULTI="1", **({"MVX_VS_FLOAT": "1"} if FLOAT else {}))
        env.pop("MVX_VS_MULTI_LOOKAHEAD", None)
        if la != "-":
            env["MVX_VS_MULTI_LOOKAHEAD"] = la
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT), host, PLUGINS[plugin], "run", pipeline, src, str(w), str(h), str(bits), str(N), out] + args +
                           ["x.threads=%d" % T, "x.order=frame"], capture_output=True, text=True, env=env)
        if r.returncode != 0 or "DONE" not in r.stdout:   # nothing more is started on the GPU after a run that failed
            print("FAILED (%d): %s %s lookahead=%s\n%s" % (r.returncode, plugin, name, la, r.stdout[-500:] + r.stderr[-1500:]), flush=True)
            sys.exit(1)
        loaded = float(re.search(r"clip loaded at ([0-9.]+) s", r.stderr).group(1))
        built = float(re.search(r"graph built at ([0-9.]+) s", r.stderr).group(1))
        asked = float(re.search(r"output clip \(frame order\) ([0-9.]+) s", r.stderr).group(1))
        res = results[i]
        res["rates"].append(N / (built - loaded + asked))
        res["req"].append(N / max(asked, 0.005))
        m = re.search(r"upload=([0-9.]+)/(\d+) download=([0-9.]+)/(\d+)", r.stderr)
        if m:
            res["moved"] = "uploads %s thread-s in %s calls, downloads %s thread-s in %s calls" % m.groups()
        m = re.search(r"mvtools_vs: AnalyseN (.*)", r.stderr)
        res["counters"] = m.group(1) if m else ""

print("%-6s %-26s %9s  %s" % ("plugin", "pipeline", "lookahead", "source frames/s: median (repeats) [spread]; the output requests alone; the last repeat's transfers and counters"))
for i, (plugin, name, pipeline, args, per, la) in enumerate(RUNS):
    res = results[i]
    med = statistics.median(res["rates"])
    print("%-6s %-26s %9s  %7.1f (%s) [%.1f]%s; %s   %s   %s" % (
        plugin, name, la, med, " ".join("%.1f" % v for v in res["rates"]), max(res["rates"]) - min(res["rates"]),
        "  = %.1f output frames/s" % (per * med) if per > 1 else "", " ".join("%.1f" % v for v in res["req"]), res["moved"], res["counters"]), flush=True)
