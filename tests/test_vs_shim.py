"""The VapourSynth API-4 filter shell (vsplugin/mvtools_vs.c) driven through the in-repo mini host (vsplugin/minihost.c).

CPU part: the plugin loads, registers the reference's plugin id / namespace / function names / argument strings
(src/EntryPoint.c:28-33, src/MVSuper.c:279-291, src/MVAnalyse.c:639-671, src/MVDegrains.cpp:813-932,
src/MVCompensate.c:579-592) and reports the reference's creation-time errors.  Graph part: whole filter graphs
(Super -> Analyse x2 -> Degrain / Compensate / BlockFPS / Recalculate / Finest / SCDetection) evaluated frame by frame through the shell
equal the oracle.  Every graph test takes the `shell` fixture and so runs twice: `[device-...]` on the GPU (-m gpu), `[double-...]` on a
CPU-only machine with the test double of the device layer in front of the library (tests/fakedev/mvx_fakedev.c) -- the same plugin, the
same mini host, the oracle's kernels: what that run tests is the shell's own logic.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import pipeline as pl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vapoursynth-mvtools_amd")
HOST = os.path.join(PKG, "mvx_vs_host")
PLUGIN = os.path.join(PKG, "libmvtools_vs.so")


_PRELOAD = None  # the `shell` fixture's "double" mode: path of the test double of the device layer (tests/fakedev), else None


def proc_env(**extra):
    """environment of a mini-host process in the current mode"""
    e = dict(os.environ)
    if _PRELOAD:
        e["LD_PRELOAD"] = _PRELOAD
        # the test double reports 64 MiB of free device memory so that the frame cache really evicts; the look-ahead windows are sized from
        # the free memory too (r4) -- the tests that count launches mean the default window length
        e.setdefault("MVX_VS_LOOKAHEAD_AUTOSIZE", "0")
    e.update(extra)
    return e


def host(*args, check=True):
    if not (os.path.exists(HOST) and os.path.exists(PLUGIN)):
        sys.path.insert(0, PKG)
        import build
        build.build()
    r = subprocess.run([HOST, PLUGIN] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=proc_env())
    if check:
        assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.fixture(params=[pytest.param("device", marks=pytest.mark.gpu), "double"])
def shell(request):
    """Every graph test of the shell runs twice: on the GPU (`device`, -m gpu), and on a CPU-only machine over the test double of the
    device layer (`double`: tests/fakedev/mvx_fakedev.c in front of the library, oracle kernels) -- there it tests the shell's own logic."""
    global _PRELOAD
    _PRELOAD = request.getfixturevalue("fakedev") if request.param == "double" else None  # (built only when a CPU twin runs)
    yield request.param
    _PRELOAD = None


DEGRAIN_TAIL = "thsad:int:opt;thsadc:int:opt;plane:int:opt;limit:int:opt;limitc:int:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;"
EXPECTED = {
    "Super": "clip:vnode;hpad:int:opt;vpad:int:opt;pel:int:opt;levels:int:opt;chroma:int:opt;sharp:int:opt;rfilter:int:opt;pelclip:vnode:opt;opt:int:opt;",
    "Analyse": "super:vnode;blksize:int:opt;blksizev:int:opt;levels:int:opt;search:int:opt;searchparam:int:opt;pelsearch:int:opt;isb:int:opt;lambda:int:opt;"
               "chroma:int:opt;delta:int:opt;truemotion:int:opt;lsad:int:opt;plevel:int:opt;global:int:opt;pnew:int:opt;pzero:int:opt;pglobal:int:opt;"
               "overlap:int:opt;overlapv:int:opt;divide:int:opt;badsad:int:opt;badrange:int:opt;opt:int:opt;meander:int:opt;trymany:int:opt;fields:int:opt;"
               "tff:int:opt;search_coarse:int:opt;dct:int:opt;",
    "Finest": "super:vnode;opt:int:opt;",
    "SCDetection": "clip:vnode;vectors:vnode;thscd1:int:opt;thscd2:int:opt;",
    "Recalculate": "super:vnode;vectors:vnode;thsad:int:opt;smooth:int:opt;blksize:int:opt;blksizev:int:opt;search:int:opt;searchparam:int:opt;lambda:int:opt;"
                   "chroma:int:opt;truemotion:int:opt;pnew:int:opt;overlap:int:opt;overlapv:int:opt;divide:int:opt;opt:int:opt;meander:int:opt;fields:int:opt;"
                   "tff:int:opt;dct:int:opt;",
    "BlockFPS": "clip:vnode;super:vnode;mvbw:vnode;mvfw:vnode;num:int:opt;den:int:opt;mode:int:opt;ml:float:opt;blend:int:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;",
    "Compensate": "clip:vnode;super:vnode;vectors:vnode;scbehavior:int:opt;thsad:int:opt;fields:int:opt;time:float:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;tff:int:opt;",
}
_v = "clip:vnode;super:vnode;"
for _r in range(1, 7):
    _v += "mvbw%s:vnode;mvfw%s:vnode;" % (("", "") if _r == 1 else (_r, _r))
    EXPECTED["Degrain%d" % _r] = _v + DEGRAIN_TAIL


def test_plugin_registers_reference_interface():
    out = host("list").splitlines()
    assert out[0] == "id=com.nodame.mvtools ns=mv"
    got = dict(line.split(" ", 1) for line in out[1:])
    assert got == EXPECTED


def test_plugin_exports_only_the_entry_point():
    syms = subprocess.run(["nm", "-D", "--defined-only", PLUGIN], capture_output=True, text=True).stdout
    names = [l.split()[-1] for l in syms.splitlines() if " T " in l]
    assert names == ["VapourSynthPluginInit2"]  # src/EntryPoint.c:28, everything else hidden (meson.build:15)


@pytest.mark.parametrize("args,msg", [
    (("Super", 640, 360, 8, "f.pel=3"), "Super: pel must be 1, 2, or 4."),
    (("Super", 640, 360, 8, "f.sharp=3"), "Super: sharp must be between 0 and 2 (inclusive)."),
    (("Super", 640, 360, 8, "f.rfilter=9"), "Super: rfilter must be between 0 and 4 (inclusive)."),
    (("Super", 640, 360, 8, "f.nosuch=1"), "Super: Function does not take argument(s) named nosuch"),
    (("Super", 640, 360, 8, "f.pel=2", "x.pelw=1000", "x.pelh=720"), "Super: pelclip's dimensions must be multiples of the input clip's dimensions."),
    (("Super", 640, 360, 8, "f.pel=2", "x.pelw=1280", "x.pelh=720", "x.pelbits=16"), "Super: pelclip must have the same format as the input clip, and it must have constant dimensions."),
    (("AnalyseOnClip", 640, 360, 8), "Analyse: required properties not found in first frame of super clip. Maybe clip didn't come from mv.Super? Was the first frame trimmed away?"),
])
def test_creation_errors_without_gpu(args, msg):
    assert host("error", *args).strip() == "ERROR " + msg


def test_super_create_reports_geometry_without_gpu():
    assert host("error", "Super", 640, 360, 8, "f.pel=1").strip() == "OK 672x978 frames=4"
    # a pelclip of either accepted size, or any size with pel=1 (ignored, src/MVSuper.c:240), creates fine
    assert host("error", "Super", 640, 360, 8, "f.pel=2", "x.pelw=1280", "x.pelh=720").strip().startswith("OK ")
    assert host("error", "Super", 640, 360, 8, "f.pel=2", "x.pelw=%d" % ((640 + 32) * 2), "x.pelh=%d" % ((360 + 32) * 2)).strip().startswith("OK ")
    assert host("error", "Super", 640, 360, 8, "f.pel=1", "x.pelw=100", "x.pelh=100").strip() == "OK 672x978 frames=4"


CLIP_MISMATCHES = ["x.clip=144x96x8", "x.clip=128x96x16"]  # `clip` with another width, another depth than the super clip's source


@pytest.mark.parametrize("mismatch", CLIP_MISMATCHES)
@pytest.mark.parametrize("filt", ["Degrain1", "Compensate", "BlockFPS"])
def test_clip_must_be_the_one_the_super_clip_was_made_from(fakedev, monkeypatch, filt, mismatch):
    """The kernels address the clip's planes with the super clip's geometry and sample size: every filter that takes both refuses a `clip`
    that is not the super clip's source, in the reference's words.  (CPU only: frame 0 of the super and vector clips comes from the test double.)"""
    monkeypatch.setattr(sys.modules[__name__], "_PRELOAD", fakedev)
    assert host("error", filt, 128, 96, 8, mismatch).strip() == "ERROR %s: wrong source or super clip frame size." % filt


def _write_clip(path, frames):
    with open(path, "wb") as f:
        for fr in frames:
            for p in fr:
                f.write(np.ascontiguousarray(p).tobytes())


def _read_frames(path, w, h, bits, n):
    dt = np.uint8 if bits == 8 else np.uint16
    data = np.fromfile(path, dtype=dt)
    per = w * h + 2 * (w // 2) * (h // 2)
    assert data.size == per * n
    out = []
    for i in range(n):
        d = data[i * per:(i + 1) * per]
        out.append([d[:w * h].reshape(h, w), d[w * h:w * h + (w // 2) * (h // 2)].reshape(h // 2, w // 2), d[w * h + (w // 2) * (h // 2):].reshape(h // 2, w // 2)])
    return out


@pytest.mark.parametrize("bits", [8, 16])
def test_creation_errors_with_real_frames(shell, bits):
    # these need frame 0 of the super / vector clips, i.e. a GPU
    assert host("error", "Analyse", 128, 96, bits, "f.blksize=7").strip().startswith("ERROR Analyse: the block size must be")
    assert host("error", "Analyse", 128, 96, bits, "s.levels=1", "f.levels=3").strip() == "ERROR Analyse: super clip has 1 levels. Analyse needs 3 levels."
    assert host("error", "Degrain1Swapped", 128, 96, bits).strip() == "ERROR Degrain1: mvfw must be generated with isb=False."
    assert host("error", "Degrain1", 128, 96, bits, "f.plane=7").strip() == "ERROR Degrain1: plane must be between 0 and 4 (inclusive)."
    assert host("error", "Degrain1", 128, 96, bits, "f.limit=%d" % (1 << bits)).strip() == "ERROR Degrain1: limit must be between 0 and %d (inclusive)." % ((1 << bits) - 1)
    assert host("error", "Degrain1", 128, 96, bits).strip().startswith("OK 128x96")


@pytest.mark.parametrize("w,h,bits,nf,sargs,aargs", [(128, 96, 8, 4, {}, dict(blksize=8, overlap=4)), (192, 112, 16, 3, dict(pel=1), dict(blksize=16, overlap=8))])
def test_shell_super_and_analyse_match_oracle(shell, oracle, tmp_path, w, h, bits, nf, sargs, aargs):
    frames = pl.moving_clip(w, h, bits, nf, seed=31, noise=3)
    src = tmp_path / "in.raw"
    _write_clip(src, frames)
    osup = oracle.Super(w, h, bits, **sargs)
    osf = [osup.frame(f) for f in frames]
    cli = ["s.%s=%s" % kv for kv in sargs.items()] + ["a.%s=%s" % kv for kv in aargs.items()]
    # Super: defined regions equal, Super_* props on frame 0
    out = host("run", "super", src, w, h, bits, nf, tmp_path / "sup.raw", *cli)
    info = osup.s
    assert out.splitlines()[0] == "super %dx%d Super_height=%d Super_hpad=%d Super_vpad=%d Super_pel=%d Super_modeyuv=%d Super_levels=%d" % (
        info.superWidth, info.superHeight, h, info.hpad, info.vpad, info.pel, info.modeYUV, info.levels)
    dt = np.uint8 if bits == 8 else np.uint16
    raw = np.fromfile(tmp_path / "sup.raw", dtype=dt)
    sw, sh = info.superWidth, info.superHeight
    per = sw * sh + 2 * (sw // 2) * (sh // 2)
    assert raw.size == per * nf
    for n in range(nf):
        d = raw[n * per:(n + 1) * per]
        got = [d[:sw * sh].reshape(sh, sw), d[sw * sh:sw * sh + (sw // 2) * (sh // 2)].reshape(sh // 2, sw // 2), d[sw * sh + (sw // 2) * (sh // 2):].reshape(sh // 2, sw // 2)]
        assert not pl.defined_equal(osup, osf[n], got)
    # Analyse: both props byte-identical (nMagicKey / nVersion / nCPUFlags are host dependent in the reference)
    host("run", "analyse", src, w, h, bits, nf, tmp_path / "vec.raw", *cli)
    blob = np.fromfile(tmp_path / "vec.raw", dtype=np.uint8)
    off = 0
    for n in range(nf):
        for isb in (1, 0):
            oan = oracle.Analyse(osup, num_frames=nf, isb=isb, delta=1, **aargs)
            nref = n + 1 if isb else n - 1
            want = oan.frame(osf[n], osf[nref] if 0 <= nref < nf else None)
            ad = np.frombuffer(bytes(oan.ad), dtype=np.int32)
            got_ad = blob[off:off + 84].view(np.int32)
            keep = [i for i, (k, _) in enumerate(oracle.AnalysisData._fields_) if k not in ("nMagicKey", "nVersion", "nCPUFlags")]
            assert np.array_equal(got_ad[keep], ad[keep])
            off += 84
            assert np.array_equal(blob[off:off + want.size], want), (n, isb)
            off += want.size
    assert off == blob.size


@pytest.mark.parametrize("w,h,bits,radius,dargs", [(128, 96, 8, 1, {}), (192, 112, 16, 2, dict(thsad=300, limit=2000)), (128, 96, 8, 3, dict(plane=0))])
def test_shell_degrain_matches_oracle(shell, oracle, tmp_path, w, h, bits, radius, dargs):
    nf = 2 * radius + 2
    aargs = dict(blksize=8, overlap=4)
    frames = pl.moving_clip(w, h, bits, nf, seed=33, noise=3)
    src = tmp_path / "in.raw"
    _write_clip(src, frames)
    cli = ["a.%s=%s" % kv for kv in aargs.items()] + ["d.%s=%s" % kv for kv in dargs.items()]
    host("run", "degrain%d" % radius, src, w, h, bits, nf, tmp_path / "out.raw", *cli)
    got = _read_frames(tmp_path / "out.raw", w, h, bits, nf)
    osup = oracle.Super(w, h, bits)
    osf = [osup.frame(f) for f in frames]
    ans = {(d, isb): oracle.Analyse(osup, num_frames=nf, isb=isb, delta=d, **aargs) for d in range(1, radius + 1) for isb in (1, 0)}
    odg = oracle.Degrain(radius, osup, ans[(1, 1)].ad, **dargs)
    for n in range(nf):
        refs, blobs = [], []
        for d in range(1, radius + 1):
            for isb in (1, 0):
                nref = n + d if isb else n - d
                r = osf[nref] if 0 <= nref < nf else None
                refs.append(r)
                blobs.append(ans[(d, isb)].frame(osf[n], r))
        want = odg.frame(frames[n], refs, blobs)
        for p in range(3):
            assert np.array_equal(got[n][p], want[p]), (n, p)


FORMATS = {"444": dict(subsampling=(0, 0)), "422": dict(subsampling=(1, 0)), "gray": dict(gray=True)}


def _fmt_clip(w, h, bits, nf, fmt, seed):
    frames = pl.moving_clip(w, h, bits, nf, seed=seed, noise=3, sub=FORMATS[fmt].get("subsampling", (1, 1)))
    return [[f[0]] for f in frames] if fmt == "gray" else frames


def _read_fmt_frames(path, w, h, bits, n, fmt):
    dt = np.uint8 if bits == 8 else np.uint16
    sw, sh = FORMATS[fmt].get("subsampling", (1, 1))
    dims = [(h, w)] if fmt == "gray" else [(h, w), (h >> sh, w >> sw), (h >> sh, w >> sw)]
    data = np.fromfile(path, dtype=dt)
    per = sum(a * b for a, b in dims)
    assert data.size == per * n
    out = []
    for i in range(n):
        d, o, fr = data[i * per:(i + 1) * per], 0, []
        for a, b in dims:
            fr.append(d[o:o + a * b].reshape(a, b))
            o += a * b
        out.append(fr)
    return out


@pytest.mark.parametrize("fmt,bits,pipeline,aargs,fargs", [
    ("444", 8, "degrain1", dict(blksize=8, overlap=4), {}),
    ("444", 16, "degrain2", dict(blksize=16, overlap=8), dict(limit=2000)),
    ("422", 8, "degrain1", dict(blksize=16, overlap=8), {}),
    ("422", 16, "degrain1", dict(blksize=8, overlap=4), dict(plane=3)),
    ("gray", 8, "degrain1", dict(blksize=8, overlap=4), {}),
    ("gray", 16, "degrain2", dict(blksize=16, overlap=0), {}),
    ("444", 8, "compensate", dict(blksize=8, overlap=4), dict(thsad=5000)),
    ("422", 16, "compensate", dict(blksize=16, overlap=8), {}),
    ("gray", 8, "compensate", dict(blksize=8, overlap=0), {}),
])
def test_shell_other_chroma_formats_match_oracle(shell, oracle, tmp_path, fmt, bits, pipeline, aargs, fargs):
    """r6: the whole graph -- mv.Super -> mv.Analyse -> mv.DegrainN / mv.Compensate -- through the filter shell on 4:4:4, 4:2:2 and Gray clips (MVDegrains.cpp:693-776,
    MVCompensate.c:543, MVAnalyse.c:463-517 accept them; the C-ABI cases are tests/test_gpu_formats.py)"""
    w, h = 128, 96
    radius = int(pipeline[7:]) if pipeline.startswith("degrain") else 1
    nf = 2 * radius + 2
    frames = _fmt_clip(w, h, bits, nf, fmt, seed=37)
    src = tmp_path / "in.raw"
    _write_clip(src, frames)
    key = "d" if pipeline.startswith("degrain") else "c"
    cli = ["a.%s=%s" % kv for kv in aargs.items()] + ["%s.%s=%s" % (key, k, v) for k, v in fargs.items()] + ["x.format=" + fmt]
    host("run", pipeline, src, w, h, bits, nf, tmp_path / "out.raw", *cli)
    got = _read_fmt_frames(tmp_path / "out.raw", w, h, bits, nf, fmt)
    osup = oracle.Super(w, h, bits, **FORMATS[fmt])
    osf = [osup.frame(f) for f in frames]
    ans = {(d, isb): oracle.Analyse(osup, num_frames=nf, isb=isb, delta=d, **aargs) for d in range(1, radius + 1) for isb in (1, 0)}
    if pipeline.startswith("degrain"):
        odg = oracle.Degrain(radius, osup, ans[(1, 1)].ad, **fargs)
    else:
        ocp = oracle.Compensate(osup, ans[(1, 1)].ad, **fargs)
    for n in range(nf):
        if pipeline.startswith("degrain"):
            refs, blobs = [], []
            for d in range(1, radius + 1):
                for isb in (1, 0):
                    nref = n + d if isb else n - d
                    r = osf[nref] if 0 <= nref < nf else None
                    refs.append(r)
                    blobs.append(ans[(d, isb)].frame(osf[n], r))
            want = odg.frame(frames[n], refs, blobs)
        else:
            r = osf[n + 1] if n + 1 < nf else None
            want = ocp.frame(osf[n], r, ans[(1, 1)].frame(osf[n], r))
        for p in range(len(want)):
            assert np.array_equal(got[n][p], want[p]), (fmt, n, p)


def test_shell_compensate_matches_oracle(shell, oracle, tmp_path):
    w, h, bits, nf = 128, 96, 8, 4
    aargs = dict(blksize=8, overlap=4)
    frames = pl.moving_clip(w, h, bits, nf, seed=35, noise=3)
    src = tmp_path / "in.raw"
    _write_clip(src, frames)
    host("run", "compensate", src, w, h, bits, nf, tmp_path / "out.raw", *["a.%s=%s" % kv for kv in aargs.items()], "c.thsad=5000")
    got = _read_frames(tmp_path / "out.raw", w, h, bits, nf)
    osup = oracle.Super(w, h, bits)
    osf = [osup.frame(f) for f in frames]
    oan = oracle.Analyse(osup, num_frames=nf, isb=1, delta=1, **aargs)
    ocp = oracle.Compensate(osup, oan.ad, thsad=5000)
    for n in range(nf):
        r = osf[n + 1] if n + 1 < nf else None
        want = ocp.frame(osf[n], r, oan.frame(osf[n], r))
        for p in range(3):
            assert np.array_equal(got[n][p], want[p]), (n, p)


@pytest.mark.parametrize("bits,pel,padded", [(8, 2, False), (16, 4, False), (8, 2, True)])
def test_shell_super_pelclip_matches_oracle(shell, oracle, tmp_path, bits, pel, padded):
    w, h, nf = 128, 96, 2
    frames = pl.moving_clip(w, h, bits, nf, seed=38, noise=3)
    osup = oracle.Super(w, h, bits, pel=pel)
    pw, ph = ((w + 2 * osup.s.hpad) * pel, (h + 2 * osup.s.vpad) * pel) if padded else (w * pel, h * pel)
    rng = np.random.default_rng(5)
    dt = np.uint8 if bits == 8 else np.uint16
    pelframes = [[rng.integers(0, 1 << bits, (ph >> (1 if p else 0), pw >> (1 if p else 0)), dtype=dt) for p in range(3)] for _ in frames]
    _write_clip(tmp_path / "in.raw", frames)
    _write_clip(tmp_path / "pel.raw", pelframes)
    host("run", "super", tmp_path / "in.raw", w, h, bits, nf, tmp_path / "sup.raw", "s.pel=%d" % pel, "x.pelclip=%s" % (tmp_path / "pel.raw"), "x.pelw=%d" % pw, "x.pelh=%d" % ph)
    raw = np.fromfile(tmp_path / "sup.raw", dtype=dt)
    sw, sh = osup.s.superWidth, osup.s.superHeight
    per = sw * sh + 2 * (sw // 2) * (sh // 2)
    assert raw.size == per * nf
    for n in range(nf):
        d = raw[n * per:(n + 1) * per]
        got = [d[:sw * sh].reshape(sh, sw), d[sw * sh:sw * sh + (sw // 2) * (sh // 2)].reshape(sh // 2, sw // 2), d[sw * sh + (sw // 2) * (sh // 2):].reshape(sh // 2, sw // 2)]
        assert not pl.defined_equal(osup, osup.frame_pelclip(frames[n], pelframes[n]), got)


@pytest.mark.parametrize("how", ["tff1", "tff0", "props1", "props0"])
def test_shell_fields_match_oracle(shell, oracle, tmp_path, how):
    """fields=True through the shell: parity from tff (overrides) or from the frames' _Field props (src/MVAnalyse.c:135-179,
    src/MVCompensate.c:188-225); Analyse and Compensate both apply the +-pel/2 shift"""
    w, h, bits, nf, pel = 128, 96, 8, 4, 2
    aargs = dict(blksize=8, overlap=4)
    frames = pl.moving_clip(w, h, bits, nf, seed=36, noise=3)
    src = tmp_path / "in.raw"
    _write_clip(src, frames)
    order = int(how[-1])
    extra = ["a.tff=%d" % order, "c.tff=%d" % order] if how.startswith("tff") else ["x.fieldorder=%d" % order]
    cli = ["a.%s=%s" % kv for kv in aargs.items()] + ["a.fields=1", "c.fields=1", "c.thsad=5000"] + extra
    host("run", "analyse", src, w, h, bits, nf, tmp_path / "vec.raw", *cli)
    host("run", "compensate", src, w, h, bits, nf, tmp_path / "out.raw", *cli)
    got = _read_frames(tmp_path / "out.raw", w, h, bits, nf)
    blob = np.fromfile(tmp_path / "vec.raw", dtype=np.uint8)
    osup = oracle.Super(w, h, bits)
    assert osup.s.pel == pel
    osf = [osup.frame(f) for f in frames]
    ans = {isb: oracle.Analyse(osup, num_frames=nf, isb=isb, delta=1, fields=1, **aargs) for isb in (1, 0)}
    ocp = oracle.Compensate(osup, ans[1].ad, thsad=5000)
    off, shifts = 0, set()
    for n in range(nf):
        for isb in (1, 0):
            nref = n + 1 if isb else n - 1
            r = osf[nref] if 0 <= nref < nf else None
            if how.startswith("tff"):
                fs, miss = oracle.field_shift(1, pel, n, nref, tff=order)
            else:
                fs, miss = oracle.field_shift(1, pel, n, nref, src_field=order ^ (n % 2), ref_field=order ^ (nref % 2))
            assert not miss
            if r is not None:
                shifts.add(fs)
            want = ans[isb].frame(osf[n], r, field_shift=fs if r is not None else 0)
            off += 84
            assert np.array_equal(blob[off:off + want.size], want), (n, isb)
            off += want.size
            if isb:
                wantc = ocp.frame(osf[n], r, want, field_shift=fs if r is not None else 0)
                for p in range(3):
                    assert np.array_equal(got[n][p], wantc[p]), (n, p)
    assert shifts == {1, -1}


def test_shell_fields_need_parity_information(shell):
    # no _Field prop on the frames and no tff: a frame-time error in the reference's words
    msg = "_Field property not found in input frame. Therefore, you must pass tff argument."
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        frames = pl.moving_clip(128, 96, 8, 3, seed=37, noise=3)
        _write_clip(os.path.join(d, "in.raw"), frames)
        out = host("run", "analyse", os.path.join(d, "in.raw"), 128, 96, 8, 3, os.path.join(d, "o.raw"), "a.fields=1", check=False)
        assert "Analyse: " + msg in out
        out = host("run", "compensate", os.path.join(d, "in.raw"), 128, 96, 8, 3, os.path.join(d, "o.raw"), "c.fields=1", check=False)
        assert "Compensate: " + msg in out
        # the same request through the admission gate's error leg: the filter error returned the permit before the graph was freed
        r = subprocess.run([HOST, PLUGIN, "run", "compensate", os.path.join(d, "in.raw"), "128", "96", "8", "3", os.path.join(d, "o.raw"), "c.fields=1", "x.free=1"],
                           capture_output=True, text=True, timeout=600, env=proc_env())
        assert "Compensate: " + msg in r.stdout and "FREED" in r.stdout, r.stdout + r.stderr
        assert "permits out" not in r.stderr, r.stderr[-2000:]
        out = host("run", "recalculate", os.path.join(d, "in.raw"), 128, 96, 8, 3, os.path.join(d, "o.raw"), "r.fields=1", check=False)
        assert "Recalculate: " + msg in out
        out = host("run", "recalculate", os.path.join(d, "in.raw"), 128, 96, 8, 3, os.path.join(d, "o.raw"), "r.fields=1", "r.tff=1")
        assert "DONE" in out
    assert host("error", "Compensate", 128, 96, 8, "s.pel=1", "f.fields=1").strip() == "ERROR Compensate: fields option requires pel > 1."


@pytest.mark.parametrize("bits,bargs", [(8, dict(num=60, den=1)), (16, dict(num=60, den=1, mode=4, ml="40.0")), (8, dict(num=60, den=1, thscd1=20, thscd2=10))])
def test_shell_blockfps_matches_oracle(shell, oracle, tmp_path, bits, bargs):
    w, h, nf = 128, 96, 5
    aargs = dict(blksize=8, overlap=4)
    frames = pl.moving_clip(w, h, bits, nf, seed=37, noise=3)
    src = tmp_path / "in.raw"
    _write_clip(src, frames)
    out = host("run", "blockfps", src, w, h, bits, nf, tmp_path / "out.raw", *["a.%s=%s" % kv for kv in aargs.items()], *["b.%s=%s" % kv for kv in bargs.items()])
    osup = oracle.Super(w, h, bits)
    osf = [osup.frame(f) for f in frames]
    abw = oracle.Analyse(osup, num_frames=nf, isb=1, delta=1, **aargs)
    afw = oracle.Analyse(osup, num_frames=nf, isb=0, delta=1, **aargs)
    bbw = [abw.frame(osf[n], osf[n + 1] if n + 1 < nf else None) for n in range(nf)]
    bfw = [afw.frame(osf[n], osf[n - 1] if n >= 1 else None) for n in range(nf)]
    kw = {k: (float(v) if k == "ml" else v) for k, v in bargs.items()}
    ob = oracle.BlockFPS(osup, abw.ad, afw.ad, nf, 24, 1, **kw)  # the mini host's source clip runs at 24/1
    lines = out.splitlines()
    assert lines[0] == "blockfps frames=%d fps=%d/%d" % (ob.num_frames, ob.d.outFpsNum, ob.d.outFpsDen)
    assert lines[1] == "frame1 _DurationNum=%d _DurationDen=%d" % (ob.d.outFpsDen, ob.d.outFpsNum)  # std.AssumeFPS ran (MVBlockFPS.c:989-1014)
    got = _read_frames(tmp_path / "out.raw", w, h, bits, ob.num_frames)
    for n in range(ob.num_frames):
        want = ob.frame(n, frames, osf, bbw, bfw)
        for p in range(3):
            assert np.array_equal(got[n][p], want[p][:, :got[n][p].shape[1]]), (n, p, ob.map(n))


@pytest.mark.parametrize("bits,aargs,rargs,dargs", [(8, dict(blksize=16, overlap=8), dict(blksize=8, overlap=4, thsad=100), {}),
                                                    (16, dict(blksize=16, overlap=8, divide=2), dict(blksize=8, overlap=4, thsad=60, divide=1), {})])
def test_shell_recalculate_and_divide_match_oracle(shell, oracle, tmp_path, bits, aargs, rargs, dargs):
    w, h, nf = 192, 128, 3
    frames = pl.moving_clip(w, h, bits, nf, seed=39, noise=3)
    src = tmp_path / "in.raw"
    _write_clip(src, frames)
    host("run", "recalculate", src, w, h, bits, nf, tmp_path / "vec.raw", *["a.%s=%s" % kv for kv in aargs.items()], *["r.%s=%s" % kv for kv in rargs.items()])
    blob = np.fromfile(tmp_path / "vec.raw", dtype=np.uint8)
    osup = oracle.Super(w, h, bits)
    osf = [osup.frame(f) for f in frames]
    off = 0
    keep = [i for i, (k, _) in enumerate(oracle.AnalysisData._fields_) if k not in ("nMagicKey", "nVersion", "nCPUFlags")]
    for n in range(nf):
        for isb in (1, 0):
            oan = oracle.Analyse(osup, num_frames=nf, isb=isb, delta=1, **aargs)
            nref = n + 1 if isb else n - 1
            ref = osf[nref] if 0 <= nref < nf else None
            orc = oracle.Recalculate(osup, oan.ad, **rargs)
            want = orc.frame(osf[n], ref, oan.frame(osf[n], ref))
            ad = np.frombuffer(bytes(orc.ad), dtype=np.int32)
            assert np.array_equal(blob[off:off + 84].view(np.int32)[keep], ad[keep])
            off += 84
            assert np.array_equal(blob[off:off + want.size], want), (n, isb)
            off += want.size
    assert off == blob.size


def test_shell_finest_and_scdetection(shell, oracle, tmp_path):
    w, h, bits, nf = 128, 96, 8, 3
    frames = pl.moving_clip(w, h, bits, nf, seed=43, noise=3)
    src = tmp_path / "in.raw"
    _write_clip(src, frames)
    osup = oracle.Super(w, h, bits)
    out = host("run", "finest", src, w, h, bits, nf, tmp_path / "fin.raw")
    fw, fh = (w + 32) * 2, (h + 32) * 2
    assert out.splitlines()[0] == "finest %dx%d" % (fw, fh)
    got = _read_frames(tmp_path / "fin.raw", fw, fh, bits, nf)
    for n in range(nf):
        want = osup.finest(osup.frame(frames[n]))
        for p in range(3):
            assert np.array_equal(got[n][p], want[p]), (n, p)
    # SCDetection: the clip passes through, the prop is _SceneChangeNext for backward vectors and _SceneChangePrev for forward ones;
    # frames whose reference lies outside the clip carry invalid vectors = scene change (MVSCDetection.c:62-64, Fakery.c:144-146)
    out = host("run", "scdetection", src, w, h, bits, nf, tmp_path / "sc.raw", "a.blksize=8", "a.overlap=4").splitlines()
    assert out[:nf] == ["bw frame %d next=%d prev=-1" % (n, 1 if n == nf - 1 else 0) for n in range(nf)]
    assert out[nf:2 * nf] == ["fw frame %d next=-1 prev=%d" % (n, 1 if n == 0 else 0) for n in range(nf)]
    passthrough = _read_frames(tmp_path / "sc.raw", w, h, bits, nf)
    for n in range(nf):
        for p in range(3):
            assert np.array_equal(passthrough[n][p], frames[n][p])


@pytest.mark.parametrize("bits,pipeline,extra", [(8, "degrain1", ("a.blksize=8", "a.overlap=4")), (16, "degrain3", ("a.blksize=16", "a.overlap=8")), (16, "analyse", ("a.blksize=16", "a.overlap=8"))])
def test_concurrent_requests_are_batched_and_bit_identical(shell, tmp_path, bits, pipeline, extra):
    """fmParallel (src/MVAnalyse.c:634): 64 worker threads request frames at once.  The shell's combining queue turns the concurrent
    getFrame calls of one Analyse instance into a single search launch; the clip that comes out must be the one the frame-by-frame
    evaluation gives (which the other tests compare with the oracle)."""
    w, h, n = 192, 112, 70
    frames = pl.moving_clip(w, h, bits, n, seed=17, noise=3)
    src, seq, par = str(tmp_path / "in.raw"), str(tmp_path / "seq.raw"), str(tmp_path / "par.raw")
    _write_clip(src, frames)
    assert "DONE" in host("run", pipeline, src, w, h, bits, n, seq, *extra)
    env = proc_env(MVX_VS_STATS="1", MVX_VS_BATCH_WAIT_US="20000")
    r = subprocess.run([HOST, PLUGIN] + [str(a) for a in ("run", pipeline, src, w, h, bits, n, par)] + list(extra) + ["x.threads=64"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout + r.stderr
    assert open(seq, "rb").read() == open(par, "rb").read()
    stats = [l for l in r.stderr.splitlines() if l.startswith("mvtools_vs: Analyse")]
    assert len(stats) == 1, r.stderr
    kv = {k: int(v) for k, v in (t.split("=") for t in stats[0].split()[2:])}
    # every Analyse instance served its 70 frames in a handful of launches, the largest with most of the 64 concurrent requests
    assert kv["jobs"] == n * kv["instances"] and kv["launches"] <= 8 * kv["instances"] and kv["largest_batch"] >= 32, stats[0]


def test_lookahead_windows_shrink_with_the_device_memory(fakedev, tmp_path):
    """the look-ahead windows (length, number ahead) are sized from the free device memory; on a device that cannot hold the
    default three windows of 128 frames the vector clip is still the per-frame path's, served from shorter windows -- or, when not even one
    small window fits, by the per-frame path itself.  (CPU only: the test double reports the memory MVX_FAKEDEV_MEM names.)"""
    global _PRELOAD
    _PRELOAD = fakedev
    try:
        w, h, n, bits = 192, 112, 60, 16
        frames = pl.moving_clip(w, h, bits, n, seed=23, noise=3)
        src, ref = str(tmp_path / "in.raw"), str(tmp_path / "ref.raw")
        _write_clip(src, frames)
        args = [str(a) for a in ("run", "degrain1", src, w, h, bits, n)]
        extra = ["a.blksize=16", "a.overlap=8", "x.threads=8"]
        r0 = subprocess.run([HOST, PLUGIN] + args + [ref] + extra, capture_output=True, text=True, timeout=900, env=proc_env(MVX_VS_LOOKAHEAD="0"))
        assert r0.returncode == 0 and "DONE" in r0.stdout, r0.stdout + r0.stderr
        for mem, expect in ((str(24 << 20), "short"), (str(1 << 20), "off")):
            out = str(tmp_path / ("la_%s.raw" % expect))
            r1 = subprocess.run([HOST, PLUGIN] + args + [out] + extra, capture_output=True, text=True, timeout=900,
                                env=proc_env(MVX_VS_STATS="1", MVX_VS_LOOKAHEAD_AUTOSIZE="1", MVX_FAKEDEV_MEM=mem))
            assert r1.returncode == 0 and "DONE" in r1.stdout, r1.stdout + r1.stderr
            assert open(ref, "rb").read() == open(out, "rb").read(), expect
            stats = [l for l in r1.stderr.splitlines() if l.startswith("mvtools_vs: Analyse")]
            kv = {k: int(v) for k, v in (t.split("=") for t in stats[0].split()[2:])}
            assert kv["jobs"] == n * kv["instances"], stats[0]
            if expect == "short":
                assert 1 < kv["largest_batch"] < 128, stats[0]   # windows, but not the default ones
    finally:
        _PRELOAD = None


@pytest.mark.parametrize("bits,pipeline,extra,threads", [(16, "degrain3", ("a.blksize=16", "a.overlap=8"), 32), (8, "degrain1", ("a.blksize=8", "a.overlap=4"), 1),
                                                          (8, "analyse", ("a.blksize=8", "a.overlap=4", "a.delta=2"), 8)])
def test_lookahead_serves_windows_and_is_bit_identical(shell, tmp_path, bits, pipeline, extra, threads):
    """mv.Analyse on this plugin's own mv.Super node computes its vector clip a window of 128 frames at a time (one search launch per
    window, super frames built on the device from the SOURCE frames; the request protocol stays MVAnalyse.c:84-113's arInitial /
    arAllFramesReady).  The clip must be the one the per-frame path gives (MVX_VS_LOOKAHEAD=0, which the other tests tie to the oracle),
    with at least ten times fewer launches than frames."""
    w, h, n = 192, 112, 150
    frames = pl.moving_clip(w, h, bits, n, seed=19, noise=3)
    src, ref, la = str(tmp_path / "in.raw"), str(tmp_path / "ref.raw"), str(tmp_path / "la.raw")
    _write_clip(src, frames)
    args = [str(a) for a in ("run", pipeline, src, w, h, bits, n)]
    r0 = subprocess.run([HOST, PLUGIN] + args + [ref] + list(extra) + ["x.threads=16"], capture_output=True, text=True, timeout=900, env=proc_env(MVX_VS_LOOKAHEAD="0"))
    assert r0.returncode == 0 and "DONE" in r0.stdout, r0.stdout + r0.stderr
    r1 = subprocess.run([HOST, PLUGIN] + args + [la] + list(extra) + ["x.threads=%d" % threads], capture_output=True, text=True, timeout=900, env=proc_env(MVX_VS_STATS="1"))
    assert r1.returncode == 0 and "DONE" in r1.stdout, r1.stdout + r1.stderr
    assert open(ref, "rb").read() == open(la, "rb").read()
    stats = [l for l in r1.stderr.splitlines() if l.startswith("mvtools_vs: Analyse")]
    assert len(stats) == 1, r1.stderr
    kv = {k: int(v) for k, v in (t.split("=") for t in stats[0].split()[2:])}
    assert kv["jobs"] == n * kv["instances"] and kv["launches"] * 10 <= kv["jobs"] and kv["largest_batch"] == 128, stats[0]


@pytest.mark.parametrize("bits,pipeline,extra,env", [
    (16, "degrain3", ("a.blksize=16", "a.overlap=8"), {}),
    (8, "degrain1", ("a.blksize=8", "a.overlap=4"), {"MVX_VS_LOOKAHEAD": "0", "MVX_VS_CACHE_FRAMES": "6"}),  # per-frame path, a cache so small that consumers rebuild super frames from the embedded source
    (16, "compensate", ("a.blksize=16", "a.overlap=8"), {"MVX_VS_LOOKAHEAD": "8"}),             # short look-ahead windows
])
def test_lazy_super_frames_are_bit_identical(shell, tmp_path, bits, pipeline, extra, env):
    """MVX_VS_SUPER_LAZY=1 (opt-in, r4): mv.Super's frames carry the source picture instead of the super pixels, which stay on the device; a
    consumer that finds no device copy rebuilds it from that picture with the mv.Super instance's own handle.  Every filter of the plugin
    takes its super frames through that path, so the output clip must be the default mode's, byte for byte."""
    w, h, n = 192, 112, 70
    frames = pl.moving_clip(w, h, bits, n, seed=23, noise=3)
    src, ref, lazy = str(tmp_path / "in.raw"), str(tmp_path / "ref.raw"), str(tmp_path / "lazy.raw")
    _write_clip(src, frames)
    args = [str(a) for a in ("run", pipeline, src, w, h, bits, n)]
    r0 = subprocess.run([HOST, PLUGIN] + args + [ref] + list(extra) + ["x.threads=8"], capture_output=True, text=True, timeout=900, env=proc_env(**env))
    assert r0.returncode == 0 and "DONE" in r0.stdout, r0.stdout + r0.stderr
    r1 = subprocess.run([HOST, PLUGIN] + args + [lazy] + list(extra) + ["x.threads=8", "x.order=frame"], capture_output=True, text=True, timeout=900,
                        env=proc_env(MVX_VS_SUPER_LAZY="1", **env))
    assert r1.returncode == 0 and "DONE" in r1.stdout, r1.stdout + r1.stderr
    assert open(ref, "rb").read() == open(lazy, "rb").read()
