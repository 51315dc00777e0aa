"""mv.DepanAnalyse / mv.DepanEstimate / mv.DepanCompensate / mv.DepanStabilise through the VapourSynth filter shell (vsplugin/mvtools_vs.c), which
registers them when the host's environment has MVX_VS_DEPAN=1 as the plugin is loaded.

CPU part: the function list with and without the switch (and beside MVX_VS_FLOW), creation errors and output clip info through the mini host's
`error` command.  DepanEstimate, DepanCompensate and DepanStabilise are created on DepanEstimate(clip) as their data clip, which needs no device and no
test double; only DepanAnalyse's creation reads frame 0 of a vector clip and runs over the test double of the device layer (tests/fakedev).

GPU part: one mini-host process per case on a 128 x 96 clip of 8 frames with a known global pan and one scene cut, blksize=8 overlap=4.  The expected
Depan_* values of DepanAnalyse are the estimator of tests/depan_ref.py on the CPU oracle's vectors, bit for bit; the expected frames of DepanCompensate
and DepanStabilise are the warps of tests/depan_ref.py and tests/depan_stab_ref.py with those motions, np.array_equal per plane.  DepanEstimate's values
are held to the restatement tests/depan_estimate_ref.py with the double FFT as tests/depan_estimate_checks.py holds the library: zeros and ones exact,
dx, dy, zoom within 4 D; DepanStabilise on DepanEstimate's data is expected from the data properties that very run printed, which checks the shell's
plumbing exactly without inheriting the FFT's tolerance.  Each case asserts, from the restatement alone, that it reaches what it is about."""
import re
import subprocess

import numpy as np
import pytest

import depan_estimate_cases as dec
import depan_estimate_checks as ck
import depan_estimate_ref as er
import depan_ref as dr
import depan_stab_ref as sr
import pipeline as pl
import test_vs_shim as shim
import vector_fields as vf
from test_vs_flow_shell import NEW as FLOW
from test_vs_shim import HOST, PLUGIN, _read_frames, _write_clip, host

f32 = np.float32
NEW = {  # MVDepan.cpp:4211-4288
    "DepanAnalyse": "clip:vnode;vectors:vnode;mask:vnode:opt;zoom:int:opt;rot:int:opt;pixaspect:float:opt;error:float:opt;info:int:opt;wrong:float:opt;zerow:float:opt;"
                    "thscd1:int:opt;thscd2:int:opt;fields:int:opt;tff:int:opt;",
    "DepanEstimate": "clip:vnode;trust:float:opt;winx:int:opt;winy:int:opt;wleft:int:opt;wtop:int:opt;dxmax:int:opt;dymax:int:opt;zoommax:float:opt;stab:float:opt;"
                     "pixaspect:float:opt;info:int:opt;show:int:opt;fields:int:opt;tff:int:opt;",
    "DepanCompensate": "clip:vnode;data:vnode;offset:float:opt;subpixel:int:opt;pixaspect:float:opt;matchfields:int:opt;mirror:int:opt;blur:int:opt;info:int:opt;fields:int:opt;"
                       "tff:int:opt;",
    "DepanStabilise": "clip:vnode;data:vnode;cutoff:float:opt;damping:float:opt;initzoom:float:opt;addzoom:int:opt;prev:int:opt;next:int:opt;mirror:int:opt;blur:int:opt;"
                      "dxmax:float:opt;dymax:float:opt;zoommax:float:opt;rotmax:float:opt;subpixel:int:opt;pixaspect:float:opt;fitlast:int:opt;tzoom:float:opt;info:int:opt;"
                      "method:int:opt;fields:int:opt;",
}


@pytest.fixture
def depan_on(monkeypatch):
    monkeypatch.delenv("MVX_VS_FLOW", raising=False)
    monkeypatch.setenv("MVX_VS_DEPAN", "1")  # (proc_env() copies os.environ)


@pytest.fixture
def double(monkeypatch, fakedev):
    """DepanAnalyse's creation reads frame 0 of its vector clip: mv.Super and mv.Analyse answer it over the test double of the device layer"""
    monkeypatch.setattr(shim, "_PRELOAD", fakedev)


def _listed():
    out = host("list").splitlines()
    assert out[0] == "id=com.nodame.mvtools ns=mv"
    return dict(line.split(" ", 1) for line in out[1:])


# ---------------------------------------------------------------------------------------------------- CPU

def test_switch_registers_exactly_the_four_filters(depan_on):
    assert _listed() == dict(shim.EXPECTED, **NEW)


def test_both_switches_register_the_nine_filters(depan_on, monkeypatch):
    monkeypatch.setenv("MVX_VS_FLOW", "1")
    assert _listed() == dict(shim.EXPECTED, **dict(FLOW, **NEW))


def test_without_the_switch_the_interface_is_unchanged(monkeypatch):
    monkeypatch.delenv("MVX_VS_FLOW", raising=False)
    for value in (None, "0"):
        if value is None:
            monkeypatch.delenv("MVX_VS_DEPAN", raising=False)
        else:
            monkeypatch.setenv("MVX_VS_DEPAN", value)
        assert _listed() == shim.EXPECTED
        assert host("error", "DepanEstimate", 128, 96, 8).strip() == "ERROR no function DepanEstimate"
    monkeypatch.setenv("MVX_VS_FLOW", "1")      # the other switch does not bring them either
    assert _listed() == dict(shim.EXPECTED, **FLOW)


NOTEXT = "%s: failed to invoke text.FrameProps: the host has no plugin com.vapoursynth.text."


@pytest.mark.parametrize("args,msg", [
    # the reference's texts (MVDepan.cpp:1326-1425, :2785-2828, :3977-4050), the first that applies
    (("DepanEstimate", 128, 96, 8, "e.trust=101.0"), "DepanEstimate: trust must be between 0.0 and 100.0 (inclusive)."),
    (("DepanEstimate", 128, 96, 8, "e.trust=101.0", "e.pixaspect=0.0"), "DepanEstimate: trust must be between 0.0 and 100.0 (inclusive)."),
    (("DepanEstimate", 128, 96, 8, "e.pixaspect=0.0", "e.winx=256"), "DepanEstimate: pixaspect must be positive."),
    (("DepanEstimate", 128, 96, 8, "e.winx=256"), "DepanEstimate: winx must not be greater than width-wleft."),
    (("DepanEstimate", 128, 96, 8, "e.winy=64", "e.dymax=32"), "DepanEstimate: dymax must be less than winy/2."),
    (("DepanCompensate", 128, 96, 8, "f.offset=11.0"), "DepanCompensate: offset must be between -10.0 and 10.0 (inclusive)."),
    (("DepanCompensate", 128, 96, 8, "f.offset=1.0", "f.subpixel=3", "f.mirror=16"), "DepanCompensate: subpixel must be between 0 and 2 (inclusive)."),
    (("DepanCompensate", 128, 96, 8, "f.offset=1.0", "f.blur=-1"), "DepanCompensate: blur must not be negative."),
    (("DepanStabilise", 128, 96, 8, "f.method=2"), "DepanStabilise: method must be between 0 and 1 (inclusive)."),
    (("DepanStabilise", 128, 96, 8, "f.cutoff=0.0", "f.method=2"), "DepanStabilise: cutoff must be greater than 0."),
    (("DepanStabilise", 128, 96, 8, "f.prev=-1"), "DepanStabilise: prev must not be negative."),
    # then the library's own
    (("DepanEstimate", 128, 96, 8, "e.winx=100"), "DepanEstimate: winx (after the halving for zoom) and winy must be powers of two between 8 and 8192."),
    (("DepanStabilise", 128, 96, 8, "f.tzoom=-1.0"), "DepanStabilise: tzoom must not be negative."),
    (("DepanCompensate", 128, 96, 8, "x.clip=2x2x8", "f.offset=1.0"), "DepanCompensate: every plane must be at least 2 samples wide and 2 high, and the frame at most 32767 x 32767."),
    # an unknown argument
    (("DepanEstimate", 128, 96, 8, "e.nosuch=1"), "DepanEstimate: Function does not take argument(s) named nosuch"),
    (("DepanCompensate", 128, 96, 8, "f.nosuch=1"), "DepanCompensate: Function does not take argument(s) named nosuch"),
    (("DepanStabilise", 128, 96, 8, "f.show=1"), "DepanStabilise: Function does not take argument(s) named show"),
    # info=1 on a host without the text plugin
    (("DepanEstimate", 128, 96, 8, "e.info=1", "x.notext=1"), NOTEXT % "DepanEstimate"),
    (("DepanCompensate", 128, 96, 8, "f.offset=1.0", "f.info=1", "x.notext=1"), NOTEXT % "DepanCompensate"),
    (("DepanStabilise", 128, 96, 8, "f.info=1", "x.notext=1"), NOTEXT % "DepanStabilise"),
])
def test_creation_errors_without_a_device(depan_on, args, msg):
    assert host("error", *args).strip() == "ERROR " + msg


@pytest.mark.parametrize("args,msg", [
    (("DepanAnalyse", 128, 96, 8, "f.pixaspect=0.0"), "DepanAnalyse: pixaspect must be positive."),
    (("DepanAnalyse", 128, 96, 8, "a.delta=2"), "DepanAnalyse: vectors clip must be created with delta=1."),
    (("DepanAnalyse", 128, 96, 8, "f.pixaspect=-1.0", "a.delta=2"), "DepanAnalyse: pixaspect must be positive."),
    (("DepanAnalyse", 128, 96, 8, "f.nosuch=1"), "DepanAnalyse: Function does not take argument(s) named nosuch"),
    (("DepanAnalyse", 128, 96, 8, "f.info=1", "x.notext=1"), NOTEXT % "DepanAnalyse"),
])
def test_creation_errors_of_depananalyse(depan_on, double, args, msg):
    assert host("error", *args).strip() == "ERROR " + msg


def test_info_invokes_frameprops_with_the_filters_property(depan_on):
    for filt, pre in (("DepanEstimate", "e"), ("DepanCompensate", "f"), ("DepanStabilise", "f")):
        out = host("error", filt, 128, 96, 8, pre + ".info=1").strip().split("\n")
        assert out == ["text.FrameProps props=%s_info" % filt, "OK 128x96 frames=4"], filt
        assert host("error", filt, 128, 96, 8).strip() == "OK 128x96 frames=4"      # and not without info


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("fmt", ["420", "422", "444", "gray"])
def test_output_clip_info(depan_on, fmt, bits):
    extra = [] if fmt == "420" else ["x.format=" + fmt]
    for filt in ("DepanEstimate", "DepanCompensate", "DepanStabilise"):
        assert host("error", filt, 128, 96, bits, *extra).strip() == "OK 128x96 frames=4", filt


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("fmt", ["420", "422", "444", "gray"])
def test_output_clip_info_of_depananalyse(depan_on, double, fmt, bits):
    extra = [] if fmt == "420" else ["x.format=" + fmt]
    assert host("error", "DepanAnalyse", 128, 96, bits, *extra).strip() == "OK 128x96 frames=4"


# ---------------------------------------------------------------------------------------------------- GPU

gpu = pytest.mark.gpu
W, H, NF, CUT = 128, 96, 8, 4
PAN = (4, -2)           # per frame, even: the 4:2:0 chroma planes pan by whole samples too
B84 = dict(blksize=8, overlap=4)


def pan_clip(bits=8):
    """8 frames cut from one canvas (tests/depan_estimate_cases.py: low-pass noise), each displaced by PAN from the one before; from frame CUT on, from another"""
    m = 40
    out = []
    for n in range(NF):
        seed = 900 if n < CUT else 950
        k = n if n < CUT else n - CUT
        planes = []
        for p in range(3):
            s = 2 if p else 1
            c = dec.canvas(H // s + 2 * m, W // s + 2 * m, bits, seed + p, smooth=1, power=2 if p == 0 else 1)
            oy, ox = m + k * PAN[1] // s, m + k * PAN[0] // s
            planes.append(np.ascontiguousarray(c[oy:oy + H // s, ox:ox + W // s]))
        out.append(planes)
    return out


class Clip:
    """the clip on disk and what the CPU oracle and the restatements make of it"""

    def __init__(self, oracle, tmp_path, bits=8):
        self.bits, self.dir = bits, tmp_path
        self.frames = pan_clip(bits)
        self.src = tmp_path / "in.raw"
        _write_clip(self.src, self.frames)
        self.osup = oracle.Super(W, H, bits)
        self.osf = [self.osup.frame(f) for f in self.frames]
        self.an, self.blobs = {}, {}
        for isb in (0, 1):
            a = oracle.Analyse(self.osup, num_frames=NF, isb=isb, delta=1, **B84)
            inside = lambda k: self.osf[k] if 0 <= k < NF else None
            self.an[isb] = a
            self.blobs[isb] = [a.frame(self.osf[n], inside(n + 1 if isb else n - 1)) for n in range(NF)]

    def motions(self, isb, top_field=None, **kw):
        """depan_ref's estimator on the oracle's vectors -> per frame dict(dx, dy, zoom, rot, iter, error)"""
        ad = self.an[isb].ad
        _, s1, s2 = vf.scaled_thresholds(ad, 400)
        ref = dr.Analyse(ad, W, H, s1, s2, **kw)
        return [ref.frame(self.blobs[isb][max(0, n - 1) if isb else n], None, bool(top_field[n]) if top_field else False) for n in range(NF)]

    def run(self, pipeline, *args, name="out.raw"):
        path = self.dir / name
        cmd = [HOST, PLUGIN] + [str(a) for a in ("run", pipeline, self.src, W, H, self.bits, NF, path)] + ["a.%s=%s" % kv for kv in B84.items()] + list(args)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=shim.proc_env(MVX_VS_DEPAN="1"))
        assert r.returncode == 0 and "DONE" in r.stdout, r.stdout + r.stderr
        return r.stdout, path

    def read(self, path):
        return _read_frames(path, W, H, self.bits, NF)


def printed(stdout):
    """-> per frame (dx, dy, zoom, rot) as float32 from the hex floats, the info strings by property name, and the property lines as printed"""
    props, info, lines = {}, {}, []
    for line in stdout.splitlines():
        m = re.match(r"frame (\d+) Depan_dx=(\S+) Depan_dy=(\S+) Depan_zoom=(\S+) Depan_rot=(\S+)$", line)
        if m:
            props[int(m.group(1))] = tuple(f32(float.fromhex(v)) for v in m.groups()[1:])
            lines.append(line)
        m = re.match(r"frame (\d+) (Depan\w+_info)=(.*)$", line)
        if m:
            info.setdefault(m.group(2), {})[int(m.group(1))] = m.group(3)
    assert sorted(props) == list(range(NF))
    return [props[n] for n in range(NF)], info, lines


def _bits(values):
    return [int(f32(v).view(np.uint32)) for v in values]


def _same(got, want, what):
    assert len(got) == len(want), what
    for n, (g, w) in enumerate(zip(got, want)):
        for p in range(len(w)):
            assert np.array_equal(g[p], w[p]), "%s frame %d plane %d: %s" % (what, n, p, pl.first_diff(g[p], w[p]))


@pytest.fixture
def clip(oracle, tmp_path):
    c = Clip(oracle, tmp_path)
    # a condition on the INPUT, from the CPU oracle's vectors alone: every frame has a result but frame 0 and the frame after the cut -- no case passes on an
    # all-zero data clip.  (Backward vectors: frame 0 reads the vectors of frame 0 against frame 1 and has a result, :287.)
    fw, bw = c.motions(0), c.motions(1)
    assert [m["dx"] != 0 for m in fw] == [n not in (0, CUT) for n in range(NF)]
    assert [m["dx"] != 0 for m in bw] == [n != CUT for n in range(NF)]
    assert all(abs(m["dx"] - PAN[0]) < 0.5 and abs(m["dy"] - PAN[1]) < 0.5 for n, m in enumerate(fw) if n not in (0, CUT))
    return c


ANALYSE_INFO = "fn=%d iter=%d error=%.3f dx=%.2f dy=%.2f rot=%.3f zoom=%.5f"


@gpu
@pytest.mark.parametrize("isb,kw", [(0, {}), (1, {}), (0, dict(zoom=0, rot=0)), (1, dict(zoom=0)), (0, dict(fields=1))], ids=repr)
def test_depananalyse_equals_the_estimator_on_the_oracles_vectors(clip, isb, kw):
    top = [1 ^ (n % 2) for n in range(NF)] if kw.get("fields") else None            # x.fieldorder=1
    want = clip.motions(isb, top, **{k: bool(v) for k, v in kw.items()})
    args = ["n.%s=%s" % i for i in kw.items()] + ["n.info=1"] + ([] if isb else ["x.vectors=fw"]) + (["x.fieldorder=1"] if top else [])
    out, path = clip.run("depananalyse", *args)
    got, info, _ = printed(out)
    for n in range(NF):
        assert _bits(got[n]) == _bits([want[n][k] for k in ("dx", "dy", "zoom", "rot")]), (n, got[n], want[n])
        m = want[n]
        assert info["DepanAnalyse_info"][n] == ANALYSE_INFO % (n, m["iter"], m["error"], m["dx"], m["dy"], m["rot"], m["zoom"])
    assert "text.FrameProps props=DepanAnalyse_info" in out
    _same(clip.read(path), clip.frames, "DepanAnalyse returns the clip's frames")


@gpu
def test_depananalyse_with_a_mask_clip(clip):
    """the mask's luma plane weighs the blocks (:309-313): zero over the left third, random elsewhere; the restatement reads the same plane"""
    rng = np.random.default_rng(77)
    luma = rng.integers(1, 256, (H, W)).astype(np.uint8)
    luma[:, :W // 3] = 0
    masks = [[np.roll(luma, n, axis=0), np.full((H // 2, W // 2), 128, np.uint8), np.full((H // 2, W // 2), 128, np.uint8)] for n in range(NF)]
    path = clip.dir / "mask.raw"
    _write_clip(path, masks)
    ad = clip.an[0].ad
    _, s1, s2 = vf.scaled_thresholds(ad, 400)
    ref = dr.Analyse(ad, W, H, s1, s2, has_mask=True)
    want = [ref.frame(clip.blobs[0][n], masks[n][0]) for n in range(NF)]
    plain = clip.motions(0)
    assert any(_bits(_quad(a)) != _bits(_quad(b)) for a, b in zip(want, plain)) and sum(m["dx"] != 0 for m in want) >= 4     # the mask changes results
    out, _ = clip.run("depananalyse", "x.vectors=fw", "x.mask=%s" % path)
    assert [_bits(g) for g in printed(out)[0]] == [_bits(_quad(m)) for m in want]


@gpu
def test_depananalyse_without_field_property_is_the_references_error(clip):
    cmd = [HOST, PLUGIN] + [str(a) for a in ("run", "depananalyse", clip.src, W, H, 8, NF, clip.dir / "o.raw")] + ["a.blksize=8", "a.overlap=4", "n.fields=1", "x.vectors=fw"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=shim.proc_env(MVX_VS_DEPAN="1"))
    assert "ERROR output frame: DepanAnalyse: _Field property not found in input frame. Therefore, you must pass tff argument." in r.stdout
    out, _ = clip.run("depananalyse", "n.fields=1", "n.tff=1", "x.vectors=fw")
    want = clip.motions(0, [1 ^ (n % 2) for n in range(NF)], fields=True)
    assert [_bits(g) for g in printed(out)[0]] == [_bits([m[k] for k in ("dx", "dy", "zoom", "rot")]) for m in want]


def _quad(m):
    return (m["dx"], m["dy"], m["zoom"], m["rot"])


@gpu
@pytest.mark.parametrize("fargs", [dict(offset="1.0", subpixel=2), dict(offset="-1.0", subpixel=1), dict(offset="1.0", subpixel=0), dict(offset="-1.0", subpixel=2, mirror=15, blur=2),
                                   dict(offset="1.5", subpixel=2, info=1)], ids=repr)
def test_depancompensate_on_depananalyse_equals_the_restatement(clip, fargs):
    motions = [_quad(m) for m in clip.motions(0)]
    offset = float(fargs["offset"])
    want, warped, passed, infos = [], 0, 0, {}
    for n in range(NF):
        fm = dr.frame_map(offset, n, NF)
        if fm is None:
            want.append(clip.frames[n])
            passed += 1
            continue
        nsrc, start, end = fm
        trsum, mo = dr.motion_to_transform([motions[k] for k in range(start + 1, end + 1)], offset, W, H)
        warped += not np.array_equal(trsum, dr.null())
        want.append(dr.compensate_frame(clip.frames[nsrc], trsum, fargs["subpixel"], 8, (1, 1), False, fargs.get("mirror", 0), fargs.get("blur", 0)))
        infos[n] = "offset=%.2f, %d to %d, dx=%.2f, dy=%.2f, rot=%.3f zoom=%.5f" % (f32(offset), nsrc, n, mo[0], mo[1], mo[3], mo[2])
    assert warped >= 1 and passed >= 1
    out, path = clip.run("depancompensate", "x.data=analyse", "x.vectors=fw", *["f.%s=%s" % i for i in fargs.items()])
    got, info, _ = printed(out)
    assert [_bits(g) for g in got] == [_bits(m) for m in motions]
    _same(clip.read(path), want, "DepanCompensate")
    if fargs.get("info"):
        assert info["DepanCompensate_info"] == infos


def _stab_expected(c, motions, **kw):
    e = sr.Stabilise(W, H, NF, fps=(24, 1), **kw)
    plans = [e.plan(n, motions) for n in range(NF)]
    src = lambda s: None if s is None else (c.frames[s["frame"]], s["tr"])
    return e, plans, [e.paint(c.frames[n], p["tr"], src(p["prev"]), src(p["next"])) for n, p in enumerate(plans)]


STAB = dict(cutoff="0.5", mirror=15, blur=2, subpixel=2, prev=2, next=2)
STAB_INFO = "frame=%d %s=%d dx=%.2f dy=%.2f rot=%.3f zoom=%.5f"


def _stab_kw(fargs):
    return {k: (float(v) if isinstance(v, str) else v) for k, v in fargs.items() if k != "info"}


@gpu
@pytest.mark.parametrize("method", [0, 1])
def test_depanstabilise_on_depananalyse_equals_the_restatement(clip, method):
    motions = [_quad(m) for m in clip.motions(0)]
    fargs = dict(STAB, method=method, info=1)
    e, plans, want = _stab_expected(clip, motions, **_stab_kw(fargs))
    stats = {}
    for n, p in enumerate(plans):
        e.paint(clip.frames[n], p["tr"], (clip.frames[p["prev"]["frame"]], p["prev"]["tr"]), (clip.frames[p["next"]["frame"]], p["next"]["tr"]), stats)
    assert all(p["prev"] is not None and p["next"] is not None for p in plans) and stats["from_prev"] and stats["from_next"] and stats["from_cur"]
    assert plans[CUT]["base"]
    out, path = clip.run("depanstabilise", "x.data=analyse", "x.vectors=fw", *["f.%s=%s" % i for i in fargs.items()])
    got, info, _ = printed(out)
    assert [_bits(g) for g in got] == [_bits(m) for m in motions]
    _same(clip.read(path), want, "DepanStabilise")
    for n, p in enumerate(plans):
        mo = p["motion"]
        assert info["DepanStabilise_info"][n] == STAB_INFO % (n, "BASE!" if p["base"] else "base ", p["nbase"], mo[0], mo[1], mo[3], mo[2])


def _estimate_expected(c, **kw):
    e = er.Estimate(W, H, 8, num_frames=NF, **kw)
    luma = [f[0] for f in c.frames]
    out = {}
    for which, fft in ((64, er.FFT64), (32, er.FFT32)):
        ref = [e.pair(luma[max(0, n - 1)], luma[n], n, fft) for n in range(NF)]
        out[which] = (ref, [e.finish(n, [ref[max(0, n - 1)], ref[n], ref[min(n + 1, NF - 1)]]) for n in range(NF)])
    return e, out


@gpu
@pytest.mark.parametrize("kw", [{}, dict(zoommax="1.2", winx=128, winy=64, wtop=32), dict(winx=64, winy=32, dxmax=20, dymax=10)], ids=repr)
def test_depanestimate_is_held_to_the_double_restatement(clip, kw):
    e, ref = _estimate_expected(clip, **{k: (float(v) if isinstance(v, str) else v) for k, v in kw.items()})
    res, want = ref[64]
    # conditions on the input: both FFTs of the restatement decide alike, and the clip has results and a scene change
    assert [[v == 0 for v in m[:2]] + [m[2] == 1] for m in want] == [[v == 0 for v in m[:2]] + [m[2] == 1] for m in ref[32][1]]
    assert [m[0] != 0 for m in want] == [n not in (0, CUT) for n in range(NF)]
    D = ck.D()
    # and the independent single-precision FFT of the restatement is itself within the bound on this clip and these windows: D comes from other scenes
    assert all(abs(float(a[q]) - float(b[q])) <= 4 * D[k] for a, b in zip(want, ref[32][1]) for q, k in enumerate(("dx", "dy", "zoom")))
    if "zoommax" in kw:
        assert any(m[2] != 1 for m in want)
    out, path = clip.run("depanestimate", "e.info=1", *["e.%s=%s" % i for i in kw.items()])
    got, info, _ = printed(out)
    for n in range(NF):
        g, w = got[n], want[n]
        print("frame %d: dx off by %.3g (4 D = %.3g), dy %.3g (%.3g), zoom %.3g (%.3g)" % (n, abs(g[0] - float(w[0])), 4 * D["dx"], abs(g[1] - float(w[1])), 4 * D["dy"],
                                                                                       abs(g[2] - float(w[2])), 4 * D["zoom"]))
        assert [v == 0 for v in g[:2]] == [v == 0 for v in w[:2]] and (g[2] == 1) == (w[2] == 1) and g[3] == 0
        assert abs(g[0] - float(w[0])) <= 4 * D["dx"] and abs(g[1] - float(w[1])) <= 4 * D["dy"] and abs(g[2] - float(w[2])) <= 4 * D["zoom"]
        m = re.match(r"fn=(\d+) dx=(\S+) dy=(\S+) zoom=(\S+) trust=(\S+)$", info["DepanEstimate_info"][n])
        assert m and int(m.group(1)) == n and m.group(2) == "%.2f" % g[0] and m.group(3) == "%.2f" % g[1] and m.group(4) == "%.5f" % g[2]
        assert abs(float(m.group(5)) - float(res[n]["trust"])) <= 4 * D["trust"] + 0.005          # (%.2f rounds by at most 0.005)
    _same(clip.read(path), clip.frames, "DepanEstimate returns the clip's frames")


@gpu
@pytest.mark.parametrize("method", [0, 1])
def test_depanstabilise_on_depanestimate_equals_the_restatement_on_the_printed_data(clip, method):
    fargs = dict(STAB, method=method)
    out, path = clip.run("depanstabilise", "x.data=estimate", *["f.%s=%s" % i for i in fargs.items()])
    motions, _, _ = printed(out)
    assert [m[0] != 0 for m in motions] == [n not in (0, CUT) for n in range(NF)]
    _, plans, want = _stab_expected(clip, motions, **_stab_kw(fargs))
    assert plans[CUT]["base"]
    _same(clip.read(path), want, "DepanStabilise on DepanEstimate")


@gpu
def test_depancompensate_on_depanestimate_equals_the_restatement_on_the_printed_data(clip):
    out, path = clip.run("depancompensate", "f.offset=1.0", "f.subpixel=2")
    motions, _, _ = printed(out)
    want = []
    for n in range(NF):
        fm = dr.frame_map(1.0, n, NF)
        want.append(clip.frames[n] if fm is None else dr.compensate_frame(clip.frames[fm[0]], dr.motion_to_transform([motions[n]], 1.0, W, H)[0], 2, 8, (1, 1), False, 0, 0))
    _same(clip.read(path), want, "DepanCompensate on DepanEstimate")


@gpu
def test_depanestimate_does_not_depend_on_the_order_of_requests(clip):
    runs = [printed(clip.run("depanestimate", *extra, name="o%d.raw" % k)[0])[2] for k, extra in enumerate([(), ("x.threads=8", "x.order=frame"), ("x.cache=2",),
                                                                                                         ("x.threads=8", "x.order=frame", "x.cache=2", "e.show=1")])]
    assert len(runs[0]) == NF and runs[0] == runs[1] == runs[2] == runs[3]


@gpu
def test_depanestimate_show_paints_the_window_rows_of_the_output_frame(clip):
    import test_gpu_depan_show as show
    e, ref = _estimate_expected(clip)
    plain, _ = clip.run("depanestimate", name="plain.raw")
    out, path = clip.run("depanestimate", "e.show=1")
    assert printed(out)[2] == printed(plain)[2]
    got = clip.read(path)
    rows, cols = slice(e.wtop, e.wtop + e.winy), slice(e.wleft, e.wleft + e.winx)
    tol = max(1, 4 * show.Dshow())
    for n in range(NF):
        want = [p.copy() for p in clip.frames[n]]
        outside = np.ones((H, W), bool)
        outside[rows, cols] = False
        assert np.array_equal(got[n][0][outside], want[0][outside]) and np.array_equal(got[n][1], want[1]) and np.array_equal(got[n][2], want[2])
        painted = show.paint(ref[64][0][n]["surfaces"][0], 255)
        off = int(abs(got[n][0][rows, cols].astype(np.int64) - painted).max())
        print("frame %d: the painted window is off by at most %d (max(1, 4 Dshow) = %d)" % (n, off, tol))
        assert off <= tol
