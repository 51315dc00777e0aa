"""mv.FlowInter / mv.FlowFPS / mv.Flow / mv.FlowBlur / mv.Mask through the VapourSynth filter shell (vsplugin/mvtools_vs.c), which registers
them when the host's environment has MVX_VS_FLOW=1 as the plugin is loaded.

CPU part: the function list with and without the switch, creation errors and output clip info through the mini host's `error` command.  The
five mvx_*_create calls touch no device; frame 0 of the super and vector clips, which every creation reads, comes from the test double of the
device layer (tests/fakedev).

GPU part: whole graphs -- Super -> Analyse x2 -> FlowFPS | FlowInter | FlowBlur, Super -> Analyse -> Flow | Mask -- evaluated through getFrame by
one mini-host process per case.  The expected frames are the CPU restatements (tests/flow_ref.py, flowmc_ref.py, mask_ref.py) fed the CPU oracle's
super frames (as Finest frames) and vectors; never the Python package's or the shell's.  Comparison is np.array_equal per plane.  Each case
asserts the path its frames took in the restatement (last_kind, the counters), so that it cannot pass without reaching it.

mv.Mask's cases only use exponents that take no pow (kind 0 at gamma 2, kinds 1 and 2 at gamma 1, kinds 3-5), where the library is exact
(include/mvtools_amd.h); the restatement's pow_dist stays infinite, which is asserted.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import flow_ref
import flowmc_ref
import mask_ref
import pipeline as pl
import test_vs_shim as shim
from test_vs_shim import HOST, PLUGIN, _fmt_clip, _read_fmt_frames, _read_frames, _write_clip, host

NEW = {
    "FlowInter": "clip:vnode;super:vnode;mvbw:vnode;mvfw:vnode;time:float:opt;ml:float:opt;blend:int:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;",  # MVFlowInter.c:700-710
    "FlowFPS": "clip:vnode;super:vnode;mvbw:vnode;mvfw:vnode;num:int:opt;den:int:opt;mask:int:opt;ml:float:opt;blend:int:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;",  # MVFlowFPS.c:913-925
    "Flow": "clip:vnode;super:vnode;vectors:vnode;time:float:opt;mode:int:opt;fields:int:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;tff:int:opt;",  # MVFlow.cpp:597-607
    "FlowBlur": "clip:vnode;super:vnode;mvbw:vnode;mvfw:vnode;blur:float:opt;prec:int:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;",  # MVFlowBlur.c:555-565
    "Mask": "clip:vnode;vectors:vnode;ml:float:opt;gamma:float:opt;kind:int:opt;time:float:opt;ysc:int:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;",  # MVMask.c:350-360
}
B84 = dict(blksize=8, overlap=4)
SC = dict(thscd1=20, thscd2=10)  # every analysed frame counts as a scene change


@pytest.fixture
def flow_on(monkeypatch):
    monkeypatch.setenv("MVX_VS_FLOW", "1")  # (proc_env() copies os.environ)


@pytest.fixture
def double(monkeypatch, fakedev):
    """the CPU tests' mini-host processes run over the test double of the device layer: mv.Super and mv.Analyse answer frame 0"""
    monkeypatch.setattr(shim, "_PRELOAD", fakedev)


def _listed():
    out = host("list").splitlines()
    assert out[0] == "id=com.nodame.mvtools ns=mv"
    return dict(line.split(" ", 1) for line in out[1:])


# ---------------------------------------------------------------------------------------------------- CPU

def test_switch_registers_exactly_the_five_filters(flow_on):
    assert _listed() == dict(shim.EXPECTED, **NEW)


def test_without_the_switch_the_interface_is_unchanged(monkeypatch):
    monkeypatch.delenv("MVX_VS_FLOW", raising=False)
    assert _listed() == shim.EXPECTED
    monkeypatch.setenv("MVX_VS_FLOW", "0")
    assert _listed() == shim.EXPECTED


@pytest.mark.parametrize("args,msg", [
    (("FlowInter", 128, 96, 8, "f.time=101.0"), "FlowInter: time must be between 0 and 100 % (inclusive)."),
    (("FlowFPS", 128, 96, 8, "f.mask=3"), "FlowFPS: mask must be 0, 1, or 2."),
    (("FlowBlur", 128, 96, 8, "f.prec=0"), "FlowBlur: prec must be at least 1."),
    (("Mask", 128, 96, 8, "f.kind=6"), "Mask: kind must 0, 1, 2, 3, 4, or 5."),
    (("Flow", 128, 96, 8, "f.mode=2"), "Flow: mode must be 0 or 1."),
    (("FlowInter", 16, 16, 8, "a.blksize=16"), "FlowInter: the frame must be at least two blocks wide and two blocks high."),
    (("FlowFPS", 16, 16, 8, "a.blksize=16"), "FlowFPS: the frame must be at least two blocks wide and two blocks high."),
    (("Flow", 16, 16, 8, "a.blksize=16"), "Flow: the frame must be at least two blocks wide and two blocks high."),
    (("FlowBlur", 16, 16, 8, "a.blksize=16"), "FlowBlur: the frame must be at least two blocks wide and two blocks high."),
    (("Mask", 16, 16, 8, "a.blksize=16"), "Mask: the frame must be at least two blocks wide and two blocks high."),
    # the reference's clip check (MVMask.c:321-322): mv.Mask takes 8-bit clips only
    (("Mask", 128, 96, 16, "f.kind=5"), "Mask: input clip must be GRAY8, YUV420P8, YUV422P8, YUV440P8, or YUV444P8, with constant dimensions."),
    (("Mask", 128, 96, 8, "f.nosuch=1"), "Mask: Function does not take argument(s) named nosuch"),
])
def test_creation_errors(flow_on, double, args, msg):
    assert host("error", *args).strip() == "ERROR " + msg


@pytest.mark.parametrize("mismatch", shim.CLIP_MISMATCHES)
@pytest.mark.parametrize("filt", ["FlowInter", "FlowFPS", "Flow", "FlowBlur"])
def test_clip_must_be_the_one_the_super_clip_was_made_from(flow_on, double, filt, mismatch):
    assert host("error", filt, 128, 96, 8, mismatch).strip() == "ERROR %s: wrong source or super clip frame size." % filt


def test_without_the_switch_the_filters_do_not_exist(monkeypatch, double):
    monkeypatch.delenv("MVX_VS_FLOW", raising=False)
    assert host("error", "FlowFPS", 128, 96, 8).strip() == "ERROR no function FlowFPS"


def test_output_clip_info(flow_on, double, oracle):
    osup = oracle.Super(128, 96, 8)
    ad = oracle.Analyse(osup, num_frames=4, isb=1, delta=1).ad
    ref = flow_ref.Flow(ad, ad, 4, 3, osup.s.hpad, osup.s.vpad, fps=(24, 1), num=60, den=1)   # the mini host's blank clip: 4 frames at 24/1
    assert ref.num_frames == 8
    assert host("error", "FlowFPS", 128, 96, 8, "f.num=60", "f.den=1").strip() == "OK 128x96 frames=%d" % ref.num_frames
    assert host("error", "FlowFPS", 128, 96, 8, "f.num=0", "f.den=0").strip() == "OK 128x96 frames=7"   # double the input rate
    for f in ("FlowInter", "Flow", "FlowBlur", "Mask"):
        assert host("error", f, 128, 96, 8).strip() == "OK 128x96 frames=4", f
    assert host("error", "Mask", 128, 96, 8, "x.format=gray").strip() == "OK 128x96 frames=4"   # three 8-bit planes from a Gray clip (MVMask.c:328-329)
    assert host("error", "Flow", 128, 96, 8, "s.pel=1", "f.fields=1").strip() == "OK 128x96 frames=4"   # accepted by the reference too (MVFlow.cpp:265)
    assert host("error", "FlowInter", 128, 96, 16, "x.format=422").strip() == "OK 128x96 frames=4"


# ---------------------------------------------------------------------------------------------------- GPU: graphs against the restatements

gpu = pytest.mark.gpu


class Graph:
    """a synthetic clip on disk and what the CPU oracle makes of it: super frames, Finest frames, the delta-`delta` vector pair"""

    def __init__(self, oracle, tmp_path, w, h, bits, nf, fmt="420", seed=51, sargs=None, aargs=None, delta=1):
        self.w, self.h, self.bits, self.nf, self.fmt, self.delta = w, h, bits, nf, fmt, delta
        self.sargs, self.aargs = dict(sargs or {}), dict(B84 if aargs is None else aargs)
        self.frames = pl.moving_clip(w, h, bits, nf, seed=seed, noise=3) if fmt == "420" else _fmt_clip(w, h, bits, nf, fmt, seed)
        self.dir = tmp_path
        self.src = tmp_path / "in.raw"
        _write_clip(self.src, self.frames)
        kw = dict(shim.FORMATS, **{"420": {}, "gray": dict(gray=True, subsampling=(0, 0))})[fmt]   # (a Gray clip has no subsampling: chroma ratios 1 / 1, as in the mini host)
        self.osup = oracle.Super(w, h, bits, **dict(kw, **self.sargs))
        self.nplanes = self.osup.nplanes
        self.hpad, self.vpad, self.pel = self.osup.s.hpad, self.osup.s.vpad, self.osup.s.pel
        self.osf = [self.osup.frame(f) for f in self.frames]
        self._finest = {}
        self.abw = oracle.Analyse(self.osup, num_frames=nf, isb=1, delta=delta, **self.aargs)
        self.afw = oracle.Analyse(self.osup, num_frames=nf, isb=0, delta=delta, **self.aargs)
        inside = lambda k: self.osf[k] if 0 <= k < nf else None
        self.bbw = [self.abw.frame(self.osf[n], inside(n + delta)) for n in range(nf)]
        self.bfw = [self.afw.frame(self.osf[n], inside(n - delta)) for n in range(nf)]

    def finest(self, k):
        if k not in self._finest:
            self._finest[k] = self.osup.finest(self.osf[k])
        return self._finest[k]

    def cli(self, fargs, *extra):
        out = ["s.%s=%s" % kv for kv in self.sargs.items()] + ["a.%s=%s" % kv for kv in self.aargs.items()] + ["f.%s=%s" % kv for kv in fargs.items()]
        if self.fmt != "420":
            out.append("x.format=" + self.fmt)
        if self.delta != 1:
            out.append("x.delta=%d" % self.delta)
        return out + list(extra)

    def run(self, pipeline, fargs, *extra, name="out.raw", env=None, check=True):
        """one mini-host process; returns (CompletedProcess, path of the result file)"""
        path = self.dir / name
        cmd = [HOST, PLUGIN] + [str(a) for a in ("run", pipeline, self.src, self.w, self.h, self.bits, self.nf, path)] + self.cli(fargs, *extra)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=shim.proc_env(**(env or {})))
        if check:
            assert r.returncode == 0 and "DONE" in r.stdout, r.stdout + r.stderr
        return r, path

    def read(self, path, n, bits=None, fmt=None):
        fmt = self.fmt if fmt is None else fmt
        bits = self.bits if bits is None else bits
        return _read_frames(path, self.w, self.h, bits, n) if fmt == "420" else _read_fmt_frames(path, self.w, self.h, bits, n, fmt)


def _same(got, want, what):
    assert len(got) == len(want), what
    for n, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (what, n)
        for p in range(len(w)):
            assert g[p].shape == w[p].shape, (what, n, p, g[p].shape, w[p].shape)
            assert np.array_equal(g[p], w[p]), "%s frame %d plane %d: %s" % (what, n, p, pl.first_diff(g[p], w[p]))


def _fkw(fargs):
    """filter arguments as the restatements take them: float arguments travel as text ("33.3") on the mini host's command line"""
    return {k: (float(v) if isinstance(v, str) else v) for k, v in fargs.items()}


def _flow_expected(g, fargs, fps):
    kw = _fkw(fargs)
    ref = flow_ref.Flow(g.abw.ad, g.afw.ad, g.nf, g.nplanes, g.hpad, g.vpad, fps=(24, 1) if fps else None, **kw)
    want, kinds = [], set()
    for n in range(ref.num_frames):
        want.append(ref.frame(n, g.frames, g.finest, g.bbw, g.bfw))
        kinds.add(ref.last_kind)
    return ref, want, ",".join(sorted(kinds))


FLOWFPS_CASES = [
    # w, h, bits, fmt, filter arguments, the paths the output frames take in the restatement
    (128, 96, 8, "420", dict(num=60, mask=2), "copy,extra,simple"),
    (128, 96, 16, "420", dict(num=48, mask=1), "copy,regular128"),
    (128, 96, 8, "420", dict(num=60, mask=0), "copy,simple"),
    (128, 96, 8, "420", dict(num=60, mask=2, **SC), "blend,copy"),
    (128, 96, 8, "420", dict(num=60, mask=2, blend=0, **SC), "copy,left"),
    (206, 118, 8, "420", dict(num=60, mask=2), "copy,extra,simple"),   # nBlkXP > nBlkX and nBlkYP > nBlkY
    (128, 96, 16, "444", dict(num=60, mask=2), "copy,extra,simple"),
    (128, 96, 8, "gray", dict(num=60, mask=2, ml="40.0"), "copy,extra,simple"),
]


@gpu
@pytest.mark.parametrize("w,h,bits,fmt,fargs,kinds", FLOWFPS_CASES)
def test_flowfps_graph_matches_restatement(flow_on, oracle, tmp_path, w, h, bits, fmt, fargs, kinds):
    g = Graph(oracle, tmp_path, w, h, bits, 5, fmt, seed=61)
    ref, want, seen = _flow_expected(g, fargs, fps=True)
    assert seen == kinds
    r, path = g.run("flowfps", fargs)
    lines = r.stdout.splitlines()
    assert lines[0] == "flowfps frames=%d fps=%d/%d" % ((ref.num_frames,) + ref.fps)
    assert lines[1] == "frame1 _DurationNum=%d _DurationDen=%d" % (ref.fps[1], ref.fps[0])   # std.AssumeFPS ran (MVFlowFPS.c:881-900)
    _same(g.read(path, ref.num_frames), want, "FlowFPS")


FLOWINTER_CASES = [
    # bits, fmt, delta, filter arguments, paths.  The last `delta` frames have nright past the end: Blend
    (8, "420", 1, dict(time="50.0"), "blend,extra128,regular128"),
    (16, "420", 1, dict(time="33.0", ml="33.3"), "blend,extra,regular"),
    (8, "420", 1, dict(time="0.0"), "blend,extra,regular"),     # no copy shortcut at time 0
    (8, "420", 2, dict(time="50.0"), "blend,extra128,regular128"),
    (8, "422", 1, dict(time="50.0"), "blend,extra128,regular128"),
]


@gpu
@pytest.mark.parametrize("bits,fmt,delta,fargs,kinds", FLOWINTER_CASES)
def test_flowinter_graph_matches_restatement(flow_on, oracle, tmp_path, bits, fmt, delta, fargs, kinds):
    g = Graph(oracle, tmp_path, 128, 96, bits, 5 + delta, fmt, seed=63, delta=delta)   # (delta 2: frame 2 alone has all four vector frames usable)
    ref, want, seen = _flow_expected(g, fargs, fps=False)
    assert seen == kinds
    assert [ref.map(n)[1] >= g.nf for n in range(g.nf)] == [False] * 5 + [True] * delta
    _, path = g.run("flowinter", fargs)
    _same(g.read(path, g.nf), want, "FlowInter")


def _flowcomp_expected(g, fargs, fw, shift_of=None):
    kw = _fkw(fargs)
    for k in ("fields", "tff"):
        kw.pop(k, None)
    an, blobs = (g.afw, g.bfw) if fw else (g.abw, g.bbw)
    ref = flowmc_ref.Flow(an.ad, g.nf, g.nplanes, g.hpad, g.vpad, g.bits, **kw)
    want, kinds, stats, shifts = [], set(), {}, set()
    for n in range(g.nf):
        fs = shift_of(n, ref.ref(n)) if shift_of and 0 <= ref.ref(n) < g.nf else 0
        want.append(ref.frame(n, g.frames, g.finest, blobs[n], fs, stats))
        kinds.add(ref.last_kind)
        if ref.last_kind != "copy":
            shifts.add(fs)
    return want, ",".join(sorted(kinds | {k for k, v in stats.items() if v > 0})), shifts


SH = "collide,copy,hole,shift"
FLOW_CASES = [
    # bits, super arguments, forward vectors, filter arguments, paths
    (8, {}, False, dict(time="100.0"), "copy,fetch"),
    (8, {}, False, dict(time="100.0", mode=1), SH),
    (8, {}, True, dict(time="37.5"), "copy,fetch"),
    (8, {}, True, dict(time="37.5", mode=1), SH),
    (8, dict(pel=1), False, dict(time="100.0", mode=1), SH),
    (8, dict(pel=4), True, dict(time="100.0"), "copy,fetch"),
    (16, {}, False, dict(time="100.0"), "copy,fetch"),
    (16, {}, True, dict(time="100.0", mode=1), SH),
    (8, {}, False, dict(time="100.0", **SC), "copy"),   # scene change: the clip frame
]


@gpu
@pytest.mark.parametrize("bits,sargs,fw,fargs,kinds", FLOW_CASES)
def test_flow_graph_matches_restatement(flow_on, oracle, tmp_path, bits, sargs, fw, fargs, kinds):
    g = Graph(oracle, tmp_path, 128, 96, bits, 5, seed=65, sargs=sargs)
    want, seen, _ = _flowcomp_expected(g, fargs, fw)
    assert seen == kinds
    _, path = g.run("flow", fargs, *(["x.vectors=fw"] if fw else []))
    _same(g.read(path, g.nf), want, "Flow")


@gpu
@pytest.mark.parametrize("how,fw", [("props1", False), ("tff1", True)])
def test_flow_fields_shift_by_parity(flow_on, oracle, tmp_path, how, fw):
    """fields=1: the parities of frames n and nref -- from the frames' _Field props, or from tff, which overrides -- give the vertical shift of
    MVFlow.cpp:264-302"""
    g = Graph(oracle, tmp_path, 128, 96, 8, 5, seed=67)
    assert g.pel == 2
    order = int(how[-1])
    if how.startswith("tff"):
        shift_of = lambda n, nref: oracle.field_shift(1, g.pel, n, nref, tff=order)[0]
        fargs, extra = dict(fields=1, tff=order), []
    else:
        shift_of = lambda n, nref: oracle.field_shift(1, g.pel, n, nref, src_field=order ^ (n % 2), ref_field=order ^ (nref % 2))[0]
        fargs, extra = dict(fields=1), ["x.fieldorder=%d" % order]
    want, seen, shifts = _flowcomp_expected(g, {}, fw, shift_of)
    assert seen == "copy,fetch" and shifts == {1, -1}
    plain, _, _ = _flowcomp_expected(g, {}, fw)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(want, plain)), "the shift changes nothing: the case cannot tell"
    _, path = g.run("flow", fargs, *(extra + (["x.vectors=fw"] if fw else [])))
    _same(g.read(path, g.nf), want, "Flow fields")


@gpu
def test_flow_fields_need_parity_information(flow_on, oracle, tmp_path):
    g = Graph(oracle, tmp_path, 128, 96, 8, 3, seed=67)
    r, _ = g.run("flow", dict(fields=1), check=False)
    assert "ERROR output frame: Flow: _Field property not found in super frame. Therefore, you must pass tff argument." in r.stdout
    r, _ = g.run("flow", dict(fields=1, tff=0))
    assert "DONE" in r.stdout


def _blur_expected(g, fargs):
    ref = flowmc_ref.FlowBlur(g.abw.ad, g.afw.ad, g.nf, g.nplanes, g.hpad, g.vpad, g.bits, **_fkw(fargs))
    want, kinds, stats = [], [], {}
    for n in range(g.nf):
        want.append(ref.frame(n, g.frames, g.finest, g.bbw, g.bfw, stats))
        kinds.append(ref.last_kind)
    return want, kinds, ",".join(sorted(k for k, v in stats.items() if v > 0))


FLOWBLUR_CASES = [
    # bits, super arguments, delta, filter arguments, the restatement's counters
    (8, {}, 1, {}, "notaps,taps"),
    (8, {}, 1, dict(blur="200.0", prec=2), "taps,trunc"),
    (16, dict(pel=1), 1, dict(blur="200.0"), "taps,trunc"),
    (8, {}, 2, dict(blur="150.0"), "taps,trunc"),
]


@gpu
@pytest.mark.parametrize("bits,sargs,delta,fargs,counters", FLOWBLUR_CASES)
def test_flowblur_graph_matches_restatement(flow_on, oracle, tmp_path, bits, sargs, delta, fargs, counters):
    g = Graph(oracle, tmp_path, 128, 96, bits, 6, seed=69, sargs=sargs, delta=delta)
    want, kinds, seen = _blur_expected(g, fargs)
    assert kinds == ["copy"] * delta + ["blur"] * (g.nf - 2 * delta) + ["copy"] * delta   # mvbw at n - delta or mvfw at n + delta outside the clip
    assert seen == counters
    _, path = g.run("flowblur", fargs)
    _same(g.read(path, g.nf), want, "FlowBlur")


def _mask_expected(g, fargs, fw):
    an, blobs = (g.afw, g.bfw) if fw else (g.abw, g.bbw)
    ref = mask_ref.Mask(an.ad, **_fkw(fargs))
    stats = {}
    want = [ref.frame(blobs[n], g.frames[n][0], stats) for n in range(g.nf)]
    assert ref.pow_dist == math.inf, "the case takes a pow: not exact by construction"
    return want, ",".join(sorted(k for k, v in stats.items() if v > 0))


MASK_CASES = [
    # w, h, fmt, forward vectors, filter arguments, the restatement's counters ("sc": the frame at the clip's end has no reference)
    (128, 96, "420", False, dict(kind=0, gamma="2.0"), "sc"),
    (206, 118, "420", True, dict(kind=0, gamma="2.0", ml="3.0"), "cut,edgex,edgey,sc"),
    (128, 96, "420", False, dict(kind=1, gamma="1.0"), "sc"),
    (128, 96, "420", True, dict(kind=2, gamma="1.0"), "sc"),
    (128, 96, "420", False, dict(kind=2, time="50.0", ml="3.0"), "cut,sc"),
    (128, 96, "420", False, dict(kind=3), "sc"),
    (206, 118, "420", True, dict(kind=4, ml="3.0"), "edgex,edgey,sc"),
    (206, 118, "420", False, dict(kind=5), "edgex,edgey,sc"),
    (128, 96, "420", False, dict(kind=0, gamma="2.0", ysc=77, **SC), "sc"),   # every frame filled with ysc
    (128, 96, "420", True, dict(kind=5, ysc=77, **SC), "sc"),                  # kind 5 keeps the clip's luma
    (128, 96, "gray", False, dict(kind=5, ml="10.0"), "sc"),                   # a Gray clip: three full-size planes
    (128, 96, "gray", True, dict(kind=1), "sc"),
    (128, 96, "422", False, dict(kind=2), "sc"),
    (128, 96, "422", True, dict(kind=5, ml="3.0"), "cut,sc"),
]


@gpu
@pytest.mark.parametrize("w,h,fmt,fw,fargs,counters", MASK_CASES)
def test_mask_graph_matches_restatement(flow_on, oracle, tmp_path, w, h, fmt, fw, fargs, counters):
    g = Graph(oracle, tmp_path, w, h, 8, 4, fmt, seed=71)
    want, seen = _mask_expected(g, fargs, fw)
    assert seen == counters
    if "thscd1" in fargs:
        assert all(np.all(fr[1] == fargs["ysc"]) for fr in want)
    _, path = g.run("mask", fargs, *(["x.vectors=fw"] if fw else []))
    _same(g.read(path, g.nf, fmt="444" if fmt == "gray" else fmt), want, "Mask")


@gpu
def test_mask_takes_8_bit_clips_only(flow_on, oracle, tmp_path):
    """the reference refuses clips of more than 8 bits (MVMask.c:321-322), and so does the library: there is no 16-bit luma for kind 5 to keep"""
    g = Graph(oracle, tmp_path, 128, 96, 16, 3, seed=71)
    r, _ = g.run("mask", dict(kind=5), check=False)
    assert "ERROR mask: Mask: input clip must be GRAY8, YUV420P8, YUV422P8, YUV440P8, or YUV444P8, with constant dimensions." in r.stdout


# ---------------------------------------------------------------------------------------------------- GPU: threads, the admission gate, lazy super frames

THREADED = [("flowfps", dict(num=60, mask=2)), ("flowinter", dict(time="33.0")), ("flow", dict(mode=1)), ("flowblur", dict(blur="120.0")), ("mask", dict(kind=5))]


@gpu
@pytest.mark.parametrize("pipeline,fargs", THREADED, ids=[t[0] for t in THREADED])
def test_concurrent_requests_through_the_gate_are_bit_identical(flow_on, oracle, tmp_path, pipeline, fargs):
    """fmParallel: eight worker threads ask for output frames only, the admission gate lets three requests in at a time; the clip is the one the
    frame-by-frame evaluation gives (which the cases above tie to the restatements), the graph tears down with every permit returned"""
    g = Graph(oracle, tmp_path, 128, 96, 8, 12, seed=73)
    _, seq = g.run(pipeline, fargs, name="seq.raw")
    r, par = g.run(pipeline, fargs, "x.threads=8", "x.order=frame", "x.free=1", name="par.raw", env=dict(MVX_VS_MAX_INFLIGHT="3"))
    assert "FREED" in r.stdout and "DONE" in r.stdout
    assert "permits out" not in r.stderr, r.stderr
    assert open(seq, "rb").read() == open(par, "rb").read()


@gpu
@pytest.mark.parametrize("pipeline,fargs,env", [("flowfps", dict(num=60, mask=2), {}),
                                                ("flow", dict(time="100.0"), {"MVX_VS_LOOKAHEAD": "0", "MVX_VS_CACHE_FRAMES": "3"})])   # per-frame path, a cache so small that the consumer rebuilds super frames from the embedded source
def test_lazy_super_frames_are_bit_identical(flow_on, oracle, tmp_path, pipeline, fargs, env):
    """MVX_VS_SUPER_LAZY=1: the super frames the filters are handed carry the source picture only; super_to_device finds the device copy or rebuilds it"""
    g = Graph(oracle, tmp_path, 128, 96, 16, 8, seed=75)
    _, ref = g.run(pipeline, fargs, name="ref.raw", env=env)
    _, lazy = g.run(pipeline, fargs, "x.threads=4", "x.order=frame", name="lazy.raw", env=dict(env, MVX_VS_SUPER_LAZY="1"))
    assert os.path.getsize(ref) > 0
    assert open(ref, "rb").read() == open(lazy, "rb").read()
