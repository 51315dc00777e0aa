"""The cases of tests/test_vs_float_shell.py and what the numpy restatements expect of them (test infrastructure): 32-bit float clips through
the VapourSynth filter shell with MVX_VS_FLOAT=1.

Every case takes its clip and its parameters from the float family's own case modules (degrain_float_cases, compensate_float_cases,
blockfps_float_cases, flow_float_cases, flowmc_float_cases), so that their CPU proofs apply: the integer clip is the suite's moving texture, the
float clip is degrain_float_cases.float_clip of it -- its quantised copy IS the integer clip -- and the vectors are the CPU oracle's search of
the integer clip.  The expected planes come from the restatements alone (super_float_ref, degrain_float_ref, compensate_float_ref,
blockfps_float_ref, flow_float_ref, flowmc_float_ref, depan_float_ref) fed the Super restatement's frames and the oracle's blobs: nothing here
touches the library, the Python package or the shell.  The few cases with parameters of their own have CPU tests in
tests/test_vs_float_shell.py that show, through the oracle, that they test what they claim."""
import collections
import subprocess

import numpy as np

import blockfps_float_cases as bc
import compensate_float_cases as cc
import degrain_float_cases as fc
import degrain_n_cases as dc
import flow_float_cases as flc
import flowmc_float_cases as fmc
import multi_cases as mc
import pipeline as pl
import super_float_ref as sf
import test_vs_shim as shim

F = np.float32
SUB = {"420": (1, 1), "422": (1, 0), "444": (0, 0), "gray": (0, 0)}   # (the mini host's Gray clip has no subsampling)
# what oracle.Super takes for a format: the mini host's Gray clip states chroma ratios of 1 / 1 in its analysis data
FORMATS = dict(dc.FORMATS, gray=dict(gray=True, subsampling=(0, 0)))
Info = collections.namedtuple("Info", "hpad vpad pel sharp")   # what the restatements read of a float super clip's mvx_super_info


def info_of(skw):
    return Info(skw.get("hpad", 16), skw.get("vpad", 16), skw.get("pel", 2), skw.get("sharp", 2))


def super_kw(fmt, skw):
    """super_float_ref.frame's keyword arguments for a format and mv.Super's arguments"""
    i = info_of(skw)
    return dict(sub=SUB[fmt] if fmt != "gray" else (1, 1), gray=fmt == "gray", hpad=i.hpad, vpad=i.vpad, pel=i.pel, sharp=i.sharp)


def float_supers(floats, fmt, skw):
    """k -> the float super frame of clip frame k (level 0, planes of the super clip's shapes), computed once"""
    cache = {}

    def sup(k):
        if k not in cache:
            cache[k] = sf.frame(floats[k], **super_kw(fmt, skw))[0]
        return cache[k]
    return sup


def shapes(w, h, fmt):
    if fmt == "gray":
        return [(h, w)]
    sx, sy = SUB[fmt]
    return [(h, w)] + [(h >> sy, w >> sx)] * 2


def read_float(path, plane_shapes, n):
    """n frames of float32 planes, tightly packed, as uint32 views are compared"""
    data = np.fromfile(path, dtype=F)
    per = sum(a * b for a, b in plane_shapes)
    assert data.size == per * n, (data.size, per, n)
    out, off = [], 0
    for _ in range(n):
        fr = []
        for a, b in plane_shapes:
            fr.append(data[off:off + a * b].reshape(a, b))
            off += a * b
        out.append(fr)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same(got, want, what):
    """bit for bit, as uint32 per plane; want[n] None: not compared"""
    assert len(got) == len(want), (what, len(got), len(want))
    for n, (g, w) in enumerate(zip(got, want)):
        if w is None:
            continue
        assert len(g) == len(w), (what, n)
        for p in range(len(w)):
            assert g[p].shape == w[p].shape and w[p].dtype == F, (what, n, p, g[p].shape, w[p].shape, w[p].dtype)
            assert np.array_equal(bits(g[p]), bits(w[p])), "%s frame %d plane %d: %s" % (what, n, p, pl.first_diff(g[p], w[p]))


class Graph:
    """an integer clip and its float clip on disk, and mini-host runs over them with the float switch on"""

    def __init__(self, tmp_path, q, floats, w, h, bits_, fmt):
        self.dir, self.q, self.floats, self.w, self.h, self.bits, self.fmt, self.n = tmp_path, q, floats, w, h, bits_, fmt, len(q)
        self.src, self.fsrc = tmp_path / "in.raw", tmp_path / "in_float.raw"
        shim._write_clip(self.src, q)
        shim._write_clip(self.fsrc, floats)
        assert all(p.dtype == F for fr in floats for p in fr)

    def run(self, pipeline, *cli, name="out.raw", env=None, check=True, use_float=True):
        """one mini-host process under a time limit of its own -> (CompletedProcess, path of the result file)"""
        path = self.dir / name
        cmd = [shim.HOST, shim.PLUGIN] + [str(a) for a in ("run", pipeline, self.src, self.w, self.h, self.bits, self.n, path)] + [str(a) for a in cli]
        if use_float:
            cmd.append("x.float=%s" % self.fsrc)
        if self.fmt != "420":
            cmd.append("x.format=" + self.fmt)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=shim.proc_env(**dict(ENV, **(env or {}))))
        if check:
            assert r.returncode == 0 and "DONE" in r.stdout, r.stdout + r.stderr
            if use_float:
                assert "output format sample=float bits=32 bytes=4" in r.stdout, r.stdout
        return r, path

    def read(self, path, n=None):
        return read_float(path, shapes(self.w, self.h, self.fmt), self.n if n is None else n)


ENV = {"MVX_VS_FLOAT": "1", "MVX_VS_FLOW": "1", "MVX_VS_DEPAN": "1", "MVX_VS_MULTI": "1"}


def cli(prefix, kw):
    return ["%s.%s=%s" % (prefix, k, v) for k, v in kw.items()]


# ------------------------------------------------------------------------------------------------ Super
# (size, fmt, pel, sharp, (hpad, vpad)): pel 1 / 2 / 4, sharp 0 / 2; the clips are tests/test_gpu_super_float.py's
SUPER_CASES = [((70, 54), "420", 2, 2, (16, 16)), ((140, 38), "422", 4, 0, (8, 4)), ((36, 36), "gray", 1, 2, (0, 0))]


def super_clip(size, fmt):
    w, h = size
    sub = (1, 1) if fmt == "gray" else SUB[fmt]
    q = pl.moving_clip(w, h, 16, 3, seed=5, noise=3, sub=sub)
    if fmt == "gray":
        q = [[f[0]] for f in q]
    return q, fc.float_clip(q, 16, seed=2)


def super_shapes(size, fmt, pel, pad):
    return sf.geometry(size[0], size[1], (1, 1) if fmt == "gray" else SUB[fmt], fmt == "gray", pad[0], pad[1], pel)[1]


# ------------------------------------------------------------------------------------------------ DegrainN
B168, B84 = dict(blksize=16, overlap=8), dict(blksize=8, overlap=4)
PAD0 = dict(hpad=0, vpad=0)
A, B, C = (70, 54), (140, 38), (36, 36)
# name -> (size, fmt, bits of the searched copy, super kwargs, analyse kwargs, radius, DegrainN kwargs).  All but the last two are cases of
# tests/test_gpu_degrain_float.py (clip: degrain_n_cases.clip with its noise, float_clip seed 9); plane0-limit2 joins two of its cases'
# arguments and scene is its clip with a cut after frame 3: tests/test_vs_float_shell.py shows on the CPU what they must show
DEGRAIN_CASES = {
    "A-r1-16/8": (A, "420", 16, {}, B168, 1, {}),
    "A-r3-8/4": (A, "420", 16, {}, B84, 3, {}),
    "A-r7-8/4-falloff": (A, "420", 16, {}, B84, 7, dict(thsad=1600, thsad2=400)),
    "B-r3-8/4": (B, "420", 16, {}, B84, 3, {}),
    "C-gray-pad0-r3-8/4": (C, "gray", 16, PAD0, B84, 3, {}),
    "A-444-r3-8/4": (A, "444", 16, {}, B84, 3, {}),
    "A-r3-16/8-plane0-limit2": (A, "420", 16, {}, B168, 3, dict(plane=0, limit=2)),
    "A-r3-8/4-scene": (A, "420", 16, {}, B84, 3, {}),
}
CUT = 4   # the scene case: frames 0..3 of the texture, 4..6 its negative (moving_clip draws ONE texture whatever its seed)


def degrain_clip(name):
    (w, h), fmt, bits_, skw, akw, radius, dkw = DEGRAIN_CASES[name]
    n = 2 * radius + 1
    q = dc.clip(w, h, bits_, n, fmt, noise=3)
    if name.endswith("scene"):
        q = q[:CUT] + [[((1 << bits_) - 1 - p).astype(p.dtype) for p in fr] for fr in q[CUT:]]
    return q, fc.float_clip(q, bits_, seed=9)


def degrain_expected(oracle, name, q, floats, targets):
    """-> ({n: planes}, {n: the restatement after frame n}) for the output frames `targets`"""
    (w, h), fmt, bits_, skw, akw, radius, dkw = DEGRAIN_CASES[name]
    sup = float_supers(floats, fmt, skw)
    want, refs = {}, {}
    for t in targets:
        f = FORMATS[fmt]
        _, _, ad, nrefs, blobs = fc.oracle_job(oracle, q, w, h, bits_, radius, t, akw, skw, sub=f.get("subsampling", (1, 1)), gray=fmt == "gray")
        ref = fc.restatement(oracle, radius, ad, *dc.tables(ad, radius, dkw), dkw, gray=fmt == "gray")
        want[t] = ref.frame(floats[t], [sup(m) if m is not None else None for m in nrefs], blobs)
        refs[t] = ref
    return want, refs


# ------------------------------------------------------------------------------------------------ Compensate / CompensateN
# compensate_float_cases.SEARCHED's 70x54 cases at tr 2 (thsad 300; tests/test_compensate_float_cases.py shows the shares at distance 2) and its 4:4:4 one:
# CompensateN at tr 2, mv.Compensate on the backward vectors of delta 2 with and without overlap
COMP_N_CASE = ("420", 16, mc.B84, 2, 70, 54, 300)
COMP_CASES = {"overlap": ("420", 16, mc.B84, 2, 70, 54, 300), "side-by-side": ("420", 16, mc.B160, 2, 70, 54, 300), "444": ("444", 8, mc.B84, 3, mc.W, mc.H, mc.THSAD)}
assert COMP_N_CASE in cc.SEARCHED and all(c in cc.SEARCHED for c in COMP_CASES.values())


def comp_clip(case):
    fmt, bits_, blk, tr, w, h, thsad = case
    q = dc.clip(w, h, bits_, mc.nframes(tr), fmt)
    return q, fc.float_clip(q, bits_, seed=9)


def _searches(oracle, q, w, h, bits_, fmt, skw, akw, fields):
    """fields: [(isb, delta)] -> per field (analysis data, [blob of every frame, searched against n +- delta or nothing outside the clip])"""
    osup = oracle.Super(w, h, bits_, **dict(FORMATS[fmt], **skw))
    osf = [osup.frame(f) for f in q]
    n, out = len(q), []
    for isb, d in fields:
        an = oracle.Analyse(osup, num_frames=n, isb=isb, delta=d, **akw)
        ref = lambda m: m + d if isb else m - d
        out.append((an.ad, [an.frame(osf[m], osf[ref(m)] if 0 <= ref(m) < n else None) for m in range(n)]))
    return out


def compensate_expected(oracle, case, q, floats, delta):
    """mv.Compensate on the backward vectors of `delta`: every frame"""
    fmt, bits_, blk, tr, w, h, thsad = case
    (ad, blobs), = _searches(oracle, q, w, h, bits_, fmt, blk[1], blk[2], [(1, delta)])
    sup = float_supers(floats, fmt, blk[1])
    ref = cc.restatement(oracle, ad, dict(thsad=thsad), gray=fmt == "gray")
    out, used = [], []
    for n in range(len(q)):
        out.append(ref.field(sup(n), sup(n + delta) if n + delta < len(q) else None, blobs[n]))
        if ref.from_ref is not None:
            used.append(float(ref.from_ref.mean()))
    return out, used


def compensate_n_expected(oracle, case, q, floats):
    """[n * (2 tr + 1) + k] -> planes"""
    fmt, bits_, blk, tr, w, h, thsad = case
    found = _searches(oracle, q, w, h, bits_, fmt, blk[1], blk[2], [mc.field_of(r) for r in range(2 * tr)])
    sup = float_supers(floats, fmt, blk[1])
    ref = cc.restatement(oracle, found[0][0], dict(thsad=thsad), gray=fmt == "gray")
    out = []
    for n in range(len(q)):
        refs = []
        for r in range(2 * tr):
            isb, d = mc.field_of(r)
            m = n + d if isb else n - d
            refs.append(sup(m) if 0 <= m < len(q) else None)
        out += ref.job(tr, sup(n), refs, [found[r][1][n] for r in range(2 * tr)])
    return out


# ------------------------------------------------------------------------------------------------ BlockFPS
# blockfps_float_cases.SEARCHED's masked 70x54 case (mode 7, ml 20: tests/test_blockfps_float_cases.py shows the masks) and its 4:2:2 one; mode 0 reads no
# mask and runs on the same geometry with blocks side by side
FPS_CASES = {"70x54-mode7": ("420", 16, bc.B84, 70, 54, 7, 20.0), "422-mode6": ("422", 16, bc.B160, 96, 64, 6, 20.0), "70x54-mode0": ("420", 16, bc.B160, 70, 54, 0, 100.0)}
assert all(c in bc.SEARCHED for k, c in FPS_CASES.items() if k != "70x54-mode0")


def fps_clip(case):
    fmt, bits_, blk, w, h, mode, ml = case
    q = bc.int_clip(fmt, bits_, w, h)
    return q, fc.float_clip(q, bits_, seed=9)


def fps_expected(oracle, case, q, floats):
    """24 -> 60: -> (the eleven output frames, time256 of each)"""
    fmt, bits_, blk, w, h, mode, ml = case
    (adb, bw), (adf, fw) = _searches(oracle, q, w, h, bits_, fmt, blk[1], blk[2], [(1, 1), (0, 1)])
    osup = oracle.Super(w, h, bits_, **dict(FORMATS[fmt], **blk[1]))
    bkw = dict(mode=mode, ml=ml)
    ob = oracle.BlockFPS(osup, adb, adf, len(q), 24, 1, num=60, den=1, **bkw)
    ref = bc.restatement(oracle, adb, adf, bkw, gray=fmt == "gray")
    sup = float_supers(floats, fmt, blk[1])
    sups = [sup(k) for k in range(len(q))]
    return [bc.want_frame(ref, ob.map, n, floats, sups, bw, fw) for n in range(ob.num_frames)], [ob.map(n)[2] for n in range(ob.num_frames)]


# ------------------------------------------------------------------------------------------------ the Flow family: searched cases of the two modules, by name
def _named(cases, *names):
    byname = {c.name: c for c in cases}
    return [byname[n] for n in names]


FLOWINTER_CASES = _named(flc.INTER_SEARCHED, "36x36-gray-pad0-8/4-time37.5", "35x30-444-pel1-8/4-time50", "70x54-8bit-pel2-4/2-time0")
FLOWFPS_CASES = _named(flc.FPS_SEARCHED, "70x54-16bit-pel2-4/2-60-mask2", "35x30-444-pel2-8/4-48-mask2")
FLOW_CASES = _named(fmc.FLOW_SEARCHED, "70x54-8bit-pel2-4/2-fw", "70x54-16bit-pel2-4/2-bw-shift", "35x30-444-pel2-8/4-fw-shift", "36x36-gray-pad0-8/4-bw")
BLUR_CASES = _named(fmc.BLUR_SEARCHED, "420-16bit-pel2-16/8-d2-blur200", "444-8bit-pel4-16/0-blur200")


def flow_expected(oracle, c):
    """-> (integer clip, float clip, the module's Expected) for a case of flow_float_cases (kind inter / fps) or flowmc_float_cases (flow / blur)"""
    mod = flc if c.kind in ("inter", "fps") else fmc
    q, floats = mod.clips(c)
    found = mod.search_oracle(oracle, c, q)
    if c.fmt == "gray":   # (the oracle's Gray analysis data carries 4:2:0 ratios; nothing of a one-plane clip reads them)
        assert all(ad.nWidth == c.w for ad, _ in found)
    return q, floats, mod.Expected(c, floats, found, info_of(c.skw))


def flow_cli(c):
    akw = {k: v for k, v in c.akw.items() if k not in ("isb", "delta")}
    fkw = {k: v for k, v in c.fkw.items() if k != "fps"}
    out = cli("s", c.skw) + cli("a", akw) + cli("f", fkw)
    if c.akw.get("delta", 1) != 1:
        out.append("x.delta=%d" % c.akw["delta"])
    if c.kind == "flow" and not c.akw["isb"]:
        out.append("x.vectors=fw")
    return out


# ------------------------------------------------------------------------------------------------ DepanCompensate / DepanStabilise
# tests/test_vs_depan_shell.py's panning clip with a cut (8 bits: the data clip comes from mv.DepanAnalyse on it), at any chroma format and size.  128x96 4:2:0 is that
# file's own clip; its float rows (512 and 256 bytes) fill the 256-byte device pitch exactly, so the other two do not: 70x54 4:4:4 has rows of 280 bytes, 100x72 4:2:2
# rows of 400 and 200
PAN_NF, PAN_CUT, PAN = 8, 4, (4, -2)
PAN_SHAPES = {"420-128x96": ("420", 128, 96), "444-70x54": ("444", 70, 54), "422-100x72": ("422", 100, 72)}


def pan_clip(fmt, w, h):
    import depan_estimate_cases as dec
    sub, m, out = SUB[fmt], 40, []
    for n in range(PAN_NF):
        seed = 900 if n < PAN_CUT else 950
        k = n if n < PAN_CUT else n - PAN_CUT
        planes = []
        for p in range(3):
            sx, sy = (1 << sub[0], 1 << sub[1]) if p else (1, 1)
            c = dec.canvas(h // sy + 2 * m, w // sx + 2 * m, 8, seed + p, smooth=1, power=2 if p == 0 else 1)
            oy, ox = m + k * PAN[1] // sy, m + k * PAN[0] // sx
            planes.append(np.ascontiguousarray(c[oy:oy + h // sy, ox:ox + w // sx]))
        out.append(planes)
    return out


def pan_motions(oracle, frames, fmt, w, h):
    """depan_ref's estimator on the oracle's forward vectors (blocks of 8 stepping by 4) -> per frame (dx, dy, zoom, rot)"""
    import depan_ref as dr
    import vector_fields as vf
    (ad, blobs), = _searches(oracle, frames, w, h, 8, fmt, {}, B84, [(0, 1)])
    _, s1, s2 = vf.scaled_thresholds(ad, 400)
    ref = dr.Analyse(ad, w, h, s1, s2)
    found = [ref.frame(blobs[n], None, False) for n in range(len(frames))]
    assert [m["dx"] != 0 for m in found] == [n not in (0, PAN_CUT) for n in range(len(frames))]   # (no case passes on an all-zero data clip)
    return [(m["dx"], m["dy"], m["zoom"], m["rot"]) for m in found]
