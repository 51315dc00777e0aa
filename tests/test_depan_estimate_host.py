"""CPU tests of mv.DepanEstimate: creation (no device is touched) against the restatement tests/depan_estimate_ref.py with the reference's messages
in its order (MVDepan.cpp:1271-1433) and the library's refusals; the struct layouts against the C header; the host tail and stage 3
(csrc/mvx_depan_estimate_host.h) bit for bit against the restatement on the cases' scan results and on crafted ones; the text of the kernels
(csrc/mvx_depan_fft_core.h) compiled for the host and held to the same three checks as the GPU (tests/depan_estimate_checks.py); and both as
stand-alone programs under AddressSanitizer and UBSan."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import depan_estimate_cases as dc
import depan_estimate_checks as ck
import depan_estimate_ref as er

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "vapoursynth-mvtools_amd", "csrc")
f32 = np.float32
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _bits(v):
    return int(f32(v).view(np.uint32))


def _filter(mv, c, **kw):
    return mv.DepanEstimate(c.width, c.height, c.bits, **dict(c.kw, **kw))


# ------------------------------------------------------------------------------------------------ creation

GOOD = [dict(w=1920, h=1080), dict(w=3840, h=2160, bits=16), dict(w=64, h=48), dict(w=1920, h=1080, zoommax=1.5),
        dict(w=1920, h=1080, zoommax=1.5, winx=512, wleft=100, wtop=9, winy=64), dict(w=640, h=480, winx=64, winy=64, dxmax=31, dymax=31),
        dict(w=20000, h=64), dict(w=75, h=37, winx=32, winy=16, wleft=13, wtop=7, dxmax=0, dymax=0), dict(w=640, h=480, trust=0.0), dict(w=640, h=480, trust=100.0)]
BAD = [dict(trust=-0.5), dict(trust=100.5), dict(pixaspect=0.0), dict(bits=17), dict(bits=7), dict(bits=16, float_samples=True), dict(winx=1024),
       dict(winx=512, wleft=200), dict(winy=512), dict(winy=256, wtop=300), dict(winx=64, dxmax=32), dict(winy=64, dymax=32),
       dict(bits=32, float_samples=True), dict(bits=32, float_samples=True, dxmax=9999), dict(winx=100), dict(winy=48), dict(winx=4, winy=8),
       dict(winx=24, zoommax=1.2), dict(w=4, h=4), dict(w=20000, h=64, winx=16384), dict(zoommax=1.2, winx=256, wleft=200)]
_ORDER = dict(trust=101, pixaspect=-1, bits=17, winx=1024, winy=512, dxmax=9999, dymax=9999)
BAD += [dict(list(_ORDER.items())[k:]) for k in range(len(_ORDER))]


@pytest.mark.parametrize("kw", GOOD, ids=repr)
def test_creation_resolves_as_the_restatement(mv, kw):
    kw = dict(kw)
    w, h = kw.pop("w"), kw.pop("h")
    g, e = mv.DepanEstimate(w, h, **kw), er.Estimate(w, h, **kw)
    i = g.info
    assert (i.winx, i.winy, i.wleft, i.wtop, i.dxmax, i.dymax, i.windows, i.spectrum_bytes) == (e.winx, e.winy, e.wleft, e.wtop, e.dxmax, e.dymax, e.windows,
                                                                                               e.spectrum_bytes)


@pytest.mark.parametrize("kw", BAD, ids=repr)
def test_creation_fails_with_the_restatement_s_message(mv, kw):
    kw = dict(kw)
    w, h = kw.pop("w", 640), kw.pop("h", 480)
    with pytest.raises(er.CreateError) as want:
        er.Estimate(w, h, **kw)
    with pytest.raises(mv.MvtoolsError) as got:
        mv.DepanEstimate(w, h, **kw)
    assert str(got.value) == str(want.value)


def test_struct_layouts_match_the_header(mv, tmp_path):
    names = ["mvx_depan_estimate_args", "mvx_depan_estimate_info", "mvx_depan_estimate_result", "mvx_depan_estimate_scan"]
    py = [mv.DepanEstimateArgs, mv.DepanEstimateInfo, mv.DepanEstimateResult, mv.DepanEstimateScan]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mvtools_amd.h"', 'int main(void) {']
    for n, t in zip(names, py):
        lines.append('printf("%%zu", sizeof(%s));' % n)
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (n, f[0]) for f in t._fields_]
        lines.append('printf("\\n");')
    (tmp_path / "layout.c").write_text("\n".join(lines + ["return 0;", "}"]))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", exe])
    for line, t in zip(subprocess.check_output([exe]).decode().split("\n"), py):
        assert [int(v) for v in line.split()] == [C.sizeof(t)] + [getattr(t, f[0]).offset for f in t._fields_], t.__name__


def test_zero_frames_and_zero_pairs_are_no_ops_without_a_device(mv):
    g = mv.DepanEstimate(64, 48)
    assert g.spectra([]) == [] and g.correlate([], []) == [] and g.run([]) == [] and g.host_tail([]) == [] and g.finish([]) == []


# ------------------------------------------------------------------------------------------------ host tail and stage 3

def _scan(S):
    return {k: (int(v) if k in ("imax", "jmax") else float(v)) for k, v in S.items()}


def _same(got, want):
    assert [_bits(got[q]) for q in ck.QUANTITIES] == [_bits(want[q]) for q in ck.QUANTITIES], (got, {q: want[q] for q in ck.QUANTITIES})


@pytest.mark.parametrize("c", dc.CASES, ids=repr)
def test_host_tail_equals_the_restatement_on_the_cases(mv, c):
    g, e = _filter(mv, c), c.ref()
    for which in (64, 32):
        r = c.result(which)
        got = g.host_tail([_scan(S) for S in r["scans"]], None if c.prop is None else [c.prop], [c.n])[0]
        _same(got, r)


def _crafted(e, rng, k):
    """scan results at the tail's branches: flat and one-sided neighbourhoods (f2 == 0, the +-1 clamp), peaks on the edge of the search area (the veto),
    at zero (the 0.011 rule), values that put trust on either side of the limit"""
    peak = f32(rng.choice([1e3, 1e6, 3e9]))
    pos = [(0, 0), (e.dxmax, e.dymax), (e.winx - e.dxmax, e.winy - e.dymax), (1, e.winy - 1), (e.winx - 1, 0)][k % 5]
    nb = [f32(peak * f32(rng.choice([1.0, 0.999, 0.5, 0.0, 1.001]))) for _ in range(4)]
    count = (2 * e.dxmax + 1) * (2 * e.dymax + 1)
    mean = f32(peak * f32(rng.choice([0.999, 0.97, 0.9, 0.5, 0.1])))
    return dict(max=float(peak), sum=float(f32(mean * f32(count))), imax=pos[0], jmax=pos[1], xp=float(nb[0]), xm=float(nb[1]), yp=float(nb[2]), ym=float(nb[3]))


@pytest.mark.parametrize("kw", [dict(winx=64, winy=32), dict(winx=64, winy=32, fields=True, tff=1, pixaspect=1.094, stab=2.5),
                                dict(winx=128, winy=32, zoommax=1.05, trust=10.0), dict(winx=16, winy=8, dxmax=0, dymax=0, fields=True)], ids=repr)
def test_host_tail_equals_the_restatement_on_crafted_scans(mv, kw):
    g, e = mv.DepanEstimate(160, 40, **kw), er.Estimate(160, 40, **kw)
    rng = np.random.default_rng(5)
    seen = set()
    for k in range(400):
        scans = [_crafted(e, rng, k + w) for w in range(e.windows)]
        n, prop = int(rng.integers(0, 4)), int(rng.integers(0, 2))
        want = e.combine([{q: (v if q in ("imax", "jmax") else f32(v)) for q, v in S.items()} for S in scans], n, prop)
        _same(g.host_tail(scans, [prop], [n])[0], want)
        seen.add((want["dbg"][0]["scene_change"], want["dx"] == f32(0.011), want["good_zoom"]))
    assert len(seen) >= 3   # both sides of the scene-change decision and the 0.011 rule were met


def test_a_missing_field_property_without_tff_is_the_reference_s_error(mv):
    g = mv.DepanEstimate(160, 40, winx=64, winy=32, fields=True)
    S = _scan(dc.BY_NAME["fields_prop_top"].result(64)["scans"][0])
    with pytest.raises(mv.MvtoolsError) as e:
        g.host_tail([S], None, [1])
    assert str(e.value) == "DepanEstimate: _Field property not found in input frame. Therefore, you must pass tff argument."
    g.host_tail([S], [1], [1])


@pytest.mark.parametrize("nf,n,trusts,zeroed", dc.STAGE3)
def test_stage3_table(mv, nf, n, trusts, zeroed):
    g = mv.DepanEstimate(64, 48, trust=4.0, num_frames=nf)
    tri = (mv.DepanEstimateResult * 3)(*[mv.DepanEstimateResult(1.5, -2.5, 1.01, t) for t in trusts])
    m = mv.DepanMotion()
    assert mv.lib().mvx_depan_estimate_finish(g.h, n, tri, C.byref(m)) == 0
    assert (m.dx, m.dy, m.zoom, m.rot) == ((0, 0, 1, 0) if zeroed else (f32(1.5), f32(-2.5), f32(1.01), 0))


def test_finish_walks_a_run_with_clamped_ends(mv):
    g, e = mv.DepanEstimate(64, 48, trust=4.0, num_frames=4), er.Estimate(64, 48, trust=4.0, num_frames=4)
    res = [dict(dx=0.0, dy=0.0, zoom=1.0, trust=0.0), dict(dx=2.0, dy=1.0, zoom=1.0, trust=30.0), dict(dx=3.0, dy=1.0, zoom=1.0, trust=7.0),
           dict(dx=4.0, dy=1.0, zoom=1.0, trust=29.0)]
    want = [e.finish(n, [res[max(0, n - 1)], res[n], res[min(n + 1, 3)]]) for n in range(4)]
    assert g.finish(res) == [tuple(float(v) for v in w) for w in want]
    assert g.finish(res)[2] == (0, 0, 1, 0) and g.finish(res)[1][0] == 2


# ------------------------------------------------------------------------------------------------ the kernels' text on the host

def _emu_build(tmp, flags):
    exe = os.path.join(tmp, "depan_fft_emu")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "depan_fft_emu.cpp"), "-o", exe] + flags)
    return exe


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return _emu_build(str(tmp_path_factory.mktemp("emu")), ["-O2"])


def _emulate(exe, c, tmp):
    """-> spectra of prev and cur as [windows, winy, nx, 2] float32, scans as dicts"""
    e = c.ref()
    prev, cur = c.frames()
    pitch = prev.strides[0] + 6 * prev.itemsize              # a pitch that is no multiple of the window
    src, dst = os.path.join(tmp, c.name + ".in"), os.path.join(tmp, c.name + ".out")
    with open(src, "wb") as f:
        f.write(struct.pack("<11i", e.winx, e.winy, e.wleft, e.wleft + c.width // 2, e.wtop, e.windows, e.dxmax, e.dymax, int(c.bits > 8), pitch, c.height))
        for p in (prev, cur):
            rows = np.full((c.height, pitch), 0xAB, np.uint8)
            rows[:, :prev.strides[0]] = p.view(np.uint8).reshape(c.height, -1)
            f.write(rows.tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(dst, np.float32)
    n = e.windows * e.winy * (e.winx // 2 + 1) * 2
    shape = (e.windows, e.winy, e.winx // 2 + 1, 2)
    words = raw[2 * n:].view(np.uint32).reshape(e.windows, 8)
    keys = ("max", "sum", "imax", "jmax", "xp", "xm", "yp", "ym")
    scans = [{k: (int(w[i]) if k in ("imax", "jmax") else float(w[i:i + 1].view(np.float32)[0])) for i, k in enumerate(keys)} for w in words]
    return raw[:n].reshape(shape), raw[n:2 * n].reshape(shape), scans


@pytest.mark.parametrize("c", dc.CASES, ids=repr)
def test_kernel_text_on_the_host_passes_the_three_checks(mv, emu, c, tmp_path):
    sp, sc, scans = _emulate(emu, c, str(tmp_path))
    prev, cur = c.frames()
    ck.assert_spectrum(c, prev, sp)
    ck.assert_spectrum(c, cur, sc)
    result = _filter(mv, c).host_tail(scans, None if c.prop is None else [c.prop], [c.n])[0]
    ck.assert_discrete(c, scans, result)
    ck.assert_close(c, result)


# ------------------------------------------------------------------------------------------------ under the sanitizers

def _sanitizers_link(tmp):
    src = os.path.join(tmp, "one.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    if not shutil.which("g++"):
        return "no g++"
    r = subprocess.run(["g++", "-fsanitize=address,undefined", src, "-o", os.path.join(tmp, "one")], capture_output=True)
    return None if r.returncode == 0 and subprocess.run([os.path.join(tmp, "one")]).returncode == 0 else "g++ does not link -fsanitize=address,undefined here"


def test_host_tail_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    why = _sanitizers_link(str(tmp_path))
    if why:
        pytest.fail(why + ": the sanitizer run is part of this filter's checks")
    exe = str(tmp_path / "depan_estimate_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "depan_estimate_host_main.cpp"), "-o", exe] + SAN)
    for name in ("w256x128_8bit", "fields_prop_bottom", "zoom_good", "zoom_one_window_changes_scene", "scene_change_256x128", "frame0", "w64x16_dymax0"):
        c = dc.BY_NAME[name]
        e, r = c.ref(), c.result(64)
        kw = c.kw
        path = str(tmp_path / (name + ".bin"))
        pairs = [(c.n, r["scans"]), (c.n + 1, c.result(32)["scans"]), (c.n + 2, r["scans"])]
        with open(path, "wb") as f:
            f.write(struct.pack("<4f", kw.get("trust", 4.0), kw.get("zoommax", 1.0), kw.get("stab", 1.0), kw.get("pixaspect", 1.0)))
            f.write(struct.pack("<13i", kw.get("winx", 0), kw.get("winy", 0), kw.get("wleft", -1), kw.get("wtop", -1), kw.get("dxmax", -1), kw.get("dymax", -1),
                                int(e.fields), int(bool(e.tff)), int(e.tff is not None), c.width, c.height, c.bits, 3))
            f.write(struct.pack("<i", len(pairs)))
            for n, scans in pairs:
                f.write(struct.pack("<2i", -1 if c.prop is None else c.prop, n))
                for S in scans:
                    f.write(struct.pack("<2f2i4f", S["max"], S["sum"], S["imax"], S["jmax"], S["xp"], S["xm"], S["yp"], S["ym"]))
        out = subprocess.run([exe, path], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.strip().split("\n")
        assert [int(v) for v in lines[0].split()] == [e.winx, e.winy, e.wleft, e.wtop, e.dxmax, e.dymax, e.windows]
        want = [e.combine(scans, n, c.prop) for n, scans in pairs]
        for line, w in zip(lines[1:4], want):
            assert [int(v, 16) for v in line.split()] == [_bits(w[q]) for q in ck.QUANTITIES]
        e3 = er.Estimate(c.width, c.height, c.bits, **dict(kw, num_frames=3))
        for n, line in enumerate(lines[4:7]):
            m = e3.finish(n, [want[max(0, n - 1)], want[n], want[min(n + 1, 2)]])
            assert [int(v, 16) for v in line.split()] == [_bits(v) for v in m[:3]]


def test_kernel_text_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    why = _sanitizers_link(str(tmp_path))
    if why:
        pytest.fail(why + ": the sanitizer run is part of this filter's checks")
    exe = _emu_build(str(tmp_path), ["-O1", "-g"] + SAN)
    # every batch size of the transforms, both sample types, two windows, an odd origin, dymax = 0, and a search area that keeps every row
    for name in ("w8x8_8bit", "w32x16_16bit", "w512x8_8bit", "w8x1024_16bit", "w8192x8_8bit", "w8x8192_16bit", "w32x16_odd_origin", "w64x16_dymax0", "zoom_good_16bit_auto"):
        c = dc.BY_NAME[name]
        want = c.result(64)
        _, _, scans = _emulate(exe, c, str(tmp_path))
        assert [(S["imax"], S["jmax"]) for S in scans] == [(S["imax"], S["jmax"]) for S in want["scans"]]
