"""`show` of mv.DepanEstimate: mvx_depan_estimate_correlate_show (csrc/mvx_depan_fft.hip) paints the correlation surface into the window(s) of a copy
of the luma plane, as showcorrelation does (MVDepan.cpp:895-953).  The surface comes out of a single-precision FFT, so the paint is held to the paint
restated in numpy (the float32 arithmetic of :903-947) on the surface of tests/depan_estimate_ref.py with the double FFT, within max(1, 4 * Dshow):
Dshow is the largest per-sample distance over the cases below between that paint on scipy's single-precision surface and on its double one,
computed here, never from the code under test.  Everything outside the window rectangles is the input, byte for byte; the results and scan results
of the call equal those of mvx_depan_estimate_correlate bit for bit.

The cases: the smallest window (8 x 8); windows of which the scan keeps only some rows (2 * dymax + 3 < winy), where the surface of the scan and the
full one differ in layout; one whose scan keeps every row (dymax = winy / 2 - 1); two windows; 8, 10 and 16 bits; a window with an odd origin; one
large enough for several workgroups of the minimum / maximum and paint passes (256 x 128: 8 groups).  The CPU twin compiles the text of the passes
(csrc/mvx_depan_fft_core.h) for the host (tests/depan_show_emu.cpp) and holds its paint to the numpy paint exactly, on the very surface it painted."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import depan_estimate_cases as dc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vapoursynth-mvtools_amd", "csrc")
f32 = np.float32

ALL_ROWS = dc.Case("w32x16_all_rows", 38, 20, 8, "pan", 207, pan=(3, 2), winx=32, winy=16, dymax=7)
CASES = [dc.BY_NAME[n] for n in ("w8x8_8bit", "w8x8_16bit", "w16x64_8bit", "w32x16_16bit", "w64x32_10bit", "w32x16_odd_origin", "w256x128_16bit", "zoom_good",
                                 "zoom_good_16bit_auto")] + [ALL_ROWS]


def test_the_cases_cover_what_they_claim():
    e = ALL_ROWS.ref()
    assert min(e.winy, 2 * e.dymax + 3) == e.winy
    assert all(min(c.ref().winy, 2 * c.ref().dymax + 3) < c.ref().winy for c in CASES[:-1])
    assert sorted({c.ref().windows for c in CASES}) == [1, 2] and sorted({c.bits for c in CASES}) == [8, 10, 16]
    assert (CASES[0].ref().winx, CASES[0].ref().winy) == (8, 8)


def paint(surface, pixel_max):
    """showcorrelation, :903-947, of one float32 surface [winy, winx] -> integers; a flat surface gives zeros (the library's divergence 13)"""
    s = np.asarray(surface, dtype=f32)
    cmin, cmax = s.min(), s.max()
    if cmax == cmin:
        return np.zeros(s.shape, np.int64)
    norm = f32(f32(pixel_max) / f32(cmax - cmin))
    return ((s - cmin) * norm).astype(f32).astype(np.int64)


@functools.lru_cache(maxsize=None)
def painted(c, which):
    return [paint(s, (1 << c.bits) - 1) for s in c.result(which)["surfaces"]]


@functools.lru_cache(maxsize=None)
def Dshow():
    return max(int(abs(a - b).max()) for c in CASES for a, b in zip(painted(c, 32), painted(c, 64)))


def rect(c, w):
    e = c.ref()
    left = e.wleft + (c.width // 2 if w else 0)
    return slice(e.wtop, e.wtop + e.winy), slice(left, left + e.winx)


# ------------------------------------------------------------------------------------------------ the text of the passes on the host

@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("show_emu") / "depan_show_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "depan_show_emu.cpp"), "-o", exe])
    return exe


def _emulate(exe, c, prev, cur, tmp):
    """-> the surfaces [windows, winy, winx] and the painted plane [height, width] of the host build"""
    e = c.ref()
    pitch = prev.strides[0] + 6 * prev.itemsize
    src, dst = os.path.join(tmp, c.name + ".in"), os.path.join(tmp, c.name + ".out")
    with open(src, "wb") as f:
        f.write(struct.pack("<12i", e.winx, e.winy, e.wleft, e.wleft + c.width // 2, e.wtop, e.windows, e.dxmax, e.dymax, int(c.bits > 8), pitch, c.height,
                            (1 << c.bits) - 1))
        for p in (prev, cur):
            rows = np.full((c.height, pitch), 0xAB, np.uint8)
            rows[:, :prev.strides[0]] = p.view(np.uint8).reshape(c.height, -1)
            f.write(rows.tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(dst, np.uint8)
    n = e.windows * e.winy * e.winx * 4
    surfaces = raw[:n].view(np.float32).reshape(e.windows, e.winy, e.winx)
    rows = raw[n:].reshape(c.height, pitch)
    assert np.all(rows[:, prev.strides[0]:] == 0xAB)
    return surfaces, rows[:, :prev.strides[0]].copy().view(prev.dtype)


def _check_plane(c, cur, got, D, exact_surfaces=None):
    want = cur.astype(np.int64)
    outside = np.ones(cur.shape, bool)
    pm = (1 << c.bits) - 1
    for w in range(c.ref().windows):
        outside[rect(c, w)] = False
        inside = got[rect(c, w)].astype(np.int64)
        if exact_surfaces is not None:
            assert np.array_equal(inside, paint(exact_surfaces[w], pm))
        s64 = c.result(64)["surfaces"][w]
        lo, hi = np.unravel_index(np.argmin(s64), s64.shape), np.unravel_index(np.argmax(s64), s64.shape)
        off = int(abs(inside - painted(c, 64)[w]).max())
        print("%s window %d: at the minimum %d, at the maximum %d of %d, off by at most %d (max(1, 4 Dshow) = %d)" % (c.name, w, inside[lo], inside[hi], pm, off,
                                                                                                                 max(1, 4 * D)))
        assert inside[lo] == 0 and inside[hi] in (pm, pm - 1)
        assert off <= max(1, 4 * D)
    assert np.array_equal(got.astype(np.int64)[outside], want[outside])


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_kernel_text_on_the_host_paints_as_numpy_does(emu, c, tmp_path):
    print("Dshow = %d" % Dshow())
    prev, cur = c.frames()
    surfaces, got = _emulate(emu, c, prev, cur, str(tmp_path))
    _check_plane(c, cur, got, Dshow(), exact_surfaces=surfaces)


def test_kernel_text_on_the_host_paints_a_flat_surface_black(emu, tmp_path):
    c = dc.BY_NAME["w32x16_odd_origin"]
    flat = np.full((c.height, c.width), 7, np.uint8)
    surfaces, got = _emulate(emu, c, flat, flat, str(tmp_path))
    assert surfaces.min() == surfaces.max() != 0
    want = flat.copy()
    want[rect(c, 0)] = 0
    assert np.array_equal(got, want)


def test_kernel_text_in_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """the show passes index the surface, the partial results and the plane: AddressSanitizer and UBSan over the host build, every case"""
    probe = tmp_path / "one.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "one")], capture_output=True).returncode != 0:
        pytest.fail("g++ does not link -fsanitize=address,undefined here: the sanitizer run is part of this filter's checks")
    exe = str(tmp_path / "depan_show_emu_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "depan_show_emu.cpp"), "-o", exe] + san)
    for c in CASES:
        prev, cur = c.frames()
        surfaces, got = _emulate(exe, c, prev, cur, str(tmp_path))
        for w in range(c.ref().windows):
            assert np.array_equal(got[rect(c, w)].astype(np.int64), paint(surfaces[w], (1 << c.bits) - 1))


# ------------------------------------------------------------------------------------------------ on the GPU

_runs = {}


def _dev(plane):
    """a device plane whose pitch is its row plus 6 samples: no multiple of any window"""
    import torch
    h, rowbytes = plane.shape[0], plane.shape[1] * plane.itemsize
    t = torch.full((h, rowbytes + 6 * plane.itemsize), 0xAB, dtype=torch.uint8, device="cuda")
    t[:, :rowbytes] = torch.from_numpy(plane.view(np.uint8).reshape(h, rowbytes)).to("cuda")
    return t


def _run(mv, c, frames=None):
    key = c.name if frames is None else None
    if key is None or key not in _runs:
        g = mv.DepanEstimate(c.width, c.height, c.bits, **c.kw)
        prev, cur = frames or c.frames()
        dprev, dcur = _dev(prev), _dev(cur)
        sp = g.spectra([dprev, dcur])
        prop, before = None if c.prop is None else [c.prop], dcur.cpu().numpy().copy()
        plain = g.correlate([sp[0]], [sp[1]], prop, [c.n], scans=True)
        res, scans, shown = g.correlate([sp[0]], [sp[1]], prop, [c.n], scans=True, show=[dcur])
        assert np.array_equal(dcur.cpu().numpy(), before)      # the caller's plane is not the painted one
        rows = shown[0].cpu().numpy()
        rowbytes = cur.shape[1] * cur.itemsize
        assert np.all(rows[:, rowbytes:] == 0xAB)
        r = dict(plain=plain, show=(res, scans), plane=rows[:, :rowbytes].copy().view(cur.dtype))
        if key is None:
            return r
        _runs[key] = r
    return _runs[key]


def _bits(v):
    return f32(v).tobytes() if isinstance(v, float) else v


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=repr)
def test_show_paints_the_window_and_nothing_else(mv, c):
    print("Dshow = %d" % Dshow())
    _check_plane(c, c.frames()[1], _run(mv, c)["plane"], Dshow())


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=repr)
def test_results_and_scans_of_the_show_call_equal_the_plain_call_bit_for_bit(mv, c):
    r = _run(mv, c)
    for (pres, pscans), (sres, sscans) in [(r["plain"], r["show"])]:
        assert [[_bits(v) for v in d.values()] for d in pres] == [[_bits(v) for v in d.values()] for d in sres]
        assert [[_bits(v) for v in d.values()] for d in pscans] == [[_bits(v) for v in d.values()] for d in sscans]
        assert len(pscans) == c.ref().windows


@pytest.mark.gpu
def test_frame_zero_is_painted_like_any_other_pair(mv):
    c = dc.BY_NAME["frame0"]
    r = _run(mv, c)
    assert tuple(r["show"][0][0].values()) == (0, 0, 1, 0)
    _check_plane(c, c.frames()[1], r["plane"], Dshow())


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [8, 16])
def test_a_constant_frame_paints_zeros(mv, bits):
    c = dc.BY_NAME["zoom_good" if bits == 8 else "zoom_good_16bit_auto"]
    flat = np.full((c.height, c.width), 7, np.uint8 if bits == 8 else np.uint16)
    got = _run(mv, c, (flat, flat))["plane"]
    want = flat.copy()
    for w in range(2):
        want[rect(c, w)] = 0
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_show_refuses_a_missing_plane_and_a_short_pitch(mv):
    import ctypes as C
    c = dc.BY_NAME["w8x8_8bit"]
    g = mv.DepanEstimate(c.width, c.height, c.bits, **c.kw)
    sp = g.spectra([_dev(p) for p in c.frames()])
    ptr = lambda t: (C.c_void_p * 1)(t.data_ptr())
    out, lib = (mv.DepanEstimateResult * 1)(), mv.lib()
    plane = _dev(c.frames()[1])
    assert lib.mvx_depan_estimate_correlate_show(g.h, 1, ptr(sp[0]), ptr(sp[1]), None, None, out, None, None, plane.stride(0), None) != 0
    assert lib.mvx_depan_estimate_correlate_show(g.h, 1, ptr(sp[0]), ptr(sp[1]), None, None, out, None, ptr(plane), c.width - 1, None) != 0
    assert lib.mvx_depan_estimate_correlate_show(g.h, 0, None, None, None, None, None, None, None, 0, None) == 0
