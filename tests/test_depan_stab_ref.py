"""CPU tests of DepanStabilise's painting: the restatement tests/depan_stab_ref.py against what follows from the reference's source alone, the
condition on the cases of tests/depan_stab_cases.py -- each reaches the sources and branches it names -- and the kernel's own per-sample text
(csrc/mvx_depan_sample.h) compiled for the host and held to the restatement's sequential painting on every case, so that the fused
selection is proven before a GPU sees it.  The same text and the host planner run as a stand-alone program under AddressSanitizer and UBSan;
nothing loaded into python runs under a sanitizer."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import depan_cases as dc
import depan_ref as dr
import depan_stab_cases as sc
import depan_stab_ref as sr

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vapoursynth-mvtools_amd", "csrc")


def _frames(bits=8, n=3, seed=3):
    c = dict(bits=bits, seed=seed, fmt="420", w=70, h=38)
    return sc.sources(c)[:n]


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_without_fill_sources_the_painting_is_depan_compensate_s(sub):
    src = _frames()
    for t in sc.T3 + sc.R3 + sc.Z3:
        got = sr.paint(src[0], t, None, None, sub, 8, (1, 1), False, 15, 3)
        want = dr.compensate_frame(src[0], t, sub, 8, (1, 1), False, 15, 3, "library")
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("sub", [0, 2])
def test_the_order_of_the_sources(sub):
    """whole-pixel shifts, so that every sample can be named: the current frame where its position is inside, else next, else prev, else prev's
    border value -- and with a mirror only prev, the first pass, mirrors"""
    src = [[np.full((38, 70), v, np.uint8), np.full((19, 35), v, np.uint8), np.full((19, 35), v, np.uint8)] for v in (10, 20, 30)]
    args = (src[0], dc.tr(8, 0), (src[2], dc.tr(0, 36)), (src[1], dc.tr(0, -5)), sub)
    out = sr.paint(*args)[0]
    want = np.zeros((38, 70), np.uint8)             # prev's border value ...
    want[:2, :] = 30                                # ... below its rows 0 and 1
    want[5:, :] = 20                                # next: rows 5 .. 37
    want[:, :62] = 10                               # the current frame: columns 0 .. 61
    assert np.array_equal(out, want)
    out = sr.paint(*args, mirror=15)[0]
    want[2:5, 62:] = 30                             # prev mirrors at the bottom; next and the current frame mirror nothing
    assert np.array_equal(out, want)
    st = {}
    sr.paint(*args, stats=st)
    assert st["from_cur"] == 62 * 38 + 2 * 31 * 19 and st["from_next"] == 8 * 33 + 2 * 4 * 17 and st["from_prev"] == 8 * 5 + 2 * 4 * 2 and st["passes"] == 9


def test_next_alone_is_the_first_pass_and_mirrors():
    src = [[np.full((38, 70), v, np.uint8)] for v in (10, 20)]
    out = sr.paint(src[0], dc.tr(8, 0), None, (src[1], dc.tr(0, 6)), 0, gray=True, mirror=2)[0]
    assert np.all(out[:, :62] == 10) and np.all(out[:, 62:] == 20)
    out = sr.paint(src[0], dc.tr(8, 0), None, (src[1], dc.tr(0, 6)), 0, gray=True)[0]
    assert np.all(out[:32, 62:] == 20) and np.all(out[32:, 62:] == 0)


def test_a_nan_transform_leaves_the_plane_to_the_other_sources():
    src = _frames()
    nan = dc.tr(np.nan, 0)
    st = {}
    out = sr.paint(src[0], nan, (src[2], sc.T3[2]), (src[1], sc.T3[1]), 2, stats=st)
    want = sr.paint(src[1], sc.T3[1], (src[2], sc.T3[2]), None, 0)
    assert all(np.array_equal(a, b) for a, b in zip(out, want)) and st["from_cur"] == 0
    out = sr.paint(src[0], nan, None, None, 2)
    assert np.all(out[0] == 0) and np.all(out[1] == 128)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.ids(sc.CASES))
def test_cases_reach_what_they_name(case):
    _, _, stats = sc.expected(case)
    assert not sc.missing(case, stats), stats


def test_full_size_cases_take_seconds():
    import time
    t = time.time()
    for case in sc.FULL_CASES:
        _, _, stats = sc.expected(case)
        assert not sc.missing(case, stats), stats
    assert time.time() - t < 60


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """csrc/mvx_depan_sample.h and csrc/mvx_depan_stab_host.h compiled for the host (tests/depan_warp_emu.cpp)"""
    so = str(tmp_path_factory.mktemp("depan_stab_emu") / "libdepan_stab_emu.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I" + CSRC, os.path.join(HERE, "depan_warp_emu.cpp"), "-o", so])
    return C.CDLL(so)


def _plane_jobs(case):
    """per job and plane: the three source planes (None where absent), the 18 floats, border, blur, subsampling"""
    src, want, _ = sc.expected(case)
    f = dc.FORMATS[case["fmt"]]
    gray = f.get("gray", False)
    ssw, ssh = (0, 0) if gray else f["subsampling"]
    for k, (cur, nxt, prev) in enumerate(case["jobs"]):
        trs = np.zeros((3, 6), f32)
        trs[0] = cur
        if nxt is not None:
            trs[1] = nxt[1]
        if prev is not None:
            trs[2] = prev[1]
        for p in range(len(src[0])):
            planes = [src[0][p], None if nxt is None else src[nxt[0]][p], None if prev is None else src[prev[0]][p]]
            blur = case["blur"] // 2 if p and ssw else case["blur"]
            yield k, p, planes, trs, 0 if p == 0 else 1 << (case["bits"] - 1), blur, ssw, ssh, want[k][p]


@pytest.mark.parametrize("case", sc.CASES, ids=sc.ids(sc.CASES))
def test_the_kernel_text_on_the_host_equals_the_sequential_painting(emu, case):
    """every sample of every plane, with a 0xA5 canary around a destination whose pitch is wider than its rows"""
    bps = 2 if case["bits"] > 8 else 1
    for k, p, planes, trs, border, blur, ssw, ssh, want in _plane_jobs(case):
        h, w = want.shape
        keep = [None if s is None else np.ascontiguousarray(s) for s in planes]
        ptrs = (C.c_void_p * 3)(*[None if s is None else s.ctypes.data for s in keep])
        pitch = w * bps + 6
        buf = np.full((h + 2, pitch), 0xA5, np.uint8)
        emu.depan_stab_emu_plane(ptrs, C.c_longlong(w * bps), w, h, bps, case["sub"], case["mirror"], (1 << case["bits"]) - 1, border, blur, ssw, ssh, p,
                                 C.c_void_p(trs.ctypes.data), C.c_void_p(buf[1:].ctypes.data), C.c_longlong(pitch))
        got = np.ascontiguousarray(buf[1:-1, :w * bps]).view(want.dtype)
        assert np.array_equal(got, want), (k, p, trs.tolist())
        assert np.all(buf[0] == 0xA5) and np.all(buf[-1] == 0xA5) and np.all(buf[1:-1, w * bps:] == 0xA5)


def plan_input(e, fps, ndest, motions):
    """the input of `depan_warp_emu plan` / depan_stab_emu_plan for the restatement object e, whose arguments are kept in e.args"""
    a = e.args
    ints = [e.width, e.height, e.num_frames, int(a["addzoom"]), a["prev"], a["next"], a["mirror"], a["blur"], a["subpixel"], a["fitlast"], a["method"], int(a["fields"])]
    floats = [a[k] for k in ("cutoff", "damping", "initzoom", "dxmax", "dymax", "zoommax", "rotmax", "pixaspect", "tzoom")]
    w = e.window(ndest)
    ms = np.array([motions[n] for n in range(w[0], w[1] + 1)], dtype=f32)
    return ints, floats, ms


def test_the_planner_and_the_kernel_text_under_the_sanitizers(tmp_path):
    """heap planes of exactly the plane's size: an index outside them, a signed overflow or an undefined float -> int conversion ends the program"""
    one = tmp_path / "one.cpp"
    one.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]
    if not shutil.which("g++") or subprocess.run(["g++"] + flags + [str(one), "-o", str(tmp_path / "one")], capture_output=True).returncode or \
            subprocess.run([str(tmp_path / "one")]).returncode:
        pytest.skip("g++ does not link -fsanitize=address,undefined here")
    exe = str(tmp_path / "depan_warp_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DDEPAN_EMU_MAIN"] + flags + ["-I" + CSRC, os.path.join(HERE, "depan_warp_emu.cpp"), "-o", exe])
    runs = 0
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    names = ("small_s0_8", "small_s1_16", "small_s2_8", "gray_s2", "f444_s1", "undef_s0", "undef_s1", "undef_s2", "self_s2", "covers_s2")
    for case in [c for c in sc.CASES if c["name"] in names]:
        bps = 2 if case["bits"] > 8 else 1
        for k, p, planes, trs, border, blur, ssw, ssh, want in _plane_jobs(case):
            if p == 2:
                continue
            h, w = want.shape
            with open(fin, "wb") as fh:
                fh.write(struct.pack("<13i", w, h, bps, case["sub"], case["mirror"], (1 << case["bits"]) - 1, border, blur, ssw, ssh, p, planes[1] is not None, planes[2] is not None))
                fh.write(trs.tobytes())
                for s in planes:
                    if s is not None:
                        fh.write(np.ascontiguousarray(s).tobytes())
            r = subprocess.run([exe, "plane", fin, fout], capture_output=True, text=True)
            assert r.returncode == 0, (case["name"], k, p, r.stderr[-2000:])
            assert np.array_equal(np.fromfile(fout, dtype=want.dtype).reshape(h, w), want), (case["name"], k, p)
            runs += 1
    assert runs > 100
    # the planner: both methods, with and without the adaptive zoom, a bad frame in the middle, fills either side, the radius-0 NaN
    plans = 0
    for kw in (dict(method=0, prev=2, next=3, cutoff=0.5), dict(method=0, addzoom=1, prev=1, fitlast=6, dxmax=-2.0), dict(method=1, prev=2, next=2, cutoff=0.5),
               dict(method=1, addzoom=1, next=9, cutoff=2.0), dict(method=1, cutoff=7.0, prev=1, next=1)):
        n = 24
        motions = sc.track(n, 7, bad=(11,))
        e = sr.Stabilise(70, 38, n, **kw)
        for ndest in (0, 1, 10, 11, 12, 17, n - 1):
            ints, floats, ms = plan_input(e, (25, 1), ndest, motions)
            with open(fin, "wb") as fh:
                fh.write(struct.pack("<12i9f2q2i", *ints, *floats, 25, 1, ndest, len(ms)))
                fh.write(ms.tobytes())
            r = subprocess.run([exe, "plan", fin], capture_output=True, text=True)
            assert r.returncode == 0, (kw, ndest, r.stderr[-2000:])
            assert [int(v, 16) for v in r.stdout.split()] == sr.plan_words(e.plan(ndest, motions)), (kw, ndest)
            plans += 1
    assert plans == 35
