"""CPU tests of the restatement tests/depan_ref.py itself, which stand in for pinning it to the reference's object code: what a null
transform and a whole-pixel translation must give follows from the reference's source alone; bicubic's table; the two modes; and the
condition on the GPU parity cases of tests/depan_cases.py -- each is in domain (strict mode raises nothing) and reaches the branches it names.
The kernel's own per-sample text (csrc/mvx_depan_sample.h) is compiled for the host as well and held to the restatement on every case."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import depan_cases as dc
import depan_ref as dr

f32 = np.float32


def _src(bits, h=38, w=70, seed=4):
    pm = (1 << bits) - 1
    return np.random.default_rng(seed).integers(0, pm + 1, (h, w)).astype(np.uint16 if bits > 8 else np.uint8), pm


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("sub", [0, 1, 2])
def test_a_null_transform_returns_the_source(sub, bits):
    """nearest and bicubic exactly.  Bilinear's translation form interpolates only where rowleft < row_size - 1 (:1948-1950) and has no
    nearest-column rule there, so without MIRROR_RIGHT the last column takes the border value (:2001-2002); with it, srcp[row_size - 1]."""
    src, pm = _src(bits)
    st = {}
    out = dr.compensate_plane(src, dr.null(), sub, 0, 7, 0, pm, "strict", st)
    if sub == 1:
        assert np.array_equal(out[:, :-1], src[:, :-1]) and np.all(out[:-1, -1] == 7) and st["border"] == src.shape[0] - 1
        assert out[-1, -1] == src[-1, -1]                               # the last row copies every column (:2006-2010)
        assert np.array_equal(dr.compensate_plane(src, dr.null(), 1, 8, 7, 0, pm), src)
    else:
        assert np.array_equal(out, src) and st["border"] == 0
    assert st["cls0"] == 1


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("shift", [(3, -2), (-4, 5), (0, 1), (-1, 0)])
def test_a_whole_pixel_translation_shifts_the_source_and_fills_the_border(sub, bits, shift):
    src, pm = _src(bits)
    h, w = src.shape
    dx, dy = shift
    out = dr.compensate_plane(src, [dx, 1, 0, dy, 0, 1], sub, 0, 9, 0, pm, "strict")
    want = np.full_like(src, 9)
    ys, xs = np.arange(h) + dy, np.arange(w) + dx
    oky, okx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
    want[np.ix_(oky, okx)] = src[np.ix_(ys[oky], xs[okx])]
    if sub == 1:                                                          # bilinear: see the null transform
        want[np.ix_(oky & (ys < h - 1), xs == w - 1)] = 9
    assert np.array_equal(out, want)


def test_bicubic_table():
    t = dr.bicubic_table()
    assert t.shape == (257, 4) and t[0].tolist() == [0, 2048, 0, 0] and t[256].tolist() == [0, 0, 2048, 0]
    assert t[128].tolist() == [-256, 1280, 1280, -256]                  # -(128 * 128 * 128) / 8192, (2^24 - 2^23 + 2^21) / 8192
    assert np.all(np.abs(t.sum(axis=1) - 2048) <= 2)                   # four truncations


def test_cdiv_truncates_towards_zero():
    assert dr.cdiv(np.array([-4097, 4097, -2048, -1, 0]), 2048).tolist() == [-2, 2, -1, 0, 0]


def test_strict_mode_raises_where_the_reference_leaves_its_row():
    src, pm = _src(8)
    for sub in (0, 1, 2):
        with pytest.raises(dr.OutOfDomain):
            dr.compensate_plane(src, [-75, 1, 0, 0, 0, 1], sub, 4, 0, 0, pm, "strict")       # srcp[w0 + 75] in a row of 70
        with pytest.raises(dr.OutOfDomain):
            dr.compensate_plane(src, [150, 1, 0, 0, 0, 1], sub, 8, 0, 0, pm, "strict")       # srcp[w0 + 140 - 150 - 2]
        with pytest.raises(dr.OutOfDomain):
            dr.compensate_plane(src, [3e9, 1, 0, 0, 0, 1], sub, 0, 0, 0, pm, "strict")
        st = {}
        out = dr.compensate_plane(src, [-75, 1, 0, 0, 0, 1], sub, 4, 33, 0, pm, "library", st)
        assert st["ood"] > 0 and np.all(out[:, :5] == 33)
    with pytest.raises(dr.OutOfDomain):
        dr.compensate_plane(src, [68.5, 1, 0, 0, 0, 1], 1, 0, 0, 0, pm, "strict")              # one good column: dstp[-1]
    dr.compensate_plane(src, [67.5, 1, 0, 0, 0, 1], 1, 0, 0, 0, pm, "strict")                  # two


def test_the_chain_differs_from_the_direct_product():
    src, pm = _src(8, 8, 256)
    st = {}
    dr.compensate_plane(src, dc.rot(1.7, 1.0, 3.2, -4.1), 0, 0, 0, 0, pm, "strict", st)
    assert st["chain_differs"] > 0
    X, _ = dr._chain(dr._Plane(src, 0, "strict", None), [f32(v) for v in dc.rot(1.7, 1.0, 3.2, -4.1)])
    x = f32(3.2)
    for k in range(255):
        x = x + f32(np.cos(np.radians(1.7)))
    assert X[0, 255] == x                                                 # 255 sequential additions


@pytest.mark.parametrize("case", dc.CASES, ids=dc.ids(dc.CASES))
def test_parity_cases_are_in_domain_and_reach_their_branches(case):
    _, want, stats = dc.expected(case)                                    # strict: raises OutOfDomain otherwise
    assert not dc.missing(case, stats), stats
    assert not stats.get("ood") and not stats.get("undef")


@pytest.mark.parametrize("case", dc.LIBRARY_CASES, ids=dc.ids(dc.LIBRARY_CASES))
def test_library_cases_are_out_of_domain_on_purpose(case):
    _, _, stats = dc.expected(case)
    assert not dc.missing(case, stats), stats
    if "tail" not in case["name"]:
        with pytest.raises(dr.OutOfDomain):
            dc.expected(dict(case, mode="strict"))


def test_full_size_cases_take_seconds():
    import time
    t = time.time()
    for case in dc.FULL_CASES:
        _, _, stats = dc.expected(case)
        assert not dc.missing(case, stats), stats
    assert time.time() - t < 60


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """csrc/mvx_depan_sample.h compiled for the host (tests/depan_warp_emu.cpp)"""
    here = os.path.dirname(os.path.abspath(__file__))
    so = str(tmp_path_factory.mktemp("depan_emu") / "libdepan_emu.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I" + os.path.join(os.path.dirname(here), "vapoursynth-mvtools_amd", "csrc"),
                           os.path.join(here, "depan_warp_emu.cpp"), "-o", so])
    return C.CDLL(so)


@pytest.mark.parametrize("case", dc.CASES + dc.LIBRARY_CASES, ids=dc.ids(dc.CASES + dc.LIBRARY_CASES))
def test_the_kernel_text_on_the_host_equals_the_restatement(emu, case):
    """every sample of every plane, with a 0xA5 canary around a destination whose pitch is wider than its rows"""
    src, want, _ = dc.expected(case)
    f = dc.FORMATS[case["fmt"]]
    bps = 2 if case["bits"] > 8 else 1
    for k, t in enumerate(case["trs"]):
        for p, (tp, blur) in enumerate(dr.plane_transforms(t, f["subsampling"], f.get("gray", False), case["blur"])):
            s = np.ascontiguousarray(src[p])
            h, w = s.shape
            pitch = w * bps + 6
            buf = np.full((h + 2, pitch), 0xA5, np.uint8)
            tt = np.ascontiguousarray(tp, dtype=f32)
            emu.depan_emu_plane(C.c_void_p(s.ctypes.data), C.c_longlong(w * bps), w, h, bps, case["sub"], case["mirror"], (1 << case["bits"]) - 1,
                                0 if p == 0 else 1 << (case["bits"] - 1), blur, C.c_void_p(tt.ctypes.data), C.c_void_p(buf[1:].ctypes.data), C.c_longlong(pitch))
            got = np.ascontiguousarray(buf[1:-1, :w * bps]).view(s.dtype)
            assert np.array_equal(got, want[k][p]), (k, p, tt.tolist())
            assert np.all(buf[0] == 0xA5) and np.all(buf[-1] == 0xA5) and np.all(buf[1:-1, w * bps:] == 0xA5)


def test_the_kernel_text_under_the_sanitizers_on_the_library_cases(tmp_path):
    """the out-of-domain cases are where an index could leave a plane: the same text as a stand-alone program under AddressSanitizer and
    UBSan, on heap planes of exactly the plane's size.  Nothing loaded into python runs under a sanitizer."""
    here = os.path.dirname(os.path.abspath(__file__))
    one = tmp_path / "one.cpp"
    one.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]   # the last: undefined float -> int conversions
    if not shutil.which("g++") or subprocess.run(["g++"] + flags + [str(one), "-o", str(tmp_path / "one")], capture_output=True).returncode or \
            subprocess.run([str(tmp_path / "one")]).returncode:
        pytest.skip("g++ does not link -fsanitize=address,undefined here")
    exe = str(tmp_path / "depan_warp_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DDEPAN_EMU_MAIN"] + flags + [
        "-I" + os.path.join(os.path.dirname(here), "vapoursynth-mvtools_amd", "csrc"), os.path.join(here, "depan_warp_emu.cpp"), "-o", exe])
    runs = 0
    for case in dc.LIBRARY_CASES + [c for c in dc.CASES if c["name"] in ("small_s0_8", "small_s1_16", "small_s2_8", "gray_s2", "f444_s1")]:
        src, want, _ = dc.expected(case)
        f = dc.FORMATS[case["fmt"]]
        bps = 2 if case["bits"] > 8 else 1
        for k, t in enumerate(case["trs"]):
            for p, (tp, blur) in enumerate(dr.plane_transforms(t, f["subsampling"], f.get("gray", False), case["blur"])[:2]):
                h, w = src[p].shape
                fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
                with open(fin, "wb") as fh:
                    fh.write(struct.pack("<8i", w, h, bps, case["sub"], case["mirror"], (1 << case["bits"]) - 1, 0 if p == 0 else 1 << (case["bits"] - 1), blur))
                    fh.write(np.ascontiguousarray(tp, dtype=f32).tobytes())
                    fh.write(np.ascontiguousarray(src[p]).tobytes())
                r = subprocess.run([exe, "compensate", fin, fout], capture_output=True, text=True)
                assert r.returncode == 0, (case["name"], k, p, r.stderr[-2000:])
                got = np.fromfile(fout, dtype=src[p].dtype).reshape(h, w)
                assert np.array_equal(got, want[k][p]), (case["name"], k, p)
                runs += 1
    assert runs > 100
