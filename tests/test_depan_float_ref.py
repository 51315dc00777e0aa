"""CPU tests of the float rule of DepanCompensate and DepanStabilise.

1. tests/depan_float_ref.py is anchored to the integer restatement tests/depan_ref.py on integer-valued float clips (the values of an 8-bit
   clip as float32), on the geometries and transforms of depan_cases.CASES / LIBRARY_CASES and depan_stab_cases.CASES:
     border    samples are those where depan_ref.compensate_plane gives different results for two border values; there the float result is
               exactly 0.0f (luma) / 0.5f (chroma), and nowhere else is the restatement's kind BORDER.
     copies    equal.
     bilinear  floor(float) == integer.  With samples a..d in 0..255 the numerator N = (32 - ky) * ((32 - kx) * a + kx * b) + ky * ((32 - kx) * c
               + kx * d) is an integer <= 1024 * 255 < 2^18 and every partial product and sum is an integer below 2^24, so float32 holds each
               exactly; 1 / 1024 is a power of two, so the float result is N / 1024 exactly, and the integer path's is N >> 10, its floor.
     blur      floor(float) == integer.  A run of n <= 9 samples sums to an integer s <= 9 * 255, exact in float32.  The integer path gives
               s / n truncated, the floor.  s / n is either an integer, which the correctly rounded float division returns exactly, or at
               least 1 / n >= 1 / 9 below the next integer, far more than float32's spacing (2^-16 below 256): rounding cannot reach it.
     mean      the zoom form's bottom row: a + b is exact and * 0.5f is exact, so floor(float) == (a + b) / 2.
     bicubic   within BOUND_SEP (zoom, rotation) / BOUND_TRANS (translation) / BOUND_NEAR (near-edge rows), derived below from the
               reference's own truncations, not measured.  Samples where the integer result is 0 or pixel_max may have been clamped; they are
               held to the one-sided bound a clamp leaves (float < 1 + bound, float > 254 - bound) and their share is capped at the largest
               share the reference alone shows on the noise cases.
2. Float-only properties: a flat 0.5f plane stays 0.5f bit for bit wherever a source covers the sample; bicubic overshoots 0 and 1 on a
   checkerboard (no clamp); NaN, +-Inf, -0.0f, denormals and negatives pass through every copy path bit for bit; a negative current frame
   of DepanStabilise is never overpainted where it covers the sample (the painted flag).
3. csrc/mvx_depan_sample_float.h compiled for the host (tests/depan_float_emu.cpp) equals the restatement bit for bit on every case; once
   more as a stand-alone program under AddressSanitizer and UBSan on the library cases.  Nothing loaded into python runs under a sanitizer."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import depan_cases as dc
import depan_float_cases as fc
import depan_float_ref as fr
import depan_ref as dr
import depan_stab_cases as sc
import depan_stab_ref as sr

f32, u32 = np.float32, np.uint32
NOISE = [c for c in dc.CASES if c["src"] == "noise"]
ALL = NOISE + dc.LIBRARY_CASES

# ---- the bicubic bounds, in output units at 8 bits (samples 0..255).  tab: the reference's table, entries the cubic weights * 2048, truncated.
_tab = dr.bicubic_table()
_sum = _tab.sum(axis=1)                                   # 2048 but for the four truncations
_abs = np.abs(_tab).sum(axis=1).max()                     # the largest sum of magnitudes of a table row
# the float rule divides by Sx * Sy where the integer path shifts by 22: the exact values differ by |N / 2^22| * |2^22 / (Sx * Sy) - 1|,
# and |N / 2^22| < 258 wherever the integer result is inside 0..255 (it is within 1, 2.5 for the translation form, of N / 2^22)
_RHO = max(abs(float(2 ** 22) / (a * b) - 1) for a in (_sum.min(), _sum.max()) for b in (_sum.min(), _sum.max()))
# float32 rounding of the float rule: the row sums are integers below 2^24 (|ts| <= _abs * 255), exact; the column sum is four products
# and three additions of magnitude <= _abs * _abs * 255, each rounded once (2^-24 relative); the division adds one rounding of the result
_FLT = (7 * 2.0 ** -24 * _abs * _abs * 255) / (_sum.min() ** 2) + 258 * 2.0 ** -23
# zoom and rotation: N >> 22 is the floor of N / 2^22: below it by less than 1
BOUND_SEP = 1 + 258 * _RHO + _FLT
# translation: sixteen coefficients (cy * cx) / 2048, each truncated by less than 1 (in units of 1 / 2048, times a sample <= 255), then
# (1024 + sum) >> 11, round-half-up: within 1 / 2
BOUND_TRANS = 16 * 255 / 2048.0 + 0.5 + 258 * _RHO + _FLT
# near-edge rows: the reference's double expression against its float32 evaluation (four products, three sums, two weights 1 - s, each
# rounded once at magnitude <= 255: 2^-24 * 255 * 12), then the (int) cast, which truncates a non-negative value by less than 1.  The
# products sx * sample are float in the reference too.
BOUND_NEAR = 1 + 12 * 255 * 2.0 ** -24


def test_the_bounds_are_what_the_derivation_gives():
    assert _sum.min() >= 2046 and _sum.max() <= 2050 and _abs == 3072
    assert 1 < BOUND_SEP < 1.6 and 2.4 < BOUND_TRANS < 3.1 and 1 < BOUND_NEAR < 1.001


def _reference_share(c):
    """the share of bicubic's computed samples (the interpolator proper and the near-edge rows) that the reference clamped, by its own counters"""
    _, _, st = dc.expected(fc.eight(c))
    return (st.get("clamp_lo", 0) + st.get("clamp_hi", 0)) / max(st.get("interp", 0) + st.get("near", 0), 1)


@pytest.fixture(scope="module")
def clamp_cap():
    """The excluded samples are those with the integer result 0 or 255: the clamped ones, and those whose unclamped result is exactly 0 or 255,
    two of the 256 levels of a result that noise spreads over all of them: 2 / 256 on top of the largest clamped share of a noise case."""
    return max(_reference_share(c) for c in NOISE if c["sub"] == 2) + 2 / 256.0


def _anchor_plane(src8, t, c, p, blur, got, kind, counts):
    """one plane of one transform: got / kind from the float restatement on src8.astype(float32)"""
    border = (0, 128)[p > 0]
    a = dr.compensate_plane(src8, t, c["sub"], c["mirror"], 1, blur, 255, "library")
    b = dr.compensate_plane(src8, t, c["sub"], c["mirror"], 254, blur, 255, "library")
    isb = a != b
    assert np.array_equal(isb, kind == fr.BORDER), "the border sets differ"
    assert np.all(got[isb].view(u32) == np.array([fr.BORDER_VALUE[p > 0]], f32).view(u32)[0])
    a = a.astype(np.int64)
    m = kind == fr.COPY
    assert np.array_equal(got[m], a[m].astype(f32)), "copies"
    for k in (fr.BLUR, fr.MEAN) + ((fr.INTERP,) if c["sub"] == 1 else ()):
        m = kind == k
        assert np.array_equal(np.floor(got[m]).astype(np.int64), a[m]), "floor equality, kind %d" % k
    if c["sub"] == 2:
        cls0 = t[1] == 1 and t[5] == 1 and t[2] == 0 and t[4] == 0
        for k, bound in ((fr.INTERP, BOUND_TRANS if cls0 else BOUND_SEP), (fr.NEAR, BOUND_NEAR)):
            m = kind == k
            g, w = got[m].astype(np.float64), a[m]
            inside = (w > 0) & (w < 255)
            assert np.all(np.abs(g[inside] - w[inside]) <= bound), (k, np.abs(g[inside] - w[inside]).max(), bound)
            assert np.all(g[w == 0] < 1 + bound) and np.all(g[w == 255] > 254 - bound)
            counts[0] += int((~inside).sum())
            counts[1] += int(m.sum())


@pytest.mark.parametrize("case", ALL, ids=dc.ids(ALL))
def test_the_restatement_on_integer_valued_clips_is_anchored_to_the_integer_restatement(case, clamp_cap):
    src, want, kinds, stats = fc.expected(case, "int8")
    src8 = dc.source(fc.eight(case))
    f = dc.FORMATS[case["fmt"]]
    counts = [0, 0]
    for k, t in enumerate(case["trs"]):
        for p, (tp, blur) in enumerate(dr.plane_transforms(t, f["subsampling"], f.get("gray", False), case["blur"])):
            _anchor_plane(src8[p], tp, case, p, blur, want[k][p], kinds[k][p], counts)
    assert not dc.missing(case, stats), stats                              # the float restatement reaches the branches the case names
    assert counts[0] <= clamp_cap * counts[1], (counts, clamp_cap)


STAB = sc.CASES


@pytest.mark.parametrize("case", STAB, ids=sc.ids(STAB))
def test_the_float_paint_on_integer_valued_clips_is_anchored_to_the_sequential_integer_paint(case):
    """Border samples of chroma are where the integer paint at 8 and at 9 bits differ (128 against 256; with bicubic also where 255 was a
    clamp, which the test excludes anyway); luma's border is 0 in both paths.  Elsewhere: floor equality for nearest and bilinear, the
    translation form's bound (the largest) for bicubic."""
    frames, want, who, stats = fc.stab_expected(case, "int8")
    c8 = fc.eight(case)
    src8 = sc.sources(c8)
    f = dc.FORMATS[case["fmt"]]
    for k, (cur, nxt, prev) in enumerate(case["jobs"]):
        args = (src8[0], cur, None if prev is None else (src8[prev[0]], prev[1]), None if nxt is None else (src8[nxt[0]], nxt[1]), case["sub"])
        tail = (f["subsampling"], f.get("gray", False), case["mirror"], case["blur"])
        a = sr.paint(*args, 8, *tail)
        wide = lambda s: None if s is None else ([p.astype(np.uint16) for p in s[0]], s[1])
        b = sr.paint([p.astype(np.uint16) for p in args[0]], cur, wide(args[2]), wide(args[3]), case["sub"], 9, *tail)
        for p in range(len(a)):
            got, w = want[k][p], a[p].astype(np.int64)
            isb = (w != b[p]) & (w == 128) if p else np.zeros(w.shape, bool)
            assert np.all(got[isb] == f32(0.5))
            rest = ~isb
            if case["sub"] < 2:
                assert np.array_equal(np.floor(got[rest]).astype(np.int64), w[rest]), (k, p)
            else:
                inside = rest & (w > 0) & (w < 255)
                assert np.all(np.abs(got[inside].astype(np.float64) - w[inside]) <= BOUND_TRANS), (k, p)
    assert not sc.missing(case, stats), stats


# ------------------------------------------------------------------------------------------------ float-only properties

@pytest.mark.parametrize("case", ALL, ids=dc.ids(ALL))
def test_a_flat_plane_stays_flat_bit_for_bit(case):
    _, want, kinds, _ = fc.expected(case, "flat")
    half = np.array([0.5], f32).view(u32)[0]
    for k in range(len(want)):
        for p in range(len(want[k])):
            covered = kinds[k][p] != fr.BORDER
            assert np.all(want[k][p].view(u32)[covered] == half), (k, p)


@pytest.mark.parametrize("case", [c for c in STAB if c["name"].startswith(("combos", "blur9", "mirror15"))], ids=lambda c: c["name"])
def test_a_flat_stabilised_plane_stays_flat(case):
    _, want, who, _ = fc.stab_expected(case, "flat")
    for k in range(len(want)):
        for p in range(1, len(want[k])):                       # chroma: the border value is 0.5f too, so the whole plane
            assert np.all(want[k][p] == f32(0.5))


def test_bicubic_overshoots_below_0_and_above_1_on_a_checkerboard():
    case = [c for c in dc.CASES if c["name"] == "clamp_8"][0]
    _, want, kinds, stats = fc.expected(case, "checker")
    assert stats["cls0"] and stats["cls1"] and stats["cls2"]
    for k in range(len(want)):
        m = kinds[k][0] == fr.INTERP
        assert want[k][0][m].min() < 0 and want[k][0][m].max() > 1, k


def _index_planes(case):
    return [np.arange(h * w, dtype=np.uint16).reshape(h, w) for h, w in dc.planes_shape(case)]


COPY_CASES = [c for c in ALL if c["blur"] == 0 or c["sub"] > 0]


@pytest.mark.parametrize("case", COPY_CASES, ids=dc.ids(COPY_CASES))
def test_special_values_pass_through_every_copy_path_bit_for_bit(case):
    """where a copy comes from is read off the integer restatement run on a plane that holds its own indices (206 x 118 < 65536)"""
    src, want, kinds, _ = fc.expected(case, "special")
    idx = _index_planes(case)
    f = dc.FORMATS[case["fmt"]]
    seen = copies = 0
    for k, t in enumerate(case["trs"]):
        for p, (tp, blur) in enumerate(dr.plane_transforms(t, f["subsampling"], f.get("gray", False), case["blur"])):
            at = dr.compensate_plane(idx[p], tp, case["sub"], case["mirror"], 0, 0, 65535, "library")
            m = kinds[k][p] == fr.COPY
            if blur:                                                   # with blur the mirrored columns are runs, not copies, in both
                at2 = dr.compensate_plane(idx[p], tp, case["sub"], case["mirror"], 0, blur, 65535, "library")
                assert np.array_equal(at[m], at2[m])
            assert np.array_equal(want[k][p].view(u32)[m], src[p].view(u32).ravel()[at[m]]), (k, p)
            seen += int(np.isin(want[k][p].view(u32)[m], fc.SPECIALS).sum())
            copies += int(m.sum())
    assert seen * 10 >= copies - 20, (seen, copies)                    # three samples in ten of the clip are special values


@pytest.mark.parametrize("case", [c for c in STAB if c["name"].startswith(("combos_s", "mirror15", "small_s"))], ids=lambda c: c["name"])
def test_a_negative_current_frame_is_never_overpainted(case):
    """the current frame in [-3, -2), next and prev in [1, 2).  Where the current frame's pass covers a sample -- by the integer restatement,
    which says so through two border values -- the result is negative; everywhere else it is not."""
    rng = np.random.default_rng(7)
    shapes = dc.planes_shape(case)
    frames = [[(rng.random(s, dtype=f32) + f32(o)).astype(f32) for s in shapes] for o in (-3, 1, 1)]
    _, want, who, _ = fc.stab_expected(case, src=frames)
    f = dc.FORMATS[case["fmt"]]
    any8 = [np.zeros(s, np.uint8) for s in shapes]
    n = 0
    for k, (cur, nxt, prev) in enumerate(case["jobs"]):
        if (nxt is not None and nxt[0] == 0) or (prev is not None and prev[0] == 0):
            continue                                                   # a fill source that is the current frame itself
        first = nxt is None and prev is None
        for p, (tp, blur) in enumerate(dr.plane_transforms(cur, f["subsampling"], f.get("gray", False), case["blur"])):
            m = case["mirror"] if first else 0
            covered = dr.compensate_plane(any8[p], tp, case["sub"], m, 0, blur, 255, "library") == dr.compensate_plane(any8[p], tp, case["sub"], m, 255, blur, 255, "library")
            assert np.all(want[k][p][covered] < 0), (k, p)
            assert np.all(want[k][p][~covered] >= 0), (k, p)
            assert np.array_equal(who[k][p] == fr.CUR, covered | (first & ~covered))
            n += int(covered.sum())
    assert n > 1000


# ------------------------------------------------------------------------------------------------ the rule compiled for the host

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vapoursynth-mvtools_amd", "csrc")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("depan_float_emu") / "libdepan_float_emu.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I" + CSRC, os.path.join(HERE, "depan_float_emu.cpp"), "-o", so])
    return C.CDLL(so)


def _emu_plane(emu, s, sub, mirror, chroma, blur, tp):
    s = np.ascontiguousarray(s)
    h, w = s.shape
    pitch = w * 4 + 8
    buf = np.full((h + 2, pitch), 0xA5, np.uint8)
    tt = np.ascontiguousarray(tp, dtype=f32)
    emu.depan_float_emu_plane(C.c_void_p(s.ctypes.data), C.c_longlong(w * 4), w, h, sub, mirror, int(chroma), blur, C.c_void_p(tt.ctypes.data),
                              C.c_void_p(buf[1:].ctypes.data), C.c_longlong(pitch))
    assert np.all(buf[0] == 0xA5) and np.all(buf[-1] == 0xA5) and np.all(buf[1:-1, w * 4:] == 0xA5)
    return np.ascontiguousarray(buf[1:-1, :w * 4]).view(f32)


@pytest.mark.parametrize("kind", ["noise", "int8"])
@pytest.mark.parametrize("case", ALL, ids=dc.ids(ALL))
def test_the_kernel_text_on_the_host_equals_the_restatement(emu, case, kind):
    """every sample of every plane as uint32, with a 0xA5 canary around a destination whose pitch is wider than its rows"""
    src, want, _, _ = fc.expected(case, kind)
    f = dc.FORMATS[case["fmt"]]
    for k, t in enumerate(case["trs"]):
        for p, (tp, blur) in enumerate(dr.plane_transforms(t, f["subsampling"], f.get("gray", False), case["blur"])):
            got = _emu_plane(emu, src[p], case["sub"], case["mirror"], p > 0, blur, tp)
            assert fc.same_bits(got, want[k][p]), (k, p, fc.first_diff(got, want[k][p]))


@pytest.mark.parametrize("case", COPY_CASES, ids=dc.ids(COPY_CASES))
def test_the_kernel_text_on_special_values(emu, case):
    """copies bit for bit; a computed sample may be a NaN of another payload (which NaN an arithmetic ends on is the build's), else equal"""
    src, want, kinds, _ = fc.expected(case, "special")
    f = dc.FORMATS[case["fmt"]]
    for k, t in enumerate(case["trs"]):
        for p, (tp, blur) in enumerate(dr.plane_transforms(t, f["subsampling"], f.get("gray", False), case["blur"])):
            got = _emu_plane(emu, src[p], case["sub"], case["mirror"], p > 0, blur, tp)
            copied = (kinds[k][p] == fr.COPY) | (kinds[k][p] == fr.BORDER)
            assert np.array_equal(got.view(u32)[copied], want[k][p].view(u32)[copied]), (k, p)
            g, w = got[~copied], want[k][p][~copied]
            assert np.all((g.view(u32) == w.view(u32)) | (np.isnan(g) & np.isnan(w))), (k, p)


@pytest.mark.parametrize("case", STAB, ids=sc.ids(STAB))
def test_the_selection_on_the_host_equals_the_sequential_paint(emu, case):
    frames, want, _, _ = fc.stab_expected(case, "noise")
    f = dc.FORMATS[case["fmt"]]
    ssw, ssh = (0, 0) if f.get("gray") else f["subsampling"]
    for k, (cur, nxt, prev) in enumerate(case["jobs"]):
        trs = np.zeros(18, f32)
        trs[0:6] = cur
        if nxt is not None:
            trs[6:12] = nxt[1]
        if prev is not None:
            trs[12:18] = prev[1]
        for p in range(len(want[k])):
            blur = dr.plane_transforms(cur, f["subsampling"], f.get("gray", False), case["blur"])[p][1]
            planes = [np.ascontiguousarray(frames[0][p]), None if nxt is None else np.ascontiguousarray(frames[nxt[0]][p]),
                      None if prev is None else np.ascontiguousarray(frames[prev[0]][p])]
            h, w = planes[0].shape
            ptrs = (C.c_void_p * 3)(*[None if s is None else s.ctypes.data for s in planes])
            pitch = w * 4 + 8
            buf = np.full((h + 2, pitch), 0xA5, np.uint8)
            emu.depan_float_stab_emu_plane(ptrs, C.c_longlong(w * 4), w, h, case["sub"], case["mirror"], blur, ssw, ssh, p, C.c_void_p(trs.ctypes.data),
                                           C.c_void_p(buf[1:].ctypes.data), C.c_longlong(pitch))
            got = np.ascontiguousarray(buf[1:-1, :w * 4]).view(f32)
            assert fc.same_bits(got, want[k][p]), (k, p, fc.first_diff(got, want[k][p]))
            assert np.all(buf[0] == 0xA5) and np.all(buf[-1] == 0xA5) and np.all(buf[1:-1, w * 4:] == 0xA5)


def test_the_kernel_text_under_the_sanitizers_on_the_library_cases(tmp_path):
    """the out-of-domain cases (wide mirrored shifts, NaN / 3e9 transforms, bilinear's tail) are where an index could leave a plane: the same
    text as a stand-alone program under AddressSanitizer and UBSan, on heap planes of exactly the plane's size"""
    one = tmp_path / "one.cpp"
    one.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]
    if not shutil.which("g++") or subprocess.run(["g++"] + flags + [str(one), "-o", str(tmp_path / "one")], capture_output=True).returncode or \
            subprocess.run([str(tmp_path / "one")]).returncode:
        pytest.skip("g++ does not link -fsanitize=address,undefined here")
    exe = str(tmp_path / "depan_float_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DDEPAN_EMU_MAIN"] + flags + ["-I" + CSRC, os.path.join(HERE, "depan_float_emu.cpp"), "-o", exe])
    runs = 0
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for case in dc.LIBRARY_CASES + [c for c in dc.CASES if c["name"] in ("small_s0_8", "small_s1_16", "small_s2_8", "gray_s2", "f444_s1")]:
        src, want, _, _ = fc.expected(case, "noise")
        f = dc.FORMATS[case["fmt"]]
        for k, t in enumerate(case["trs"]):
            for p, (tp, blur) in enumerate(dr.plane_transforms(t, f["subsampling"], f.get("gray", False), case["blur"])[:2]):
                h, w = src[p].shape
                with open(fin, "wb") as fh:
                    fh.write(struct.pack("<6i", w, h, case["sub"], case["mirror"], int(p > 0), blur))
                    fh.write(np.ascontiguousarray(tp, dtype=f32).tobytes())
                    fh.write(np.ascontiguousarray(src[p]).tobytes())
                r = subprocess.run([exe, "compensate", fin, fout], capture_output=True, text=True)
                assert r.returncode == 0, (case["name"], k, p, r.stderr[-2000:])
                got = np.fromfile(fout, dtype=f32).reshape(h, w)
                assert fc.same_bits(got, want[k][p]), (case["name"], k, p)
                runs += 1
    for case in [c for c in STAB if c["name"] in ("undef_s0", "undef_s1", "undef_s2", "small_s2_8", "self_s1")]:
        frames, want, _, _ = fc.stab_expected(case, "noise")
        f = dc.FORMATS[case["fmt"]]
        for k, (cur, nxt, prev) in enumerate(case["jobs"]):
            for p in range(2):
                blur = dr.plane_transforms(cur, f["subsampling"], f.get("gray", False), case["blur"])[p][1]
                h, w = frames[0][p].shape
                with open(fin, "wb") as fh:
                    fh.write(struct.pack("<10i", w, h, case["sub"], case["mirror"], blur, f["subsampling"][0], f["subsampling"][1], p, nxt is not None, prev is not None))
                    fh.write(np.concatenate([cur, np.zeros(6, f32) if nxt is None else nxt[1], np.zeros(6, f32) if prev is None else prev[1]]).astype(f32).tobytes())
                    for s in (frames[0], None if nxt is None else frames[nxt[0]], None if prev is None else frames[prev[0]]):
                        if s is not None:
                            fh.write(np.ascontiguousarray(s[p]).tobytes())
                r = subprocess.run([exe, "plane", fin, fout], capture_output=True, text=True)
                assert r.returncode == 0, (case["name"], k, p, r.stderr[-2000:])
                assert fc.same_bits(np.fromfile(fout, dtype=f32).reshape(h, w), want[k][p]), (case["name"], k, p)
                runs += 1
    assert runs > 150
