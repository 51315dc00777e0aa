"""CPU tests of the float entries (mvx_super_create_float, mvx_degrain_n_create_float; no create touches a device): their messages and the order
of the checks, the refusal of a float super clip by every other entry that takes a super clip, the geometry of the float super clip against the
integer create's at levels=1, what the integer creates still say about 17 and 32 bits, and csrc/mvx_super_float_rule.h as a stand-alone host
program (with AddressSanitizer and UBSan where g++ links them) against tests/super_float_ref.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import super_float_ref as sf
from test_block_host import PITCH, _clips, _copy, _err

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vapoursynth-mvtools_amd", "csrc")
FORMAT = "Super: input clip must be GRAY, 420, 422, 440, or 444, up to 16 bits, with constant dimensions."
FPITCH = [1280, 768, 768]  # rows of 320 / 160 float samples, rounded up to 256 bytes


def _fsup(mv, w=320, h=192, **kw):
    return mv.Super(w, h, 32, sample_float=True, **kw)


# ------------------------------------------------------------------------------------------------ Super

def test_float_super_messages_and_their_order(mv):
    for bits in (8, 16, 31, 33):
        assert _err(lambda: mv.Super(320, 192, bits, sample_float=True)) == "Super: a float clip has 32 bits per sample."
    one = "Super: a float super clip has one level (levels=1)."
    for levels in (0, 2, 3, -1):
        assert _err(lambda: _fsup(mv, levels=levels)) == one
    assert _fsup(mv, levels=1).info.levels == 1 and _fsup(mv).info.levels == 1
    # the two come first, then mvx_super_create's in its order
    assert _err(lambda: mv.Super(320, 192, 16, sample_float=True, pel=3, levels=2)) == "Super: a float clip has 32 bits per sample."
    assert _err(lambda: _fsup(mv, levels=2, pel=3)) == one
    assert _err(lambda: _fsup(mv, pel=3, sharp=5)) == "Super: pel must be 1, 2, or 4."
    assert _err(lambda: _fsup(mv, sharp=3, rfilter=9)) == "Super: sharp must be between 0 and 2 (inclusive)."
    assert _err(lambda: _fsup(mv, rfilter=5, hpad=-1)) == "Super: rfilter must be between 0 and 4 (inclusive)."
    assert _err(lambda: _fsup(mv, subsampling=(2, 1), hpad=-1)) == FORMAT
    assert _err(lambda: _fsup(mv, w=0)) == FORMAT
    assert _err(lambda: _fsup(mv, vpad=-1)) == "Super: hpad and vpad must not be negative."
    for rf in range(5):
        assert _fsup(mv, rfilter=rf).info.rfilter == rf


def test_integer_creates_keep_their_message_for_17_and_32_bits(mv):
    for bits in (17, 32, 7):
        assert _err(lambda: mv.Super(320, 192, bits)) == FORMAT
        assert _err(lambda: mv.Super(320, 192, bits, levels=1)) == FORMAT


GEOMETRIES = [dict(), dict(pel=1), dict(pel=4, sharp=0), dict(hpad=8, vpad=4), dict(hpad=0, vpad=0, gray=True), dict(subsampling=(0, 0), pel=4),
              dict(subsampling=(1, 0), hpad=5, vpad=3), dict(chroma=0), dict(hpad=3, vpad=5, pel=1)]


@pytest.mark.parametrize("kw", GEOMETRIES, ids=lambda k: ",".join("%s=%s" % kv for kv in sorted(k.items())) or "defaults")
@pytest.mark.parametrize("size", [(320, 192), (70, 54), (36, 36)])
def test_info_is_the_integer_creates_at_one_level_except_bits(mv, size, kw):
    f, i = _fsup(mv, *size, **kw), mv.Super(size[0], size[1], 16, levels=1, **kw)
    for name, _ in mv.SuperInfo._fields_:
        a, b = getattr(f.info, name), getattr(i.info, name)
        a, b = (list(a), list(b)) if hasattr(a, "__len__") else (a, b)
        assert (a, b) == ((32, 16) if name == "bits" else (b, b)), name
    assert f.is_float and not i.is_float and mv.lib().mvx_super_is_float(f.h) == 1 and mv.lib().mvx_super_is_float(i.h) == 0
    assert f.dtype == np.float32 and f.bps == 4 and not f.shadow
    assert f.pitch == [(f.info.plane_width[p] * 4 + 255) // 256 * 256 for p in range(f.nplanes)]
    planes, shapes = sf.geometry(size[0], size[1], kw.get("subsampling", (1, 1)), kw.get("gray", False), f.info.hpad, f.info.vpad, f.info.pel)
    assert shapes == [(f.info.plane_height[p], f.info.plane_width[p]) for p in range(f.nplanes)]


def test_shadow_pelclip_and_finest_entries_refuse_a_float_super(mv):
    f, L = _fsup(mv), mv.lib()
    assert L.mvx_super_shadow_copies(f.h) == 0
    extra, three = (C.c_size_t * 3)(7, 7, 7), (C.c_ssize_t * 3)(*f.pitch)
    L.mvx_super_shadow_bytes(f.h, three, extra)
    assert list(extra) == [0, 0, 0]
    none = (C.c_void_p * 3)()
    assert L.mvx_super_shadow_frames(f.h, 1, none, three, three, None) == -1
    assert L.mvx_last_error().decode() == "mvx_super_shadow_frames: float super clips are not supported."
    assert _err(lambda: f.pelclip_mode(640, 384)) == "Super: float super clips take no pelclip."
    assert L.mvx_super_frames_pelclip(f.h, 1, none, three, none, three, 1, none, three, None) == -1
    L.mvx_finest_frames.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_ssize_t), C.POINTER(C.c_void_p), C.POINTER(C.c_ssize_t), C.c_void_p]
    assert L.mvx_finest_frames(f.h, 1, none, three, none, three, None) == -1
    assert L.mvx_last_error().decode() == "Finest: float super clips are not supported."


def _refusals():
    return {
        "Analyse": lambda mv, s, bw, fw: mv.Analyse(s, isb=1, blksize=99),
        "AnalyseN": lambda mv, s, bw, fw: mv.AnalyseN(s, 99),
        "Recalculate": lambda mv, s, bw, fw: mv.Recalculate(s, bw, blksize=99),
        "RecalculateN": lambda mv, s, bw, fw: mv.RecalculateN(s, _copy(mv, bw, nDeltaFrame=3), 99),
        "Degrain": lambda mv, s, bw, fw: mv.Degrain(9, s, bw, PITCH),
        "DegrainN": lambda mv, s, bw, fw: _dn_raw(mv, "mvx_degrain_n_create", s, bw, radius=99),
        "DegrainN-out16": lambda mv, s, bw, fw: _dn_raw(mv, "mvx_degrain_n_create_out16", s, bw, radius=99),
        "Compensate": lambda mv, s, bw, fw: mv.Compensate(s, bw, time=500.0),
        "CompensateN": lambda mv, s, bw, fw: mv.CompensateN(99, s, bw, time=500.0),
        "BlockFPS": lambda mv, s, bw, fw: mv.BlockFPS(s, bw, fw, 10, PITCH, mode=77),
        "FlowInter": lambda mv, s, bw, fw: mv.FlowInter(s, bw, fw, 10, PITCH, time=500.0),
        "FlowFPS": lambda mv, s, bw, fw: mv.FlowFPS(s, bw, fw, 10, PITCH, mask=9),
        "Flow": lambda mv, s, bw, fw: mv.Flow(s, bw, 10, PITCH, time=500.0),
        "FlowBlur": lambda mv, s, bw, fw: mv.FlowBlur(s, bw, fw, 10, PITCH, blur=900.0),
        "ScaleVect": lambda mv, s, bw, fw: mv.ScaleVect(bw, s, scale=3),
    }


def _dn_raw(mv, entry, sup, ad, radius=1, pitch=FPITCH, **kw):
    """a DegrainN create called by name (mv.DegrainN picks the float entry by the super clip); raises like the package"""
    f = dict(radius=radius, thsad=None, thsadc=None, thsad2=None, thsadc2=None, plane=None, limit=None, limitc=None, thscd1=None, thscd2=None)
    f.update(kw)
    a = mv.DegrainNArgs(*[mv.UNSET if v is None else int(v) for v in f.values()])
    h, err = C.c_void_p(), C.create_string_buffer(512)
    three = lambda l: (C.c_ssize_t * 3)(*l)
    rc = getattr(mv.lib(), entry)(C.byref(a), C.byref(_copy(mv, ad)), sup.h, three(pitch), three(sup.pitch), three(pitch), C.byref(h), err)
    if rc:
        assert not h.value
        raise mv.MvtoolsError(err.value.decode())
    bits = mv.lib().mvx_degrain_n_out_bits(h)
    mv.lib().mvx_degrain_n_destroy(h)
    return bits


@pytest.mark.parametrize("name", sorted(_refusals()))
def test_every_other_create_refuses_a_float_super_before_any_other_check(mv, name):
    """each call also carries an argument its entry would refuse first of all for an integer super clip"""
    _, bw, fw = _clips(mv)
    assert _err(lambda: _refusals()[name](mv, _fsup(mv), bw, fw)) == "%s: float super clips are not supported." % name.split("-")[0]


# ------------------------------------------------------------------------------------------------ DegrainN

def test_float_degrain_n_messages_and_their_order(mv):
    isup, bw, _ = _clips(mv)
    fsup = _fsup(mv)
    dn = lambda **kw: mv.DegrainN(kw.pop("radius", 1), kw.pop("sup", fsup), kw.pop("ad", bw), FPITCH, **kw)
    needs = "DegrainN: the float entry needs a float super clip."
    assert _err(lambda: dn(radius=0, plane=9)) == "DegrainN: radius must be between 1 and 24."
    assert _err(lambda: dn(radius=25)) == "DegrainN: radius must be between 1 and 24."
    assert _err(lambda: dn(plane=5, thscd1=99999)) == "DegrainN: plane must be between 0 and 4 (inclusive)."
    assert _err(lambda: dn(thscd1=16321, thsad=1 << 40)) == "DegrainN: thscd1 can be at most 16320."
    assert _err(lambda: dn(thsad=1 << 40)).startswith("DegrainN: with this block size and video format, thsad must")
    assert _err(lambda: dn(radius=3, thsad2=1 << 40)).startswith("DegrainN: with this block size and video format, thsad2 must")
    assert _err(lambda: dn(sup=_fsup(mv, w=336), limit=999)) == "DegrainN: wrong source or super clip frame size."
    assert _err(lambda: dn(sup=_fsup(mv, pel=4))) == "DegrainN: wrong source or super clip frame size."
    # the float entry with an integer super clip: after the frame size, before the limits
    assert _err(lambda: _dn_raw(mv, "mvx_degrain_n_create_float", isup, bw, limit=999)) == needs
    assert _err(lambda: _dn_raw(mv, "mvx_degrain_n_create_float", mv.Super(336, 192, 8), bw)) == "DegrainN: wrong source or super clip frame size."
    sup16, bw16, _ = _clips(mv, bits=16)
    assert _err(lambda: _dn_raw(mv, "mvx_degrain_n_create_float", sup16, bw16)) == needs
    # limits on the 8-bit scale whatever the depth of the search
    limit, limitc = "DegrainN: limit must be between 0 and 255 (inclusive).", "DegrainN: limitc must be between 0 and 255 (inclusive)."
    for ad in (bw, bw16):
        assert _err(lambda: dn(ad=ad, limit=256)) == limit
        assert _err(lambda: dn(ad=ad, limit=-1, limitc=999)) == limit
        assert _err(lambda: dn(ad=ad, limitc=256)) == limitc
        assert _err(lambda: dn(ad=ad, limit=10, limitc=-1)) == limitc
        dn(ad=ad, limit=255, limitc=0)
        dn(ad=ad, limit=0)
    supo, bwo, _ = _clips(mv, overlap=4)
    assert _err(lambda: dn(ad=_copy(mv, bwo, nBlkX=2))) == "overlap needs at least 3x3 blocks (window selection divides by nBlk-2)."
    assert _err(lambda: dn(out16=True)) == "DegrainN: float super clips are not supported."   # (the out16 entry's refusal)


@pytest.mark.parametrize("bits", [8, 10, 16])
def test_out_bits_and_the_threshold_tables_are_the_searchs(mv, bits):
    isup, bw, _ = _clips(mv, bits=bits, blksize=16, overlap=8)
    fsup = _fsup(mv)
    kw = dict(thsad=1200, thsadc=777, thsad2=301, thsadc2=50, thscd1=300)
    new, old = mv.DegrainN(7, fsup, bw, FPITCH, **kw), mv.DegrainN(7, isup, bw, [640, 320, 320], **kw)
    assert new.is_float and not old.is_float and (new.out_bits, old.out_bits) == (32, bits)
    assert new.info() == old.info() and new.info()["thsad_d"][0] > new.info()["thsad_d"][-1]
    assert new.dst_pitch == FPITCH
    assert _dn_raw(mv, "mvx_degrain_n_create_float", fsup, bw) == 32


# ------------------------------------------------------------------------------------------------ the rule header on the host

def _sanitizer_flags(tmp):
    src = os.path.join(tmp, "one.cpp")
    open(src, "w").write("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(["g++"] + flags + [src, "-o", os.path.join(tmp, "one")], capture_output=True)
    return flags if r.returncode == 0 and subprocess.run([os.path.join(tmp, "one")]).returncode == 0 else []


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    assert shutil.which("g++"), "the host program needs g++"
    tmp = str(tmp_path_factory.mktemp("float_rule"))
    exe = os.path.join(tmp, "float_rule_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + CSRC, os.path.join(HERE, "float_rule_host_main.cpp"), "-o", exe]
                          + _sanitizer_flags(tmp))
    return exe


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 37])
@pytest.mark.parametrize("sharp", [0, 1, 2])
def test_rule_header_on_the_host_is_the_restatement(rule_exe, sharp, n):
    """64 random rows per sharp and length: luma-like, chroma-like (negative) and overshooting values; short rows take the border rules only"""
    rows = 64
    rng = np.random.default_rng(100 * sharp + n)
    a = (rng.random((rows, n)) * 1.5 - 0.2).astype(np.float32)
    a[::3] -= np.float32(0.5)
    r = subprocess.run([rule_exe, str(sharp), str(rows), str(n)], input=a.tobytes(), capture_output=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()
    out = np.frombuffer(r.stdout, np.float32).reshape(3, rows, n)
    assert np.array_equal(out[0], sf.half_rows(a, sharp))
    assert np.array_equal(out[1], sf.diagonal(a))
    assert np.array_equal(out[2], (np.roll(a, -1, axis=0) + a) * np.float32(0.5))


# ------------------------------------------------------------------------------------------------ plane layouts of the float entries

def test_float_degrain_n_planes_and_pitches_are_multiples_of_4(mv):
    """include/mvtools_amd.h, mvx_degrain_n_create_float: "Planes and pitches must be multiples of 4 bytes" -- the clip-side contract of the block
    filters at a sample size of 4; refused with MVX_E_ARG at creation (pitches) and at the head of mvx_degrain_n_frames (addresses)"""
    _, bw, _ = _clips(mv)
    fsup = _fsup(mv)
    w = fsup.info.width
    rows = [w * 4, w * 2, w * 2]
    msg = lambda what, p: "%s pitch of plane %d must hold a row of %d bytes and be a multiple of the sample size." % (what, p, rows[p])
    mv.DegrainN(1, fsup, bw, rows)                                    # tight
    mv.DegrainN(1, fsup, bw, [r + 4 for r in rows], rows)             # one sample more
    mv.DegrainN(1, fsup, bw, [rows[0], rows[1], rows[2] + 256], rows)  # U != V
    assert _err(lambda: mv.DegrainN(1, fsup, bw, [rows[0] + 2, rows[1], rows[2]])) == msg("src", 0)
    assert _err(lambda: mv.DegrainN(1, fsup, bw, rows, [rows[0], rows[1] + 2, rows[2]])) == msg("dst", 1)
    assert _err(lambda: mv.DegrainN(1, fsup, bw, [rows[0] - 4, rows[1], rows[2]])) == msg("src", 0)
    dn = mv.DegrainN(1, fsup, bw, rows)
    L, A = mv.lib(), 0x10000  # never dereferenced
    job = (mv.DegrainNJob * 1)()
    refs, blobs = ((C.c_void_p * 3) * 2)(), (C.c_void_p * 2)()
    job[0].refs = C.cast(refs, C.POINTER(C.c_void_p * 3))
    job[0].blobs = C.cast(blobs, C.POINTER(C.c_void_p))
    for src, dst, ref, want in (((A + 2, A, A), (A, A, A), A, "mvx_degrain_n_frames: src plane 0 must be aligned to 4 bytes"),
                                ((A, A, A), (A, A + 2, A), A, "mvx_degrain_n_frames: dst plane 1 must be aligned to 4 bytes"),
                                ((A, A, A), (A, A, None), A, "mvx_degrain_n_frames: dst plane 2 is required"),
                                ((A, A, A), (A, A, A), A + 4, "mvx_degrain_n_frames: reference super plane 0 must be aligned to 16 bytes")):
        for p in range(3):
            job[0].src[p], job[0].dst[p], refs[0][p] = src[p], dst[p], ref
        assert L.mvx_degrain_n_frames(dn.h, 1, job, None) == -1 and L.mvx_last_error().decode() == want
