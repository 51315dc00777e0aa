"""CPU tests of mv.DepanCompensate and mv.DepanAnalyse: creation (no device is touched) with the reference's checks and messages in its order
(MVDepan.cpp:473-615, :2750-2881) and the library's own rejections; the struct layouts against the C header; intoffset and the frame map;
mvx_depan_motion_to_transform and the host estimator mvx_depan_analyse_host bit for bit against the restatement tests/depan_ref.py, on
vectors from the oracle's Analyse and on crafted fields that are held to what they claim; and, where the toolchain links the sanitizers,
the estimator's header in a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import depan_ref as dr
import pipeline as pl
import vector_fields as vf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
f32 = np.float32


def _err(call):
    import mvtools_amd
    with pytest.raises(mvtools_amd.MvtoolsError) as e:
        call()
    return str(e.value)


def _ad(mv, w=320, h=192, bits=8, **akw):
    return mv.Analyse(mv.Super(w, h, bits), **dict(dict(isb=0, delta=1), **akw)).ad


FORMAT = ("DepanCompensate: clip must have constant format and dimensions, integer sample type, bit depth up to 16, and it must be Gray, 420, 422, or 444, "
          "and not RGB.")
SMALL = "DepanCompensate: every plane must be at least 2 samples wide and 2 high, and the frame at most 32767 x 32767."
MASK = "DepanStabilise: mask must have constant format, the same dimensions as clip, and no more than 8 bits per sample."


def test_compensate_argument_checks_in_the_reference_order(mv):
    c = lambda **kw: mv.DepanCompensate(kw.pop("w", 320), kw.pop("h", 192), **kw)
    assert _err(lambda: c(offset=10.5)) == "DepanCompensate: offset must be between -10.0 and 10.0 (inclusive)."
    assert _err(lambda: c(offset=-10.5)) == "DepanCompensate: offset must be between -10.0 and 10.0 (inclusive)."
    assert _err(lambda: c(subpixel=3)) == "DepanCompensate: subpixel must be between 0 and 2 (inclusive)."
    assert _err(lambda: c(subpixel=-1)) == "DepanCompensate: subpixel must be between 0 and 2 (inclusive)."
    assert _err(lambda: c(pixaspect=0.0)) == "DepanCompensate: pixaspect must be greater than 0."
    assert _err(lambda: c(mirror=16)) == "DepanCompensate: mirror must be between 0 and 15 (inclusive)."
    assert _err(lambda: c(mirror=-1)) == "DepanCompensate: mirror must be between 0 and 15 (inclusive)."
    assert _err(lambda: c(blur=-1)) == "DepanCompensate: blur must not be negative."
    assert _err(lambda: c(bits=17)) == FORMAT
    assert _err(lambda: c(subsampling=(2, 1))) == FORMAT
    assert _err(lambda: c(subsampling=(0, 1))) == FORMAT           # 4:4:0
    assert _err(lambda: c(num_frames=10, data_frames=9)) == "DepanCompensate: data must have at least as many frames as clip."
    # the order
    assert _err(lambda: c(offset=11, subpixel=5, pixaspect=-1, mirror=99, blur=-2, bits=32)).startswith("DepanCompensate: offset")
    assert _err(lambda: c(subpixel=5, pixaspect=-1, mirror=99, blur=-2, bits=32)).startswith("DepanCompensate: subpixel")
    assert _err(lambda: c(pixaspect=-1, mirror=99, blur=-2, bits=32)).startswith("DepanCompensate: pixaspect")
    assert _err(lambda: c(mirror=99, blur=-2, bits=32)).startswith("DepanCompensate: mirror")
    assert _err(lambda: c(blur=-2, bits=32)).startswith("DepanCompensate: blur")
    assert _err(lambda: c(bits=32, num_frames=5, data_frames=1)) == FORMAT
    # the limits are accepted, and every format the reference takes
    c(offset=10.0, subpixel=0, mirror=15, blur=0)
    c(offset=-10.0, subpixel=2, mirror=0, blur=1000)
    for kw in (dict(gray=True, subsampling=(0, 0)), dict(subsampling=(1, 1)), dict(subsampling=(1, 0)), dict(subsampling=(0, 0))):
        for bits in (8, 10, 16):
            c(bits=bits, **kw)
    # the library's own rejections
    assert _err(lambda: c(w=2, h=192)) == SMALL                    # 4:2:0 chroma would be one column
    assert _err(lambda: c(w=320, h=3)) == SMALL
    assert _err(lambda: c(w=32768, h=192)) == SMALL
    c(w=4, h=4)
    c(w=2, h=2, subsampling=(0, 0))
    assert _err(lambda: c(bits=16, dst_pitch=[320, 160, 160])).startswith("DepanCompensate: pitches")


def test_compensate_defaults_and_derived_values(mv):
    g = mv.DepanCompensate(206, 118, bits=10, subsampling=(1, 0), offset=1.0, blur=7)
    i = g.info
    assert (i.subpixel, i.mirror, i.intoffset, i.pixel_max, i.num_planes) == (2, 0, 1, 1023, 3)
    assert list(i.plane_width) == [206, 103, 103] and list(i.plane_height) == [118, 118, 118]
    assert list(i.border) == [0, 512, 512] and list(i.blur) == [7, 3, 3]
    assert (i.xcenter, i.ycenter) == (103.0, 59.0)
    g = mv.DepanCompensate(206, 118, subsampling=(0, 0), offset=1.0, blur=7)
    assert list(g.info.blur) == [7, 7, 7] and list(g.info.border) == [0, 128, 128]
    assert mv.DepanCompensate(206, 118, gray=True, offset=1.0).info.num_planes == 1


def test_analyse_argument_checks_in_the_reference_order(mv):
    ad = _ad(mv)
    a = lambda **kw: mv.DepanAnalyse(kw.pop("ad", ad), 320, 192, **kw)
    assert _err(lambda: a(pixaspect=0.0)) == "DepanAnalyse: pixaspect must be positive."
    assert _err(lambda: a(num_frames=10, vector_frames=9)) == "DepanAnalyse: vectors must have at least as many frames as clip."
    assert _err(lambda: a(mask=(8,), num_frames=10, mask_frames=9)) == "DepanStabilise: mask must have at least as many frames as clip."
    assert _err(lambda: a(mask=(9,))) == MASK
    assert _err(lambda: a(mask=(8, 336, 192))) == MASK
    assert _err(lambda: a(mask=(8, 320, 200))) == MASK
    assert _err(lambda: a(thscd1=16321)) == "DepanAnalyse: thscd1 can be at most 16320."
    ad2 = _ad(mv, delta=2)
    assert _err(lambda: a(ad=ad2)) == "DepanAnalyse: vectors clip must be created with delta=1."
    # the delta message replaces the one of scaleThSCD (:577-580)
    assert _err(lambda: a(ad=ad2, thscd1=99999)) == "DepanAnalyse: vectors clip must be created with delta=1."
    assert _err(lambda: a(pixaspect=-1.0, num_frames=10, vector_frames=1, mask=(16,), thscd1=99999)).startswith("DepanAnalyse: pixaspect")
    assert _err(lambda: a(num_frames=10, vector_frames=1, mask=(16,), thscd1=99999)).startswith("DepanAnalyse: vectors must")
    assert _err(lambda: a(mask=(16,), thscd1=99999)) == MASK
    a(mask=(8,), thscd1=16320, zoom=0, rot=0, fields=1)


def test_struct_layouts_match_the_header(mv, tmp_path):
    names = ["mvx_depan_clip", "mvx_depan_compensate_args", "mvx_depan_compensate_info", "mvx_depan_compensate_job", "mvx_depan_analyse_args", "mvx_depan_motion"]
    py = [mv.DepanClip, mv.DepanCompensateArgs, mv.DepanCompensateInfo, mv.DepanCompensateJob, mv.DepanAnalyseArgs, mv.DepanMotion]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mvtools_amd.h"', 'int main(void) {']
    for n, t in zip(names, py):
        lines.append('printf("%%zu", sizeof(%s));' % n)
        for f in t._fields_:
            lines.append('printf(" %%zu", offsetof(%s, %s));' % (n, f[0]))
        lines.append('printf("\\n");')
    lines += ["return 0;", "}"]
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.check_output([exe]).decode().split("\n")
    for line, t in zip(out, py):
        want = [C.sizeof(t)] + [getattr(t, f[0]).offset for f in t._fields_]
        assert [int(v) for v in line.split()] == want, t.__name__


@pytest.mark.parametrize("offset,io", [(-10, -10), (-1.5, -2), (-1, -1), (-0.5, -1), (0, 0), (0.5, 1), (1, 1), (10, 10)])
def test_intoffset_and_map_at_both_clip_ends(mv, offset, io):
    nf = 12
    g = mv.DepanCompensate(64, 48, offset=offset, num_frames=nf)
    assert g.info.intoffset == io == dr.intoffset_of(offset)
    for n in (0, 1, 2, 9, 10, 11):
        want = dr.frame_map(offset, n, nf)
        assert g.map(n) == want
        if io == 0 or not 0 <= n - io <= nf - 1:
            assert want is None
        else:
            assert want == (n - io, min(n, n - io), max(n, n - io))


MOTIONS = [(1.25, -0.75, 1.001, 0.2), (-3.0, 2.0, 0.998, -0.35), (0.011, 0.5, 1.0, 0.0), (2.5, 2.5, 1.0000001, 0.00001), (7.0, -4.0, 1.01, 1.5)]


@pytest.mark.parametrize("offset", [1.0, -1.0, 0.5, -0.5, 1.5, -2.5, 3.0, -3.0])
@pytest.mark.parametrize("fmt", [dict(), dict(fields=1), dict(fields=1, tff=1), dict(fields=1, tff=0), dict(fields=1, matchfields=0), dict(pixaspect=1.0940)])
def test_motion_to_transform_equals_the_restatement(mv, offset, fmt):
    w, h = 206, 118
    g = mv.DepanCompensate(w, h, offset=offset, **fmt)
    count = abs(g.info.intoffset)
    for first in range(len(MOTIONS)):
        ms = [MOTIONS[(first + k) % len(MOTIONS)] for k in range(count)]
        for bad in (None, count // 2):
            if bad is not None:
                ms = list(ms)
                ms[bad] = (0.0,) + ms[bad][1:]                     # MOTIONBAD in mid-chain resets the sum
            for top in (0, 1):
                for ndest in (4, 5):
                    got_tr, got_mo = g.transform(ms, top_field=top, ndest=ndest)
                    want_tr, want_mo = dr.motion_to_transform(ms, offset, w, h, fmt.get("pixaspect", 1.0), bool(fmt.get("fields")), bool(fmt.get("matchfields", 1)),
                                                              top, fmt.get("tff"), ndest)
                    assert got_tr.tobytes() == want_tr.tobytes(), (ms, got_tr, want_tr)
                    assert got_mo.tobytes() == want_mo.tobytes(), (ms, got_mo, want_mo)
                    if bad is not None and not (fmt.get("fields") and fmt.get("matchfields", 1)):
                        assert got_tr.tolist() == [0, 1, 0, 0, 0, 1]


def test_the_snapping_of_rot_and_zoom_and_the_missing_field_property(mv):
    g = mv.DepanCompensate(206, 118, offset=1.0)
    tr, _ = g.transform([(2.5, 1.5, 1.0 + 5e-7, 5e-5)])              # |rotradian| < 1e-6 and |zoom - 1| < 1e-6: a pure translation
    assert tr.tolist() == [2.5, 1.0, 0.0, 1.5, 0.0, 1.0]
    assert tr.tobytes() == dr.motion_to_transform([(2.5, 1.5, 1.0 + 5e-7, 5e-5)], 1.0, 206, 118)[0].tobytes()
    tr, _ = g.transform([(2.5, 1.5, 1.0 + 3e-6, 1e-3)])              # just outside: zoom and rotation stay
    assert tr[1] != 1.0 and tr[2] != 0.0
    g = mv.DepanCompensate(206, 118, offset=1.0, fields=1)
    assert _err(lambda: g.transform([MOTIONS[0]], top_field=None)) == "DepanCompensate: _Field property not found in input frame. Therefore, you must pass tff argument."
    mv.DepanCompensate(206, 118, offset=1.0, fields=1, tff=1).transform([MOTIONS[0]], top_field=None)


def test_chroma_transforms_of_420_and_422():
    t = np.array([3.5, 1.01, 0.02, -2.5, -0.02, 1.01], dtype=f32)
    p420 = dr.plane_transforms(t, (1, 1), False, 5)
    assert p420[1][0].tolist() == [f32(1.75), t[1], t[2], f32(-1.25), t[4], t[5]] and p420[1][1] == 2 and p420[0][1] == 5
    p422 = dr.plane_transforms(t, (1, 0), False, 5)
    assert p422[1][0].tolist() == [f32(1.75), t[1], t[2] / f32(2), t[3], t[4] * f32(2), t[5]] and p422[2][1] == 2
    assert dr.plane_transforms(t, (0, 0), False, 5)[1][0].tolist() == t.tolist() and dr.plane_transforms(t, (0, 0), False, 5)[1][1] == 5
    assert len(dr.plane_transforms(t, (0, 0), True, 5)) == 1


# ------------------------------------------------------------------------------------------------ the estimator

W, H = 206, 118


def _oracle_blobs(oracle, isb, motion=(3, -1), nf=4, blk=8, ov=4, clip="moving"):
    """vectors of the oracle's Analyse on a clip with a planted pan: tests/pipeline.py's textured clip (pan `motion` per frame, noise, a
    rectangle moving the other way) or tests/synth.py's noisy checker (2 px per frame to the right)"""
    import synth
    frames = pl.moving_clip(W, H, 8, nf, seed=11, noise=2, motion=motion) if clip == "moving" else synth.survey_clip(W, H, 8, nf)
    sup = oracle.Super(W, H, 8)
    sfs = [sup.frame(f) for f in frames]
    an = oracle.Analyse(sup, num_frames=nf, blksize=blk, overlap=ov, isb=isb, delta=1)
    blobs = []
    for n in range(nf):
        k = n + 1 if isb else n - 1
        blobs.append(an.frame(sfs[n], sfs[k] if 0 <= k < nf else None))
    return an.ad, blobs


def _both(mv, ad, blobs, masks=None, top_field=None, **kw):
    """the library's host estimator and the restatement on the same blobs; asserts bit equality and returns the results and the counters"""
    _, s1, s2 = vf.scaled_thresholds(ad, 400, kw.get("thscd1", 400) if kw.get("thscd1") is not None else 400, kw.get("thscd2", 130) if kw.get("thscd2") is not None else 130)
    g = mv.DepanAnalyse(ad, W, H, mask=(8,) if masks is not None else None, **kw)
    got = g.run_host(blobs, masks, top_field)
    rkw = {k: v for k, v in kw.items() if k in ("zoom", "rot", "pixaspect", "error", "wrong", "zerow", "fields") and v is not None}
    ref = dr.Analyse(ad, W, H, s1, s2, has_mask=masks is not None, **rkw)
    stats = {}
    for n, b in enumerate(blobs):
        want = ref.frame(b, masks[n] if masks is not None else None, bool(top_field[n]) if top_field is not None else False, stats)
        for k in ("dx", "dy", "zoom", "rot", "error"):
            assert f32(got[n][k]).tobytes() == f32(want[k]).tobytes(), (n, k, got[n], want)
        assert got[n]["iter"] == want["iter"], (n, got[n], want)
    return got, stats


@pytest.mark.parametrize("isb", [0, 1])
def test_estimator_on_oracle_vectors_of_a_planted_pan(mv, oracle, isb):
    ad, blobs = _oracle_blobs(oracle, isb)
    got, stats = _both(mv, ad, blobs)
    assert stats.get("unusable") == 1                                   # the frame without a reference
    assert bool(stats.get("inverse")) == bool(isb)
    for m in (got[1], got[2]):
        assert abs(abs(m["dx"]) - 3) < 0.5 and abs(abs(m["dy"]) - 1) < 0.5 and abs(m["zoom"] - 1) < 0.01
    _both(mv, ad, blobs, fields=1, top_field=[0, 1, 0, 1])
    _both(mv, ad, blobs, zoom=0, rot=0, pixaspect=1.094)
    ad, blobs = _oracle_blobs(oracle, isb, clip="synth")
    got, stats = _both(mv, ad, blobs)
    for m in (got[1], got[2]):
        assert abs(abs(m["dx"]) - 2) < 0.5 and abs(m["dy"]) < 0.5, m


def _field(ad, fn):
    """a valid blob whose level-0 field is fn(bx, by) -> (x, y, sad) arrays, from an invalid oracle-shaped blob"""
    import mvtools_amd
    size = mvtools_amd.lib().mvx_vectors_size(C.byref(mvtools_amd.AnalysisData.from_buffer_copy(bytes(ad))))
    b = np.zeros(size, np.uint8)
    ints = b.view(np.int32)
    ints[0], ints[1] = size // 4, 1
    nwb = (ad.nBlkSizeX - ad.nOverlapX) * ad.nBlkX + ad.nOverlapX
    nhb = (ad.nBlkSizeY - ad.nOverlapY) * ad.nBlkY + ad.nOverlapY
    off = 8
    for i in range(ad.nLvCount - 1, -1, -1):
        bx = ((nwb >> i) - ad.nOverlapX) // (ad.nBlkSizeX - ad.nOverlapX)
        by = ((nhb >> i) - ad.nOverlapY) // (ad.nBlkSizeY - ad.nOverlapY)
        b[off:off + 4].view(np.int32)[0] = 4 + bx * by * 16
        off += 4 + bx * by * 16
    assert off == size
    xy, sad = vf.records(b, ad)
    gy, gx = np.mgrid[0:ad.nBlkY, 0:ad.nBlkX]
    x, y, s = fn(gx, gy)
    xy[:, :, 0], xy[:, :, 1], sad[:, :] = x, y, s
    return b


def _centres(ad, gx, gy):
    return gx * (ad.nBlkSizeX - ad.nOverlapX) + ad.nBlkSizeX // 2 - W / 2.0, gy * (ad.nBlkSizeY - ad.nOverlapY) + ad.nBlkSizeY // 2 - H / 2.0


@pytest.mark.parametrize("isb", [0, 1])
@pytest.mark.parametrize("pan", [(3, -2), (-5, 1), (0, 4)])
def test_a_planted_whole_pixel_pan_is_recovered(mv, oracle, isb, pan):
    """every block carries the pan: dx and dy come back within 0.01, the reference's own termination threshold errordif (:331,342)"""
    ad, _ = _oracle_blobs(oracle, isb, nf=1)
    b = _field(ad, lambda gx, gy: (np.full(gx.shape, pan[0] * ad.nPel), np.full(gx.shape, pan[1] * ad.nPel), np.full(gx.shape, 100)))
    got, stats = _both(mv, ad, [b])
    m = got[0]
    if pan[0] == 0:
        assert m["dx"] == f32(0.011) and stats["tiny_dx"] == 1          # the library's sign (divergence 1)
    else:
        assert abs(abs(m["dx"]) - abs(pan[0])) < 0.01 and (m["dx"] > 0) == ((pan[0] > 0) != bool(isb))   # backward vectors: the inverse motion
    assert abs(abs(m["dy"]) - abs(pan[1])) < 0.01
    # zoom and rot "to that order": the residual field of a model that is off by a translation t, a zoom z and a rotation r (radians) is
    # t + z * p + r * perp(p) at the block centre p taken from the centroid of the used blocks; on a grid with equal weights the three parts
    # are orthogonal, so error^2 = |t|^2 + (z^2 + r^2) * mean |p|^2, with `error` the estimator's own RMS residual (:175,184-185), measured
    # one update before the returned model.  Hence sqrt(z^2 + r^2) * rms |p| <= error.
    gy, gx = np.mgrid[4:ad.nBlkY - 4, 4:ad.nBlkX - 4]
    cx, cy = _centres(ad, gx, gy)
    rms = np.sqrt(((cx - cx.mean()) ** 2 + (cy - cy.mean()) ** 2).mean())
    assert np.hypot(m["zoom"] - 1, np.radians(m["rot"])) * rms <= m["error"], (m, rms)


def test_planted_zoom_and_rotation_have_the_right_sign_and_order(mv, oracle):
    ad, _ = _oracle_blobs(oracle, 0, nf=1)
    res = {}
    for name, k in (("z1", 0.01), ("z2", 0.03), ("r1", 0.01), ("r2", 0.03)):
        def fn(gx, gy, name=name, k=k):
            cx, cy = _centres(ad, gx, gy)
            vx, vy = (k * cx, k * cy) if name[0] == "z" else (-k * cy, k * cx)
            return np.rint(vx * ad.nPel), np.rint(vy * ad.nPel), np.full(gx.shape, 100)
        got, _ = _both(mv, ad, [_field(ad, fn)])
        res[name] = got[0]
    assert 1 < res["z1"]["zoom"] < res["z2"]["zoom"]
    assert (res["r1"]["rot"] > 0) == (res["r2"]["rot"] > 0) and 0 < abs(res["r1"]["rot"]) < abs(res["r2"]["rot"])
    # the opposite plant gives the opposite sign
    neg, _ = _both(mv, ad, [_field(ad, lambda gx, gy: (np.rint(-0.03 * _centres(ad, gx, gy)[0] * ad.nPel), np.rint(-0.03 * _centres(ad, gx, gy)[1] * ad.nPel), np.full(gx.shape, 100)))])
    assert neg[0]["zoom"] < 1


def test_crafted_fields_at_the_decision_edges(mv, oracle):
    ad, _ = _oracle_blobs(oracle, 0, nf=1)
    _, s1, s2 = vf.scaled_thresholds(ad, 400)
    nx, ny = ad.nBlkX, ad.nBlkY
    pel = ad.nPel
    rng = np.random.default_rng(5)
    pan = lambda gx: np.full(gx.shape, 4 * pel)

    # SAD exactly on thscd1 is kept, one above is rejected (and counted for the scene change)
    def sads(gx, gy):
        s = np.full(gx.shape, 50)
        s[6, 6], s[6, 7] = s1, s1 + 1
        return pan(gx), np.full(gx.shape, -2 * pel), s
    _, st = _both(mv, ad, [_field(ad, sads)])
    assert st["r_sad"] > 0
    ref = dr.Analyse(ad, W, H, s1, s2)
    grid = np.mgrid[0:ny, 0:nx][::-1]
    flat = lambda a, t: np.asarray(a).reshape(-1).astype(t)
    x, y, s = sads(*grid)
    one = {}
    ref.reject(dr.null(), flat(x, f32), flat(y, f32), flat(s, np.int64), np.ones(nx * ny, f32), f32(1e9), 4, one)
    assert one["r_sad"] == 1                                            # only the block one above

    # a neighbour deviation exactly on `wrong` is kept, the next representable step above it is not: one block differs from its eight equal neighbours
    for dev, rejected in ((10 * pel, 0), (10 * pel + 1, 1)):
        def lone(gx, gy, dev=dev):
            x = pan(gx).copy()
            x[8, 9] += dev
            return x, np.zeros(gx.shape, int), np.full(gx.shape, 50)
        one = {}
        x, y, s = lone(*grid)
        ref.reject(np.array([4, 1, 0, 0, 0, 1], f32), flat(x, f32) / f32(pel), flat(y, f32), flat(s, np.int64), np.ones(nx * ny, f32), f32(1e9), 4, one)
        assert one["r_x"] == rejected
        _both(mv, ad, [_field(ad, lone)])

    # zero vectors reach the zerow weight and the 0.011 rule; the 4-block border is ignored without a mask and used with one
    zero = _field(ad, lambda gx, gy: (np.zeros(gx.shape, int), np.zeros(gx.shape, int), np.full(gx.shape, 50)))
    got, st = _both(mv, ad, [zero])
    assert st["r_zero"] > 0 and st["tiny_dx"] == 1 and got[0]["dx"] == f32(0.011) and st["r_border"] > 0
    mask = rng.integers(0, 256, (H, W)).astype(np.uint8)

    def border_only(gx, gy):                                             # the pan lives in the border blocks only
        inner = (gx >= 4) & (gx < nx - 4) & (gy >= 4) & (gy < ny - 4)
        return np.where(inner, 0, 4 * pel), np.zeros(gx.shape, int), np.full(gx.shape, 50)
    got_nomask, _ = _both(mv, ad, [_field(ad, border_only)])
    got_mask, st = _both(mv, ad, [_field(ad, border_only)], masks=[np.full((H, W), 255, np.uint8)])
    assert got_nomask[0]["dx"] == f32(0.011) and got_mask[0]["dx"] > 1 and st.get("r_border", 0) == 0 and st["r_outside"] > 0
    _both(mv, ad, [_field(ad, sads), zero], masks=[mask, mask])

    # the scene-change count exactly on thscd2 is usable, one more is not
    for k, unusable in ((s2, 0), (s2 + 1, 1)):
        b = vf.scene_count(_field(ad, lambda gx, gy: (pan(gx), pan(gx), np.full(gx.shape, 50))), ad, 3, s1, k, 400)
        got, st = _both(mv, ad, [b, None, vf.invalid(b, ad)])
        assert st["unusable"] == 2 + unusable
        assert (got[0]["dx"] == 0.0) == bool(unusable) and got[1]["dx"] == 0.0 and got[2]["dx"] == 0.0 and got[1]["iter"] == 0


def test_a_mask_centre_outside_the_frame_weighs_one(mv, oracle):
    """16 x 16 blocks without overlap on 206 x 118: the grid stops inside the frame, so the frame is declared smaller than the vectors' to put the
    last centres outside it (the bounds test of :309)"""
    frames = pl.moving_clip(W, H, 8, 1, seed=3)
    sup = oracle.Super(W, H, 8)
    ad = oracle.Analyse(sup, num_frames=1, blksize=16, isb=0, delta=1).ad
    _, s1, s2 = vf.scaled_thresholds(ad, 400)
    w2, h2 = 190, 100                                                   # centres x = 200 and y = 104 lie outside
    b = _field(ad, lambda gx, gy: (np.full(gx.shape, 6), np.full(gx.shape, -4), np.full(gx.shape, 50)))
    mask = np.random.default_rng(2).integers(0, 256, (h2, w2)).astype(np.uint8)
    g = mv.DepanAnalyse(ad, w2, h2, mask=(8,))
    got = g.run_host([b], [mask])
    st = {}
    want = dr.Analyse(ad, w2, h2, s1, s2, has_mask=True).frame(b, mask, False, st)
    assert st["mask_outside"] > 0
    for k in ("dx", "dy", "zoom", "rot", "error"):
        assert f32(got[0][k]).tobytes() == f32(want[k]).tobytes()


# ------------------------------------------------------------------------------------------------ the header under the sanitizers

def _sanitizers_link(tmp):
    src = os.path.join(tmp, "one.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    gxx = shutil.which("g++")
    if not gxx:
        return "no g++"
    r = subprocess.run([gxx, "-fsanitize=address,undefined", src, "-o", os.path.join(tmp, "one")], capture_output=True)
    return None if r.returncode == 0 and subprocess.run([os.path.join(tmp, "one")]).returncode == 0 else "g++ does not link -fsanitize=address,undefined here"


def test_estimator_header_in_a_stand_alone_program_under_the_sanitizers(mv, oracle, tmp_path):
    why = _sanitizers_link(str(tmp_path))
    if why:
        pytest.skip(why)
    exe = str(tmp_path / "depan_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "vapoursynth-mvtools_amd", "csrc"), os.path.join(HERE, "depan_host_main.cpp"), "-o", exe])
    ad, blobs = _oracle_blobs(oracle, 1)
    _, s1, s2 = vf.scaled_thresholds(ad, 400)
    zero = _field(ad, lambda gx, gy: (np.zeros(gx.shape, int), np.zeros(gx.shape, int), np.full(gx.shape, 50)))
    mask = np.random.default_rng(9).integers(0, 256, (H, W)).astype(np.uint8)
    for has_mask, fields in ((0, [blobs[0], blobs[1], blobs[3], zero]), (1, [blobs[1], zero])):
        ref = dr.Analyse(ad, W, H, s1, s2, has_mask=bool(has_mask))
        for n, b in enumerate(fields):
            path = str(tmp_path / ("field%d_%d.bin" % (has_mask, n)))
            with open(path, "wb") as f:
                f.write(struct.pack("<13i", ad.nBlkX, ad.nBlkY, ad.nBlkSizeX, ad.nBlkSizeY, ad.nOverlapX, ad.nOverlapY, ad.nPel, ad.nLvCount, ad.isBackward, W, H, has_mask, s2))
                f.write(struct.pack("<q", s1))
                f.write(struct.pack("<i", len(b)))
                f.write(b.tobytes())
                if has_mask:
                    f.write(mask.tobytes())
            out = subprocess.run([exe, path], capture_output=True, text=True)
            assert out.returncode == 0, out.stderr
            bits = [int(v, 16) for v in out.stdout.split()]
            want = ref.frame(b, mask if has_mask else None)
            assert bits[:5] == [int(f32(want[k]).view(np.uint32)) for k in ("dx", "dy", "zoom", "rot", "error")] and bits[5] == want["iter"]
