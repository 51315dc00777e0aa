"""GPU tests of dct = 1..4 (the float block DCT as luma cost).  The device is held byte for byte to the library's own arithmetic
compiled for the host: mvx_analyse_dct_blocks against tests/dct_emu.cpp, Analyse and Recalculate blobs against the DCT-capable oracle that
tests/dct_oracle.py builds around the same text.  Properties that need no oracle, and one graph through the VapourSynth shell, follow.  Every test
here fails without the feature: the creates refuse these modes."""
import os
import subprocess

import numpy as np
import pytest

import dct_oracle as do
import dct_ref as dr
import pipeline as pl
from test_vs_shim import HOST, PLUGIN, _read_frames, _write_clip, host

pytestmark = pytest.mark.gpu
W, H = 128, 80


@pytest.fixture(scope="module")
def od():
    return do.module()


@pytest.fixture(autouse=True)
def dct_on(mv):
    was = mv.enable_dct_float(True)
    yield
    mv.enable_dct_float(was)


# ------------------------------------------------------------------------------------------------ 1. the device transform and quantiser

@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("bw,bh", dr.SHAPES)
def test_dct_blocks_equal_the_host_build(od, mv, bw, bh, bits):
    """blocks at the four padded corners of every sub-pel plane of the finest level, at the ends of the whole plane, and at seeded positions"""
    import torch
    frames = pl.moving_clip(W, H, bits, 1, seed=3, noise=3)
    osup, gsup = od.Super(W, H, bits, pel=2), mv.Super(W, H, bits, pel=2)
    sf = osup.frame(frames[0])
    gsf = gsup.from_host(sf)
    plane = sf[0]
    rows, cols = osup.plane_shape(0)
    rng = np.random.default_rng(bw * 100 + bh + bits)
    xs, ys = [0, cols - bw], [0, rows - bh]
    for (p, lv, k, y0, x0, h, w) in osup.defined_regions():
        if p == 0 and lv == 0:
            xs += [x0, x0 + w - bw, x0, x0 + w - bw] + [int(v) for v in rng.integers(x0, x0 + w - bw + 1, 3)]
            ys += [y0, y0, y0 + h - bh, y0 + h - bh] + [int(v) for v in rng.integers(y0, y0 + h - bh + 1, 3)]
    an = mv.Analyse(gsup, blksize=bw, blksizev=bh, dct=1)
    got = an.dct_blocks(gsf[0], xs, ys)
    torch.cuda.synchronize()
    assert got.shape == (len(xs), bh, bw)
    for i, (x, y) in enumerate(zip(xs, ys)):
        want = do.emu_bytes(plane[y:y + bh, x:x + bw], bits)
        assert np.array_equal(got[i], want), "block %d at (%d, %d): %d bytes differ" % (i, x, y, int((got[i] != want).sum()))


# ------------------------------------------------------------------------------------------------ 2. Analyse against the patched oracle

def _clip(bits, fmt=None, ramp=0, seed=11):
    f = fmt or {}
    frames = pl.moving_clip(W, H, bits, 3, seed=seed, noise=3, sub=f.get("subsampling", (1, 1)))
    if f.get("gray"):
        frames = [[fr[0]] for fr in frames]
    if ramp:
        do.luma_ramp(frames, bits, ramp)
    return frames


def _supers(od, mv, bits, skw, frames):
    osup, gsup = od.Super(W, H, bits, **skw), mv.Super(W, H, bits, **skw)
    osf = [osup.frame(f) for f in frames]
    return osup, gsup, osf, [gsup.from_host(sf) for sf in osf]  # the oracle's super frames feed the GPU search: the test isolates Analyse


JOBS = [(0, 1), (1, 0), (1, 2), (2, None)]  # the last one has ref == NULL


def _analyse_blobs(od, mv, bits, skw, akw, frames):
    import torch
    osup, gsup, osf, gsf = _supers(od, mv, bits, skw, frames)
    oan, gan = od.Analyse(osup, **akw), mv.Analyse(gsup, **akw)
    assert gan.blob_size == oan.blob_size
    got = gan.run([(gsf[a], gsf[b] if b is not None else None) for a, b in JOBS])
    torch.cuda.synchronize()
    want = [oan.frame(osf[a], osf[b] if b is not None else None) for a, b in JOBS]
    return [g.cpu().numpy() for g in got], want, oan


def _assert_blobs(got, want, ad):
    for i, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            msg = []
            for lvl in range(ad.nLvCount - 1, -1, -1):
                gx, gy, gs = pl.blob_vectors(g, ad, lvl)
                wx, wy, ws = pl.blob_vectors(w, ad, lvl)
                d = (gx != wx) | (gy != wy) | (gs != ws)
                if d.any():
                    y, x = (int(v[0]) for v in np.nonzero(d))
                    msg.append("level %d: %d/%d blocks differ, first (by=%d,bx=%d): gpu (%d,%d,%d) oracle (%d,%d,%d)" % (
                        lvl, int(d.sum()), d.size, y, x, gx[y, x], gy[y, x], gs[y, x], wx[y, x], wy[y, x], ws[y, x]))
            pytest.fail("job %d blob differs: %s" % (i, " ; ".join(msg[:4]) or "outside the vector arrays"))


R = 40  # brightness ramp: dctweight16 > 0 in mode 2, the luma switch of modes 3 / 4 fires
ANALYSE_CASES = [
    # mode 1: every block shape, overlap none and half, both sample sizes
    (8, {}, {}, dict(dct=1, blksize=4), 0),
    (8, {}, {}, dict(dct=1, blksize=8, overlap=4), 0),
    (16, {}, {}, dict(dct=1, blksize=16, overlap=8), 0),
    (8, {}, {}, dict(dct=1, blksize=32), 0),
    (16, {}, {}, dict(dct=1, blksize=8, blksizev=4, overlap=4, overlapv=2), 0),
    (8, {}, {}, dict(dct=1, blksize=16, blksizev=2), 0),
    (10, {}, {}, dict(dct=1, blksize=8, overlap=4), 0),
    (16, {}, {}, dict(dct=1, blksize=8), 0),
    # mode 2 with a brightness change
    (8, {}, {}, dict(dct=2, blksize=8), R),
    (16, {}, {}, dict(dct=2, blksize=16, overlap=8), R),
    (8, {}, {}, dict(dct=2, blksize=4, overlap=2), R),
    (16, {}, {}, dict(dct=2, blksize=32, overlap=16), R),
    (16, {}, {}, dict(dct=2, blksize=8, blksizev=4), R),
    (8, {}, {}, dict(dct=2, blksize=16, blksizev=2, overlap=8, overlapv=0), R),
    # modes 3 and 4 with the ramp
    (8, {}, {}, dict(dct=3, blksize=8, overlap=4), R),
    (16, {}, {}, dict(dct=3, blksize=16), R),
    (16, {}, {}, dict(dct=3, blksize=4), R),
    (8, {}, {}, dict(dct=3, blksize=32, overlap=16), R),
    (8, {}, {}, dict(dct=3, blksize=8, blksizev=4), R),
    (16, {}, {}, dict(dct=3, blksize=16, blksizev=2), R),
    (16, {}, {}, dict(dct=4, blksize=8), R),
    (8, {}, {}, dict(dct=4, blksize=16, overlap=8), R),
    (8, {}, {}, dict(dct=4, blksize=4, overlap=2), R),
    (16, {}, {}, dict(dct=4, blksize=32), R),
    (16, {}, {}, dict(dct=4, blksize=8, blksizev=4, overlap=4, overlapv=2), R),
    (8, {}, {}, dict(dct=4, blksize=16, blksizev=2), R),
    # sub-pel precision
    (8, {}, dict(pel=1), dict(dct=1, blksize=8, overlap=4), 0),
    (16, {}, dict(pel=4), dict(dct=3, blksize=8), R),
    (8, {}, dict(pel=4), dict(dct=1, blksize=16, overlap=8), 0),
    # search patterns: exhaustive, hexagon (the default, named), UMH
    (8, {}, {}, dict(dct=1, blksize=8, search=3, searchparam=2), 0),
    (16, {}, {}, dict(dct=2, blksize=8, overlap=4, search=3, searchparam=3), R),
    (8, {}, {}, dict(dct=4, blksize=8, search=5, searchparam=4), R),
    (8, {}, {}, dict(dct=1, blksize=16, search=4, searchparam=4), 0),
    # luma only
    (8, {}, {}, dict(dct=1, blksize=8, chroma=0), 0),
    (16, {}, {}, dict(dct=4, blksize=16, overlap=8, chroma=0), R),
    # divide, trymany, meander
    (8, {}, {}, dict(dct=1, blksize=8, overlap=4, divide=1), 0),
    (8, {}, {}, dict(dct=1, blksize=8, trymany=1), 0),
    (8, {}, {}, dict(dct=2, blksize=8, overlap=4, meander=0), R),
    # other formats
    (8, dict(subsampling=(0, 0)), {}, dict(dct=1, blksize=8, overlap=4), 0),
    (16, dict(gray=True), {}, dict(dct=3, blksize=8), R),
    (8, {}, {}, dict(dct=1, blksize=8, truemotion=0), 0),
]


@pytest.mark.parametrize("bits,fmt,skw,akw,ramp", ANALYSE_CASES)
def test_analyse_blobs_equal_the_patched_oracle(od, mv, bits, fmt, skw, akw, ramp):
    got, want, oan = _analyse_blobs(od, mv, bits, dict(fmt, **skw), akw, _clip(bits, fmt, ramp))
    _assert_blobs(got, want, oan.ad)
    if akw["dct"] == 2:  # the case means what it says: dctweight16 is not zero (the oracle's blob differs from its spatial search's)
        frames = _clip(bits, fmt, ramp)
        osup = od.Super(W, H, bits, **dict(fmt, **skw))
        assert not np.array_equal(od.Analyse(osup, **dict(akw, dct=0)).frame(osup.frame(frames[0]), osup.frame(frames[1])), want[0])


# ------------------------------------------------------------------------------------------------ 3. Recalculate

RECALC_CASES = [(m, bits, blk, smooth) for m in (1, 2, 3, 4) for bits, blk, smooth in ((8, 8, 1), (16, 16, 0), (8, 16, 0), (16, 8, 1))]


@pytest.mark.parametrize("mode,bits,blk,smooth", RECALC_CASES)
def test_recalculate_blobs_equal_the_patched_oracle(od, mv, mode, bits, blk, smooth):
    import torch
    frames = _clip(bits, None, R, seed=53)
    osup, gsup, osf, gsf = _supers(od, mv, bits, {}, frames)
    akw = dict(blksize=16 if blk == 8 else 8, overlap=0, isb=1)
    oan, gan = od.Analyse(osup, num_frames=3, **akw), mv.Analyse(gsup, num_frames=3, **akw)
    pairs = [(0, 1), (1, 2), (2, None)]
    oold = [oan.frame(osf[a], osf[b] if b is not None else None) for a, b in pairs]
    gold = gan.run([(gsf[a], gsf[b] if b is not None else None) for a, b in pairs])
    rkw = dict(blksize=blk, overlap=blk // 2, thsad=60, smooth=smooth, dct=mode)
    orc, grc = od.Recalculate(osup, oan.ad, **rkw), mv.Recalculate(gsup, gan.ad, **rkw)
    assert grc.blob_size == orc.blob_size
    got = grc.run([(gsf[a], gsf[b] if b is not None else None, gold[i]) for i, (a, b) in enumerate(pairs)])
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(pairs):
        want = orc.frame(osf[a], osf[b] if b is not None else None, oold[i])
        g = got[i].cpu().numpy()
        assert np.array_equal(g, want), (i, int(np.count_nonzero(g != want)))


# ------------------------------------------------------------------------------------------------ 4. properties that need no oracle

@pytest.mark.parametrize("bits,akw", [(8, dict(blksize=8, overlap=4)), (16, dict(blksize=16))])
def test_mode_2_without_a_brightness_change_is_the_spatial_search(od, mv, bits, akw):
    """dctweight16 == 0: the DCT is never taken and the blob is dct=0's, exactly.  The weight is the smallest plane's mean luma change per sample in
    sample units, so the 16-bit clip carries the 8-bit clip's values: scaled to 16 bits the texture's motion alone moves the mean by more than one unit."""
    frames = [[p.astype(np.uint8 if bits == 8 else np.uint16) for p in f] for f in _clip(8)]
    plain, wplain, _ = _analyse_blobs(od, mv, bits, {}, dict(akw, dct=0), frames)
    got, want, _ = _analyse_blobs(od, mv, bits, {}, dict(akw, dct=2), frames)
    assert all(np.array_equal(a, b) for a, b in zip(want, wplain)), "the clip does not have dctweight16 == 0"
    assert all(np.array_equal(a, b) for a, b in zip(got, plain))


@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("bits,akw", [(8, dict(blksize=8, overlap=4)), (16, dict(blksize=16))])
def test_modes_3_and_4_without_a_luma_difference_are_the_spatial_search(od, mv, mode, bits, akw):
    """a clip whose blocks' luma sums all lie within a 32nd of each other (the moving texture at a 32nd of its contrast): the switch never fires"""
    frames = do.flat_clip(_clip(bits), bits)
    plain, wplain, _ = _analyse_blobs(od, mv, bits, {}, dict(akw, dct=0), frames)
    got, want, _ = _analyse_blobs(od, mv, bits, {}, dict(akw, dct=mode), frames)
    assert all(np.array_equal(a, b) for a, b in zip(want, wplain)), "the luma switch fires on this clip"
    assert all(np.array_equal(a, b) for a, b in zip(got, plain))


@pytest.mark.parametrize("bits", [8, 10])
def test_mode_1_sad_of_every_block_is_the_float64_cost_of_its_own_vector(od, mv, bits):
    """every block of the finest level of a dct=1 blob: its sad equals the float64 yardstick's DCT cost of the block against the block its own vector
    points at, plus the two chroma SADs -- wherever the proven bound determines every byte involved (pel=1: blocks lie in the one padded plane)"""
    bw = 8
    frames = _clip(bits)
    got, want, oan = _analyse_blobs(od, mv, bits, dict(pel=1), dict(dct=1, blksize=bw, overlap=0), frames)
    osup = od.Super(W, H, bits, pel=1)
    osf = [osup.frame(f) for f in frames]
    reg = {p: (y0, x0) for (p, lv, k, y0, x0, h, w) in osup.defined_regions() if lv == 0}
    s, shift = osup.s, dr.dct_shift(bw, bw)
    checked = 0
    for (a, b), blob in zip(JOBS[:3], got):
        vx, vy, sad = pl.blob_vectors(blob, oan.ad, 0)
        for by in range(vx.shape[0]):
            for bx in range(vx.shape[1]):
                y0, x0 = reg[0][0] + s.vpad + bw * by, reg[0][1] + s.hpad + bw * bx
                src = osf[a][0][y0:y0 + bw, x0:x0 + bw]
                ref = osf[b][0][y0 + vy[by, bx]:y0 + vy[by, bx] + bw, x0 + vx[by, bx]:x0 + vx[by, bx] + bw]
                if not all(dr.determined(dr.coeffs64(blk), dr.error_bound(blk), bits, shift).all() for blk in (src, ref)):
                    continue
                total = dr.luma_cost(src, ref, bits, 1, 0, 0)
                cvx, cvy = (vx[by, bx] + (1 if vx[by, bx] < 0 else 0)) >> 1, (vy[by, bx] + (1 if vy[by, bx] < 0 else 0)) >> 1
                for p in (1, 2):
                    cy0, cx0 = reg[p][0] + s.vpad // 2 + (bw // 2) * by, reg[p][1] + s.hpad // 2 + (bw // 2) * bx
                    cs = osf[a][p][cy0:cy0 + bw // 2, cx0:cx0 + bw // 2].astype(np.int64)
                    cr = osf[b][p][cy0 + cvy:cy0 + cvy + bw // 2, cx0 + cvx:cx0 + cvx + bw // 2].astype(np.int64)
                    total += int(np.abs(cs - cr).sum())
                assert int(sad[by, bx]) == total, (a, b, by, bx)
                checked += 1
    assert checked > 100


# ------------------------------------------------------------------------------------------------ 5. through the VapourSynth shell

def _oracle_degrain1(od, frames, bits, akw):
    sup = od.Super(W, H, bits)
    sf = [sup.frame(f) for f in frames]
    n = len(frames)
    ans = [od.Analyse(sup, num_frames=n, isb=isb, delta=1, **akw) for isb in (1, 0)]
    dg = od.Degrain(1, sup, ans[0].ad)
    out = []
    for k in range(n):
        rs = [k + 1, k - 1]
        refs = [sf[r] if 0 <= r < n else None for r in rs]
        out.append(dg.frame(frames[k], refs, [an.frame(sf[k], ref) for an, ref in zip(ans, refs)]))
    return out


def test_shell_graph_with_MVX_VS_DCT(od, tmp_path):
    """Analyse(dct=1) -> Degrain1 through the real plugin in the mini host with MVX_VS_DCT=1, against the same chain on the patched oracle"""
    bits, n = 8, 5
    frames = pl.moving_clip(W, H, bits, n, seed=7, noise=3)
    src, out = str(tmp_path / "in.raw"), str(tmp_path / "out.raw")
    _write_clip(src, frames)
    host("list")
    r = subprocess.run([HOST, PLUGIN, "run", "degrain1", src, str(W), str(H), str(bits), str(n), out, "a.blksize=8", "a.overlap=4", "a.dct=1"],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, MVX_VS_DCT="1"))
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = _read_frames(out, W, H, bits, n)
    want = _oracle_degrain1(od, frames, bits, dict(blksize=8, overlap=4, dct=1))
    for k in range(n):
        for p in range(3):
            assert np.array_equal(got[k][p], want[k][p]), "frame %d plane %d" % (k, p)


def test_shell_without_the_switch_refuses_as_before():
    env = dict(os.environ)
    env.pop("MVX_VS_DCT", None)
    r = subprocess.run([HOST, PLUGIN, "error", "Analyse", "128", "96", "8", "f.dct=1"], capture_output=True, text=True, timeout=300, env=env)
    assert r.stdout.strip() == "ERROR Analyse: dct 1..4 (FFTW3 DCT cost) are not implemented on the GPU path.", r.stdout + r.stderr
