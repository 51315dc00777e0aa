"""Stage 2 of the speculative search's 16x16 row passes evaluates the 14 points of a Hex2 pattern in passes of eight lane groups.  Four strip-form
windows in a row share their passes (mvx_analyse_spec.h: PACK -- seven passes for the four, not eight; a packed pass holds points of two
neighbouring windows).  Packing decides only WHICH pass computes a table entry: the vector blobs must be the oracle's, byte for byte, on block
rows of one packable group (28 blocks), a group plus a short or a full window (29, 35), three windows (21: nothing to pack, the same path), two
groups and one block more (56, 57), 113; walked forwards and backwards (the meander reverses the order of a group's windows); one wave per chain
and as teams; side by side (eight windows per group: two runs of four); with groups in which one window is not in strip form; on an exhaustive
level and at pel 1.  The 8-bit 16x16 builds keep one strip buffer and do not pack: they run the same cases as the unpacked form of the code."""
import ctypes as C
import functools

import numpy as np
import pytest

import pipeline as pl

pytestmark = pytest.mark.gpu

NBLKX = [21, 28, 29, 35, 56, 57, 113]
FORMS = [0, 2, 4]  # waves per chain of the team form; 0: one wave per chain


@pytest.fixture
def dbg(mv):
    """kernel-variant switches for one test (mvx_debug_option: selects among kernels that compute identical results); reset afterwards"""
    used = []

    def set_(name, value):
        mv.debug_option(name, value)
        used.append(name)
    yield set_
    for name in used:
        mv.debug_option(name, -1 if name == "team" else 1 if name == "spec" else 0)


def _two_region_clip(w, h, bits, split_x):
    """columns left of split_x move by (5, -2) per frame, the rest by (-3, 1): the same texture and noise, cut along one luma column (even: 4:2:0)"""
    a = pl.moving_clip(w, h, bits, 3, seed=23, noise=4, motion=(5, -2))
    b = pl.moving_clip(w, h, bits, 3, seed=23, noise=4, motion=(-3, 1))
    out = []
    for fa, fb in zip(a, b):
        planes = []
        for p in range(3):
            s = split_x if p == 0 else split_x // 2
            planes.append(np.ascontiguousarray(np.concatenate([fa[p][:, :s], fb[p][:, s:]], axis=1)))
        out.append(planes)
    return out


@functools.lru_cache(maxsize=4)
def _oracle_side(w, h, bits, blk, ov, meander, search, pel, split_x):
    """frames, the oracle's blobs (backward, forward, no reference) and analysis data: the same for every form of the launch"""
    import mvoracle as oracle
    frames = _two_region_clip(w, h, bits, split_x) if split_x else pl.moving_clip(w, h, bits, 3, seed=23, noise=4, motion=(5, -2))
    osup = oracle.Super(w, h, bits, pel=pel)
    osf = [osup.frame(f) for f in frames]
    want = []
    for isb in (1, 0):
        oan = oracle.Analyse(osup, isb=isb, blksize=blk, overlap=ov, meander=meander, search=search)
        want.append((oan.frame(osf[1], osf[2 if isb else 0]), oan.frame(osf[1], None)))
    return frames, want, oan.ad


def _case(mv, dbg, bits, blk, ov, nblkx, rows, meander, team, search=None, pel=None, split_x=0, precondition=None):
    step = blk - ov
    w, h = step * nblkx + ov, step * rows + ov
    frames, want, ad = _oracle_side(w, h, bits, blk, ov, meander, search, pel, split_x)
    assert (ad.nBlkX, ad.nBlkY) == (nblkx, rows), "the clip does not have the block grid this case is about"
    assert ad.nBlkY >= 3  # (the last block row takes its "ahead" predictor from the row above: three rows exercise first, middle and last)
    if precondition:
        precondition(want, ad)  # (on the CPU, from the oracle's own vectors, before the GPU is used)
    dbg("team", team)
    gsup = mv.Super(w, h, bits, pel=pel)
    gsf = gsup.build([mv.frame_to_device(f) for f in frames])
    info = (C.c_int * 5)()
    for isb, (o_ref, o_none) in zip((1, 0), want):
        gan = mv.Analyse(gsup, isb=isb, blksize=blk, overlap=ov, meander=meander, search=search)
        got = gan.run([(gsf[1], gsf[2 if isb else 0]), (gsf[1], None)])
        mv.lib().mvx_debug_last_launch(info)
        assert info[4] == (3 if team else 2), "not the speculative kernel in the form this case is meant to cover (%s)" % list(info)
        if team:
            assert info[1] == team, list(info)
        assert got[0].cpu().numpy().tobytes() == o_ref.tobytes(), "vectors differ from the oracle (isb=%d)" % isb
        assert got[1].cpu().numpy().tobytes() == o_none.tobytes(), "the default vectors of a job without a reference differ (isb=%d)" % isb


@pytest.mark.parametrize("team", FORMS)
@pytest.mark.parametrize("meander", [1, 0])
@pytest.mark.parametrize("nblkx", NBLKX)
@pytest.mark.parametrize("bits", [16, 8])
def test_packing_16x16_overlap8(mv, dbg, bits, nblkx, meander, team):
    """windows of 7 blocks, groups of 4 windows: a full group of a smooth field packs"""
    _case(mv, dbg, bits, 16, 8, nblkx, 5, meander, team)


@pytest.mark.parametrize("team", FORMS)
@pytest.mark.parametrize("meander", [1, 0])
@pytest.mark.parametrize("nblkx", [64, 65])
@pytest.mark.parametrize("bits", [16, 8])
def test_packing_side_by_side(mv, dbg, bits, nblkx, meander, team):
    """16x16 blocks side by side: windows of 4 blocks, 8 windows per group -- runs of eight strip-form windows are two packed runs of four"""
    _case(mv, dbg, bits, 16, 0, nblkx, 3, meander, team)


def _mixed_group_precondition(want, ad):
    """at least one block row has, inside one group of 28 blocks, a window of 7 whose final vectors are all equal AND a window whose vectors are
    not (a proxy for "runs of one to three strip-form windows beside a block-form window", which cannot be observed from outside the kernel)"""
    found = False
    for o_ref, _ in want:
        vx, vy, _sad = pl.blob_vectors(o_ref, ad, 0)
        for row in range(1, ad.nBlkY):  # (the first block row is searched live)
            for g0 in range(0, ad.nBlkX - 27, 28):
                same = []
                for f in range(g0, g0 + 28, 7):
                    xs, ys = vx[row, f:f + 7], vy[row, f:f + 7]
                    same.append(bool((xs == xs[0]).all() and (ys == ys[0]).all()))
                found = found or (any(same) and not all(same))
    assert found, "the clip has no group with both a uniform and a non-uniform window: this case does not cover mixed groups"


@pytest.mark.parametrize("team", [0, 2])
@pytest.mark.parametrize("meander", [1, 0])
@pytest.mark.parametrize("bits", [16, 8])
def test_packing_mixed_groups(mv, dbg, bits, meander, team):
    """two motion regions whose boundary (block 10) falls inside the first group's second window: that group cannot pack, its strip-form windows run
    on their own beside a block-form one"""
    _case(mv, dbg, bits, 16, 8, 57, 5, meander, team, split_x=80, precondition=_mixed_group_precondition)


def test_packing_exhaustive_level_unaffected(mv, dbg):
    """search=3: 24 points are exactly three passes per window -- nothing packs, the pass tables of the Hex2 levels must not leak into this path"""
    _case(mv, dbg, 16, 16, 8, 57, 5, 1, 0, search=3)


def test_packing_pel1(mv, dbg):
    """pel 1: one plane, the pattern offsets are whole pels"""
    _case(mv, dbg, 16, 16, 8, 57, 5, 1, 0, pel=1)
