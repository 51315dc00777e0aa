"""The speculative search walks a block row in frames of two groups, and a group is a whole number of the build's row-pass windows
(mvx_analyse_spec.h: GT / FR -- 28 blocks in a frame of 56 for 16x16 blocks overlapping by 8, 30 in 60 for 8-bit 8x8 blocks overlapping by 4,
32 in 64 for blocks side by side).  Grouping decides only which blocks are speculated together: the vector blobs must be the oracle's, byte
for byte, on widths that put the number of blocks per row one below, at and one above every group and frame boundary -- of the new geometry
and of the 32 / 64 it replaces -- with the meander on and off, one wave per chain and as teams of two and four waves."""
import ctypes as C
import functools

import numpy as np
import pytest

import pipeline as pl

pytestmark = pytest.mark.gpu

# blocks per row around the boundaries of 28 / 56 (and 32 / 64, two frames, two frames + 1) and of 30 / 60
NBLKX_16 = [27, 28, 29, 55, 56, 57, 63, 64, 65, 112, 113]
NBLKX_8 = [29, 30, 31, 59, 60, 61, 63, 64, 65, 120, 121]
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


@functools.lru_cache(maxsize=4)
def _oracle_side(w, h, bits, blk, ov, meander):
    """frames, the oracle's super frames and its blobs (backward, forward, no reference): the same for every form of the launch"""
    import mvoracle as oracle
    frames = pl.moving_clip(w, h, bits, 3, seed=23, noise=4, motion=(5, -2))
    osup = oracle.Super(w, h, bits)
    osf = [osup.frame(f) for f in frames]
    want = []
    for isb in (1, 0):
        oan = oracle.Analyse(osup, isb=isb, blksize=blk, overlap=ov, meander=meander)
        want.append((oan.frame(osf[1], osf[2 if isb else 0]), oan.frame(osf[1], None)))
    return frames, want, (oan.ad.nBlkX, oan.ad.nBlkY)


def _case(mv, dbg, bits, blk, ov, nblkx, rows, meander, team):
    step = blk - ov
    w, h = step * nblkx + ov, step * rows + ov
    frames, want, (nx, ny) = _oracle_side(w, h, bits, blk, ov, meander)
    assert (nx, ny) == (nblkx, rows), "the clip does not have the block grid this case is about"
    assert ny >= 3  # (the last block row takes its "ahead" predictor from the row above: three rows exercise first, middle and last)
    dbg("team", team)
    gsup = mv.Super(w, h, bits)
    gsf = gsup.build([mv.frame_to_device(f) for f in frames])
    info = (C.c_int * 5)()
    for isb, (o_ref, o_none) in zip((1, 0), want):
        gan = mv.Analyse(gsup, isb=isb, blksize=blk, overlap=ov, meander=meander)
        got = gan.run([(gsf[1], gsf[2 if isb else 0]), (gsf[1], None)])
        mv.lib().mvx_debug_last_launch(info)
        assert info[4] == (3 if team else 2), "not the speculative kernel in the form this case is meant to cover (%s)" % list(info)
        if team:
            assert info[1] == team, list(info)
        assert got[0].cpu().numpy().tobytes() == o_ref.tobytes(), "vectors differ from the oracle (isb=%d)" % isb
        assert got[1].cpu().numpy().tobytes() == o_none.tobytes(), "the default vectors of a job without a reference differ (isb=%d)" % isb


@pytest.mark.parametrize("team", FORMS)
@pytest.mark.parametrize("meander", [1, 0])
@pytest.mark.parametrize("nblkx", NBLKX_16)
@pytest.mark.parametrize("bits", [16, 8])
def test_groups_16x16_overlap8(mv, dbg, bits, nblkx, meander, team):
    """windows of 7 blocks: groups of 28 in frames of 56"""
    _case(mv, dbg, bits, 16, 8, nblkx, 5, meander, team)


@pytest.mark.parametrize("team", FORMS)
@pytest.mark.parametrize("meander", [1, 0])
@pytest.mark.parametrize("nblkx", NBLKX_8)
def test_groups_8x8_overlap4(mv, dbg, nblkx, meander, team):
    """8-bit row passes, windows of 15 blocks: groups of 30 in frames of 60"""
    _case(mv, dbg, 8, 8, 4, nblkx, 7, meander, team)


@pytest.mark.parametrize("team", FORMS)
@pytest.mark.parametrize("meander", [1, 0])
@pytest.mark.parametrize("bits,blk", [(16, 16), (8, 16), (8, 8)])
def test_groups_side_by_side(mv, dbg, bits, blk, meander, team):
    """blocks side by side (windows of 4 / 8 blocks): groups of 32 in frames of 64, as before -- 65 blocks per row: one frame and one block"""
    _case(mv, dbg, bits, blk, 0, 65, 4, meander, team)
