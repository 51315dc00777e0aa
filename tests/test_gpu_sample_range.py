"""The block pipeline and the per-pixel Flow filters at the ENDS of the sample range: the HIP path against the CPU oracle (the Flow
filters: against the restatements tests/flow_ref.py and tests/flowmc_ref.py), bit-exact, on the clips of tests/sample_range.py
(tests/test_sample_range.py shows on the CPU that each of them reaches what it is here for).  The runners are those of
tests/test_gpu_parity.py, tests/test_gpu_flow.py and tests/test_gpu_flowmc.py, given other frames."""
import ctypes as C
import itertools

import pytest

import sample_range as sr
import test_gpu_flow as gflow
import test_gpu_flowmc as gflowmc
import test_gpu_parity as gp
import vector_fields as vf
from test_gpu_parity import dbg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def _id(v):
    if isinstance(v, dict):
        return ",".join("%s=%s" % kv for kv in v.items()) or "defaults"
    if isinstance(v, tuple):
        return "sub%d%d" % v
    return None


# ----------------------------------------------------------------------------------------------------------------- Super
@pytest.mark.parametrize("gen,w,h,bits,sub,kw", sr.SUPER_CASES, ids=_id)
def test_super_at_the_rails(oracle, mv, gen, w, h, bits, sub, kw):
    """min(pm, max(0, v)) of the bicubic / Wiener taps at every depth's own pm, the reduce filters on 0 / pm edges, both level-0 kernels"""
    gp._super_case(oracle, mv, w, h, bits, sub, kw, frames=sr.make(gen, w, h, bits, 2, sub=sub))


def test_super_fused_shadow_planes_on_checker(mv):
    gp._shadow_case(mv, 138, 70, 10, (1, 1), {}, frames=sr.checker(138, 70, 10, 2))


# --------------------------------------------------------------------------------------------------------------- Analyse
KERNELS = ["default", "general", "serial", "plain-layout", "spec-off", "spec-everywhere", "team"]


def _step_frames(case, n):
    name, bits, sub, lo, hi, akw = case
    return sr.step(sr.STEP_W, sr.STEP_H, bits, n, lo, hi, sub=sub)


def _search_through(oracle, mv, dbg, kernel, case):
    """one step-clip case through one of the kernels that hold the penalty expression: whole blobs, every level, both directions and
    the call without a reference"""
    name, bits, sub, lo, hi, akw = case
    skw = {} if sub == (1, 1) else dict(subsampling=sub)
    if kernel == "plain-layout":   # (the layout is the Super's: its own runner builds the super frames on the GPU)
        return gp._other_kernels_case(oracle, mv, dbg, kernel, sr.STEP_W, sr.STEP_H, bits, skw, akw, frames=_step_frames(case, 3))
    if kernel == "team":
        return gp._speculative_case(oracle, mv, dbg, "team", sr.STEP_W, sr.STEP_H, bits, skw, akw, frames=_step_frames(case, 3))
    if kernel == "general":
        dbg("general", 1)
    if kernel == "serial":
        dbg("spec", 0)
    if kernel == "spec-off":
        dbg("spec", 2)
        dbg("team", 0)   # (one wave per chain: a launch this small would otherwise run as a team, like "default")
    if kernel == "spec-everywhere":
        dbg("spec", 5)
        dbg("team", 0)
    try:
        gp._analyse_case(oracle, mv, sr.STEP_W, sr.STEP_H, bits, skw, akw, frames=_step_frames(case, 2))
    finally:  # the kernel this route is meant to cover did run (mvx_debug_last_launch: [0] chains per SIMD of the lean kernel, 0 = general; [4] 2 = speculative, 3 = team)
        info = (C.c_int * 5)()
        mv.lib().mvx_debug_last_launch(info)
        took = "general" if info[0] == 0 else {0: "lean", 2: "speculative", 3: "team"}[info[4]]
        want = {"default": "team", "general": "general", "serial": "lean", "spec-off": "speculative", "spec-everywhere": "speculative"}[kernel]
        assert took == ("general" if sub != (1, 1) else want), "not the kernel this route is meant to cover: %s (%s)" % (took, list(info))


@pytest.mark.parametrize("case", sr.PENALTY_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("kernel", KERNELS)
def test_analyse_penalty_product_past_2_31(oracle, mv, dbg, kernel, case):
    """pnew * SAD >= 2^31 (PlaneOfBlocks.cpp:238,247 multiply in 64 bits): a product wrapped to a negative penalty lets every new
    candidate undercut the predictor"""
    _search_through(oracle, mv, dbg, kernel, case)


@pytest.mark.parametrize("case", sr.CONTROL_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("kernel", KERNELS)
def test_analyse_penalty_controls(oracle, mv, dbg, kernel, case):
    """the largest block SAD there is (the sum's bound, 2^27) and the depths that cannot reach the product's bound"""
    _search_through(oracle, mv, dbg, kernel, case)


def test_analyse_penalty_product_444_chroma_only(oracle, mv, dbg):
    """4:4:4: pnew * (chroma SAD) passes 2^31 while pnew * (luma SAD) does not -- the second line of the expression, in the general kernel.
    (A 4:4:4 clip takes that kernel's run-time-geometry build, whose costs are 64-bit: this case held before the 32-bit products were
    mended.  In the 32-bit builds, all 4:2:0, the chroma product of "b32-pnew256" passes 2^31 as well: 2 * 256 * 63 000 * 256.)"""
    _search_through(oracle, mv, dbg, "general", sr.PENALTY_444_CASE)


@pytest.mark.parametrize("name,bits,akw", sr.RAILS_ANALYSE_CASES, ids=_id)
def test_analyse_on_rails(oracle, mv, name, bits, akw):
    """a clip the search follows, a fifth of its samples on each rail: SADs and SATD sums of full-range differences, the rescue"""
    gp._analyse_case(oracle, mv, sr.RAILS_W, sr.RAILS_H, bits, {}, akw, frames=sr.rails(sr.RAILS_W, sr.RAILS_H, bits, 2, noise=3))


# ----------------------------------------------------------------------------------------------------------- Recalculate
@pytest.mark.parametrize("gen,rkw", [("step", dict(blksize=16, overlap=8, thsad=100)), ("step", dict(blksize=16, overlap=8, thsad=100, pnew=256)),
                                     ("rails", dict(blksize=16, overlap=8, thsad=100))], ids=_id)
def test_recalculate_at_the_rails(oracle, mv, gen, rkw):
    """32x32 vectors refined to 16x16 at 16 bits: on the step every block is above thsad and is searched again, with SADs of
    256 * 49152 = 1.26e7 -- times pnew 256 past 2^31"""
    frames = sr.step(192, 128, 16, 3, 0, 49152) if gen == "step" else sr.rails(192, 128, 16, 3, noise=3)
    gp._recalculate_case(oracle, mv, 16, dict(blksize=32, overlap=16), rkw, frames=frames)


# ------------------------------------------------------------------------------------------------- Degrain and Compensate
def _consumer_clip(gen, w, h, bits, nframes):
    if gen == "step":
        return sr.step(w, h, bits, nframes, *sr.STEP_SPAN[bits])
    return sr.make(gen, w, h, bits, nframes)


@pytest.mark.parametrize("gen,w,h,bits,radius,akw,dkw", sr.DEGRAIN_CASES, ids=_id)
def test_degrain_at_the_rails(oracle, mv, gen, w, h, bits, radius, akw, dkw):
    """weights and rounding on 0 / pm samples, s - limit < 0 and s + limit > pm (rails: vectors the search finds; checker: vectors it cannot
    find, with thresholds that keep every reference in the blend), the scene-change copy on the step; 196 wide: ragged cells"""
    gp._degrain_case(oracle, mv, w, h, bits, radius, {}, akw, dkw, frames=_consumer_clip(gen, w, h, bits, 2 * radius + 1))


@pytest.mark.parametrize("gen,w,h,bits,akw,ckw", sr.COMPENSATE_CASES, ids=_id)
def test_compensate_at_the_rails(oracle, mv, gen, w, h, bits, akw, ckw):
    gp._compensate_case(oracle, mv, w, h, bits, {}, akw, ckw, frames=_consumer_clip(gen, w, h, bits, 2))


# -------------------------------------------------------------------------------------------------------------- BlockFPS
@pytest.mark.parametrize("gen,w,h,bits,akw,bkw", sr.BLOCKFPS_CASES, ids=_id)
def test_blockfps_at_the_rails(oracle, mv, gen, w, h, bits, akw, bkw):
    gp._blockfps_case(oracle, mv, w, h, bits, akw, bkw, frames=_consumer_clip(gen, w, h, bits, 6))


# ---------------------------------------------------------------------------------------- FlowInter / FlowFPS, Flow, FlowBlur
def _flow_case(runner, consumer, mv, oracle, case):
    """one case of the Flow lists through a runner of tests/test_gpu_flow.py / tests/test_gpu_flowmc.py (byte equality of every plane of every
    output frame is the runner's); the crafted fields are built as tests/test_gpu_vector_fields.py builds them: the i-th blob the runner
    edits (the backward clip's first, then the forward clip's) gets index i"""
    gen, fmt, w, h, bits, skw, akw, fkw, recipe, kinds = case
    edit = None
    if recipe is not None:
        count, ed = itertools.count(), vf.case_editor(consumer, recipe, fkw)
        edit = lambda blob, ad: ed(blob, ad, next(count))
    got = runner(mv, oracle, fmt, w, h, bits, skw, akw, fkw, nf=sr.FLOW_NF, seed=0, edit=edit, frames=sr.flow_clip(gen, fmt, w, h, bits))
    assert got == kinds, "the case did not take what it is listed for"


@pytest.mark.parametrize("case", sr.FLOWINTER_RANGE_CASES, ids=sr.flow_case_id)
def test_flowinter_flowfps_at_the_rails(oracle, mv, case):
    """Simple, regular and Extra (at time256 128 and elsewhere), Blend and the left frame on samples of 0 and pm at 10, 12, 14 and 16 bits;
    at 16 bits on saturated masks the regular formula's 32-bit product MF * (dB * (255 - MB) + MB * dF0) + 255 on its bound, 0.992 * 2^32"""
    _flow_case(gflow._run, "flowinter", mv, oracle, case)


@pytest.mark.parametrize("case", sr.FLOW_RANGE_CASES, ids=sr.flow_case_id)
def test_flow_at_the_rails(oracle, mv, case):
    """fetch and shift; the holes of a shift are painted with the DEPTH's maximum, (1 << bits) - 1, which 10, 12 and 14 bits tell apart
    from the two-byte container's 65535"""
    _flow_case(gflowmc._run_flow, "flow", mv, oracle, case)


@pytest.mark.parametrize("case", sr.BLUR_RANGE_CASES, ids=sr.flow_case_id)
def test_flowblur_at_the_rails(oracle, mv, case):
    """sums of up to 511 samples of 0 and pm divided by their count; at 16 bits sums above 2^24"""
    _flow_case(gflowmc._run_blur, "flowblur", mv, oracle, case)
