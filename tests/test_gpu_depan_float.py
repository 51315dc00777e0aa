"""GPU parity of mv.DepanCompensate on float clips (depan_warp_kernel<float, SUB, 1> of mvx_depan_warp.hip, csrc/mvx_depan_sample_float.h) against
the CPU restatement tests/depan_float_ref.py, through the Python package: every sample of every plane as uint32, all jobs of a case in ONE
mvx_depan_compensate_frames call.  Every destination plane has a guard row before and after it and is filled with 0xA5: nothing but the
samples may change.  The cases are depan_cases' (translation with the `fractions` list, zoom, rotation with the 1e-30 rotation and the chain
past column 64, the small clip, mirror 1 / 2 / 4 / 8 / 15, blur 1 and 9, 4:2:2, 4:4:4, Gray, and the three library groups) on float32 noise
in [-0.25, 1.25), for subpixel 0, 1 and 2; tests/test_depan_float_ref.py proves the same cases on the CPU with the kernel's text compiled
for the host.  Nothing here provokes a fault: NaN and out-of-range transforms are defined behaviour (the border value).

Also here, for both float filters: one handle of each over unlike calls with the scratch as the allocator leaves it and poisoned, and planes
at odd offsets inside an arena of quiet NaNs."""
import numpy as np
import pytest

import depan_cases as dc
import depan_float_cases as fc
import depan_float_ref as fr
import depan_stab_cases as sc
from test_gpu_parity import dbg  # noqa: F401  (the fixture that puts a debug option back)

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
CASES = fc.once([c for c in dc.CASES if c["src"] == "noise"]) + dc.LIBRARY_CASES
SPECIAL = [c for c in CASES if c["name"] in ("trans_s0_8", "zoom_s0_8", "rot_s0_8", "mirror15_s0", "lib_wide_s0", "trans_s1_8", "mirror15_s1", "trans_s2_8", "zoom_s2_8",
                                             "rot_s2_8", "mirror15_s2", "blur9_s2")]


def _filter(mv, case, dev, **kw):
    f = dc.FORMATS[case["fmt"]]
    return mv.DepanCompensate(case["w"], case["h"], 32, f["subsampling"], f.get("gray", False), src_pitch=[d.stride(0) for d in dev], offset=1.0, subpixel=case["sub"],
                              mirror=case["mirror"], blur=case["blur"], sample_float=True, **kw)


def _run(mv, case, kind, tolerant=False):
    import torch
    src, want, kinds, stats = fc.expected(case, kind)
    dev = [mv.plane_to_device(p) for p in src]
    g = _filter(mv, case, dev)
    assert g.dtype == np.float32 and g.info.bits == 32
    full, out = dc.guarded(g, len(case["trs"]))
    g.run([dev] * len(case["trs"]), case["trs"], out=out)
    torch.cuda.synchronize()
    fc.check(full, want, [[(k != fr.COPY) & (k != fr.BORDER) for k in ks] for ks in kinds] if tolerant else None)
    return stats


@pytest.mark.parametrize("case", CASES, ids=dc.ids(CASES))
def test_compensate_float_parity(mv, case):
    stats = _run(mv, case, "noise")
    assert not dc.missing(case, stats), stats


@pytest.mark.parametrize("case", SPECIAL, ids=dc.ids(SPECIAL))
def test_special_values(mv, case):
    """NaNs of several payloads, +-Inf, -0.0f, denormals and large negatives in three samples of ten: every copy and every border sample bit
    for bit; where the rule computes, equal bits or a NaN on both sides (which NaN an arithmetic ends on is the hardware's)"""
    _run(mv, case, "special", tolerant=True)


def test_bicubic_overshoots_on_the_gpu_too(mv):
    case = next(c for c in dc.CASES if c["name"] == "clamp_8")
    _run(mv, case, "checker")
    _, want, _, _ = fc.expected(case, "checker")
    assert all(w[0].min() < 0 and w[0].max() > 1 for w in want)


def test_no_frames_is_a_no_op(mv):
    import torch
    g = mv.DepanCompensate(206, 118, 32, offset=1.0, sample_float=True)
    full, out = dc.guarded(g, 1)
    g.launch((mv.DepanCompensateJob * 0)())
    torch.cuda.synchronize()
    assert all(bool((t == 0xA5).all()) for t in full[0])


# ------------------------------------------------------------------------------------------------ one handle over unlike calls

POISONS = (0, 0xA5, 0x5A)


@pytest.mark.parametrize("poison", POISONS, ids=lambda v: "poison%02X" % v)
def test_one_float_handle_of_each_filter_over_unlike_calls(mv, dbg, poison):  # noqa: F811
    """rotation jobs that need chain scratch, then none, a batch that outgrows the record table, and a small one again; each call against the
    restatement.  scratch_poison fills every fresh allocation of handle-owned scratch and changes no result"""
    import torch
    dbg("scratch_poison", poison)
    case = next(c for c in dc.CASES if c["name"] == "small_s1_8")
    src = fc.source(case, "noise")
    dev = [mv.plane_to_device(p) for p in src]
    g = _filter(mv, case, dev)
    f = dc.FORMATS[case["fmt"]]
    trs = list(case["trs"])
    rots, flat = [t for t in trs if t[2] != 0], [t for t in trs if t[2] == 0]
    assert len(rots) >= 2 and len(flat) >= 2
    for batch in (rots, flat[:1], (trs * 6)[:40], rots[:1] + flat[:1], flat):
        want = [fr.compensate_frame(src, t, case["sub"], f["subsampling"], False, case["mirror"], case["blur"]) for t in batch]
        full, out = dc.guarded(g, len(batch))
        g.run([dev] * len(batch), batch, out=out)
        torch.cuda.synchronize()
        fc.check(full, want)

    scase = next(c for c in sc.CASES if c["name"] == "small_s0_8")
    frames = fc.sources(scase, "noise")
    sdev = [[mv.plane_to_device(p) for p in fr_] for fr_ in frames]
    s = mv.DepanStabilise(scase["w"], scase["h"], 32, src_pitch=[d.stride(0) for d in sdev[0]], subpixel=scase["sub"], mirror=scase["mirror"], blur=scase["blur"],
                          prev=1, next=1, num_frames=3, sample_float=True)
    jobs = list(scase["jobs"])
    rotates = [j[0][2] != 0 or bool(j[1] and j[1][1][2] != 0) or bool(j[2] and j[2][1][2] != 0) for j in jobs]
    rot_jobs, flat_jobs = [j for j, r in zip(jobs, rotates) if r], [j for j, r in zip(jobs, rotates) if not r]
    assert rot_jobs and flat_jobs
    for batch in (rot_jobs, flat_jobs[:1], (jobs * 5)[:30], flat_jobs):
        want = [fr.paint(frames[0], cur, None if prev is None else (frames[prev[0]], prev[1]), None if nxt is None else (frames[nxt[0]], nxt[1]), scase["sub"],
                         mirror=scase["mirror"], blur=scase["blur"]) for cur, nxt, prev in batch]
        n = len(batch)
        full, out = dc.guarded(s, n)
        arr, _ = s.jobs([fc.stab_plan(mv, *j) for j in batch], [sdev[0]] * n, [sdev[j[2][0]] if j[2] else None for j in batch],
                        [sdev[j[1][0]] if j[1] else None for j in batch], out=out)
        s.launch(arr)
        torch.cuda.synchronize()
        fc.check(full, want)


# ------------------------------------------------------------------------------------------------ layouts

def _carve(arena, host, off, plane, pitch):
    """put a float32 plane at byte offset off with the given pitch into the host copy; returns the device view and the next free offset"""
    h, w = plane.shape
    rows = host[off:off + h * pitch].reshape(h, pitch)
    rows[:, :w * 4] = np.ascontiguousarray(plane).view(np.uint8).reshape(h, w * 4)
    assert off % 8 == 4                                                  # an odd multiple of 4
    off2 = off + h * pitch + 12
    return arena[off:off + h * pitch].view(h, pitch), off2 + (4 if off2 % 8 == 0 else 0)


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_planes_at_odd_offsets_in_an_arena_of_quiet_nans(mv, sub):
    """source and destination planes at offsets that are odd multiples of 4, a tight luma pitch, padded chroma pitches that differ between U
    and V, all inside one arena of 0x7FC00000; afterwards the arena equals the host's copy with the expected planes written into it: every
    byte between and beyond the planes is still the NaN pattern"""
    import torch
    w, h = 70, 38
    case = dict(next(c for c in dc.CASES if c["name"] == "small_s%d_8" % sub))
    src = fc.source(case, "noise")
    trs = case["trs"][:4] + case["trs"][-2:]
    want = [fr.compensate_frame(src, t, sub, (1, 1), False, 5, 2) for t in trs]
    sp, dp = [w * 4, w // 2 * 4 + 4, w // 2 * 4 + 12], [w * 4, w // 2 * 4 + 12, w // 2 * 4 + 4]
    size = 4 + sum(p.shape[0] * q + 16 for p, q in zip(src, sp)) + len(trs) * sum(p.shape[0] * q + 16 for p, q in zip(src, dp)) + 64
    host = np.full(size // 4 + 1, 0x7FC00000, u32).view(np.uint8).copy()
    arena = torch.from_numpy(host.copy()).cuda()
    off, sdev = 4, []
    for p in range(3):
        t, off = _carve(arena, host, off, src[p], sp[p])
        sdev.append(t)
    arena.copy_(torch.from_numpy(host))                                  # the sources are in place; the destinations are NaN
    out = []
    for k in range(len(trs)):
        row = []
        for p in range(3):
            t, off = _carve(arena, host, off, want[k][p], dp[p])
            row.append(t)
        out.append(row)
    assert off <= len(host)
    g = mv.DepanCompensate(w, h, 32, src_pitch=sp, dst_pitch=dp, offset=1.0, subpixel=sub, mirror=5, blur=2, sample_float=True)
    g.run([sdev] * len(trs), trs, out=out)
    torch.cuda.synchronize()
    got = arena.cpu().numpy()
    assert np.array_equal(got, host), "first difference at byte %d" % int(np.argmax(got != host))
