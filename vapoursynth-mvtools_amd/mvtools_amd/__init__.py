"""Host-side mirror of the reference's filter interface over the C ABI of libmvtools_amd.so.

    core.mv.Super(clip, ...)            -> Super(width, height, bits, ...)       .build(frames)
    core.mv.Analyse(super, ...)         -> Analyse(super, num_frames, ...)       .run(jobs)
    core.mv.Degrain1..6(clip, super, mvbw, mvfw, ...) -> Degrain(radius, super, analysis_data, ...) .run(jobs)
    (no reference name: radius 1..24)                 -> DegrainN(radius, super, analysis_data, ..., thsad2=...) .info() .run(jobs)
    core.mv.Compensate(clip, super, vectors, ...)     -> Compensate(super, analysis_data, ...)      .run(jobs)
    (no reference name: one frame against a radius)   -> AnalyseN(super, radius, num_frames, ...)  .ad(r) .fields(multi_blob) .run(jobs)
                                                         CompensateN(tr, super, analysis_data, ...) .map(k) .run(jobs)
                                                         RecalculateN(super, analysis_data, radius, ...) .get_data(r) .run(jobs)
    (no reference name: vectors of a small clip at full size) -> ScaleVect(analysis_data, super, scale) .ad .run(blobs)
    core.mv.FlowInter / FlowFPS(clip, super, mvbw, mvfw, ...) -> FlowInter / FlowFPS(super, bw_data, fw_data, ...) .run(ns, ...)
    core.mv.Flow(clip, super, vectors, ...)           -> Flow(super, analysis_data, ...)          .run(jobs)
    core.mv.FlowBlur(clip, super, mvbw, mvfw, ...)    -> FlowBlur(super, bw_data, fw_data, ...)   .run(ns, ...)
    core.mv.Mask(clip, vectors, ...)                  -> Mask(analysis_data, width, height, ...)  .run(blobs, clip)
    core.mv.DepanAnalyse(clip, vectors, ...)          -> DepanAnalyse(analysis_data, width, height, ...) .run(blobs, masks)
    core.mv.DepanEstimate(clip, trust, winx, ...)     -> DepanEstimate(width, height, bits, ...) .spectra(frames) .correlate(prev, cur) .finish(results) .run(frames)
    core.mv.DepanCompensate(clip, data, offset, ...)  -> DepanCompensate(width, height, ..., offset=...) .map(n) .transform(motions) .run(frames, transforms)
    core.mv.DepanStabilise(clip, data, cutoff, ...)   -> DepanStabilise(width, height, ..., fps=(num, den), cutoff=...) .window(n) .plan(n, motions) .run(frames, motions)

Argument names, defaults and error strings are the reference's (MVSuper.c:279-291, MVAnalyse.c:639-671,
MVDegrains.cpp:813-932, MVCompensate.c:579-592); they are resolved inside the library, not here.
PyTorch is only plumbing: device memory (uint8 tensors, one per plane, row stride = pitch) and the HIP stream.
All pixel work happens in the hand-written HIP kernels; there is no CPU fallback -- a missing library or a missing
GPU raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.environ.get("MVX_LIB") or os.path.join(os.path.dirname(_HERE), "libmvtools_amd.so")  # MVX_LIB: developer override (A/B builds)
UNSET = -2147483648
ERRLEN = 256


class MvtoolsError(Exception):
    pass


class AnalysisData(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "nMagicKey", "nVersion", "nBlkSizeX", "nBlkSizeY", "nPel", "nLvCount", "nDeltaFrame", "isBackward", "nCPUFlags",
        "nMotionFlags", "nWidth", "nHeight", "nOverlapX", "nOverlapY", "nBlkX", "nBlkY", "bitsPerSample", "yRatioUV",
        "xRatioUV", "nHPadding", "nVPadding")]


class SuperArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "bits", "subsampling_w", "subsampling_h", "gray", "hpad", "vpad",
                                         "pel", "levels", "chroma", "sharp", "rfilter")]


class SuperInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "bits", "xRatioUV", "yRatioUV", "gray", "hpad", "vpad", "pel",
                                         "levels", "chroma", "sharp", "rfilter", "modeYUV", "super_width", "super_height",
                                         "num_planes")] + [("plane_width", C.c_int32 * 3), ("plane_height", C.c_int32 * 3)]


ANALYSE_ARGS = ("blksize", "blksizev", "levels", "search", "searchparam", "pelsearch", "isb", "lambda_", "chroma", "delta",
                "truemotion", "lsad", "plevel", "global_", "pnew", "pzero", "pglobal", "overlap", "overlapv", "divide", "badsad",
                "badrange", "opt", "meander", "trymany", "fields", "tff", "search_coarse", "dct")


class AnalyseArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ANALYSE_ARGS]


class AnalyseJob(C.Structure):
    _fields_ = [("src", C.c_void_p * 3), ("ref", C.c_void_p * 3), ("blob", C.c_void_p), ("field_shift", C.c_int32), ("reserved", C.c_int32)]


class DegrainArgs(C.Structure):
    _fields_ = [("radius", C.c_int32), ("thsad", C.c_int64), ("thsadc", C.c_int64), ("plane", C.c_int32), ("limit", C.c_int32),
                ("limitc", C.c_int32), ("thscd1", C.c_int64), ("thscd2", C.c_int32)]


class DegrainJob(C.Structure):
    _fields_ = [("src", C.c_void_p * 3), ("refs", (C.c_void_p * 3) * 12), ("blobs", C.c_void_p * 12), ("dst", C.c_void_p * 3)]


DEGRAIN_N_MAX_RADIUS = 24


class DegrainNArgs(C.Structure):
    _fields_ = [("radius", C.c_int32), ("thsad", C.c_int64), ("thsadc", C.c_int64), ("thsad2", C.c_int64), ("thsadc2", C.c_int64), ("plane", C.c_int32),
                ("limit", C.c_int32), ("limitc", C.c_int32), ("thscd1", C.c_int64), ("thscd2", C.c_int32)]


class DegrainNInfo(C.Structure):
    _fields_ = [("radius", C.c_int32), ("nrefs", C.c_int32), ("thsad_d", C.c_int64 * DEGRAIN_N_MAX_RADIUS), ("thsadc_d", C.c_int64 * DEGRAIN_N_MAX_RADIUS)]


class DegrainNJob(C.Structure):
    _fields_ = [("src", C.c_void_p * 3), ("refs", C.POINTER(C.c_void_p * 3)), ("blobs", C.POINTER(C.c_void_p)), ("dst", C.c_void_p * 3)]


class CompensateArgs(C.Structure):
    _fields_ = [("scbehavior", C.c_int32), ("thsad", C.c_int64), ("time", C.c_double), ("thscd1", C.c_int64), ("thscd2", C.c_int32),
                ("fields", C.c_int32)]


class CompensateJob(C.Structure):
    _fields_ = [("src_super", C.c_void_p * 3), ("ref_super", C.c_void_p * 3), ("blob", C.c_void_p), ("dst", C.c_void_p * 3),
                ("field_shift", C.c_int32), ("reserved", C.c_int32)]


class AnalyseNJob(C.Structure):
    _fields_ = [("src", C.c_void_p * 3), ("refs", C.POINTER(C.c_void_p * 3)), ("blob", C.c_void_p), ("field_shift", C.POINTER(C.c_int32)),
                ("field_shift_all", C.c_int32), ("reserved", C.c_int32)]


class CompensateNJob(C.Structure):
    _fields_ = [("src_super", C.c_void_p * 3), ("refs", C.POINTER(C.c_void_p * 3)), ("blob", C.c_void_p), ("field_stride", C.c_size_t),
                ("dst", C.POINTER(C.c_void_p * 3))]


RECALC_ARGS = ("thsad", "smooth", "blksize", "blksizev", "search", "searchparam", "lambda_", "chroma", "truemotion", "pnew", "overlap", "overlapv", "divide",
               "meander", "fields", "dct")


class RecalculateArgs(C.Structure):
    _fields_ = [(n, C.c_int64) for n in RECALC_ARGS]


class RecalculateJob(C.Structure):
    _fields_ = [("src", C.c_void_p * 3), ("ref", C.c_void_p * 3), ("old_blob", C.c_void_p), ("blob", C.c_void_p)]


class RecalculateNJob(C.Structure):
    _fields_ = [("src", C.c_void_p * 3), ("refs", C.POINTER(C.c_void_p * 3)), ("old_blob", C.c_void_p), ("old_field_stride", C.c_size_t),
                ("blob", C.c_void_p)]


class ScaleVectJob(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p), ("fields", C.c_int32), ("field_stride", C.c_size_t)]


class BlockFPSArgs(C.Structure):
    _fields_ = [("num", C.c_int64), ("den", C.c_int64), ("mode", C.c_int32), ("ml", C.c_double), ("blend", C.c_int32), ("thscd1", C.c_int64), ("thscd2", C.c_int32)]


class BlockFPSInfo(C.Structure):
    _fields_ = [("num_frames", C.c_int32), ("fps_num", C.c_int64), ("fps_den", C.c_int64)]


class BlockFPSJob(C.Structure):
    _fields_ = [("time256", C.c_int32), ("reserved", C.c_int32), ("src_super", C.c_void_p * 3), ("ref_super", C.c_void_p * 3), ("blob_fw", C.c_void_p),
                ("blob_bw", C.c_void_p), ("clip_left", C.c_void_p * 3), ("clip_right", C.c_void_p * 3), ("dst", C.c_void_p * 3)]


class FlowInterArgs(C.Structure):
    _fields_ = [("time", C.c_double), ("ml", C.c_double), ("blend", C.c_int32), ("thscd1", C.c_int64), ("thscd2", C.c_int32)]


class FlowFPSArgs(C.Structure):
    _fields_ = [("num", C.c_int64), ("den", C.c_int64), ("mask", C.c_int32), ("ml", C.c_double), ("blend", C.c_int32), ("thscd1", C.c_int64),
                ("thscd2", C.c_int32)]


class FlowJob(C.Structure):
    _fields_ = [("time256", C.c_int32), ("reserved", C.c_int32), ("super_left", C.c_void_p * 3), ("super_right", C.c_void_p * 3), ("blob_fw", C.c_void_p),
                ("blob_bw", C.c_void_p), ("blob_fw_extra", C.c_void_p), ("blob_bw_extra", C.c_void_p), ("clip_left", C.c_void_p * 3),
                ("clip_right", C.c_void_p * 3), ("dst", C.c_void_p * 3)]


class FlowCompArgs(C.Structure):
    _fields_ = [("time", C.c_double), ("mode", C.c_int32), ("fields", C.c_int32), ("thscd1", C.c_int64), ("thscd2", C.c_int32)]


class FlowCompJob(C.Structure):
    _fields_ = [("ref_super", C.c_void_p * 3), ("blob", C.c_void_p), ("clip", C.c_void_p * 3), ("dst", C.c_void_p * 3), ("field_shift", C.c_int32),
                ("reserved", C.c_int32)]


class FlowBlurArgs(C.Structure):
    _fields_ = [("blur", C.c_double), ("prec", C.c_int32), ("thscd1", C.c_int64), ("thscd2", C.c_int32)]


class FlowBlurJob(C.Structure):
    _fields_ = [("super", C.c_void_p * 3), ("blob_bw", C.c_void_p), ("blob_fw", C.c_void_p), ("clip", C.c_void_p * 3), ("dst", C.c_void_p * 3)]


class MaskArgs(C.Structure):
    _fields_ = [("ml", C.c_double), ("gamma", C.c_double), ("kind", C.c_int32), ("time", C.c_double), ("ysc", C.c_int32), ("thscd1", C.c_int64),
                ("thscd2", C.c_int32)]


class MaskClip(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "bits", "subsampling_w", "subsampling_h", "gray")]


class MaskInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "subsampling_w", "subsampling_h", "num_planes")] + [
        ("plane_width", C.c_int32 * 3), ("plane_height", C.c_int32 * 3), ("time256", C.c_int32), ("fMaskNormFactor", C.c_float),
        ("fMaskNormFactor2", C.c_float), ("fHalfGamma", C.c_float)]


class MaskJob(C.Structure):
    _fields_ = [("blob", C.c_void_p), ("clip_luma", C.c_void_p), ("dst", C.c_void_p * 3)]


class DepanClip(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "bits", "subsampling_w", "subsampling_h", "gray")]


class DepanCompensateArgs(C.Structure):
    _fields_ = [("offset", C.c_double), ("subpixel", C.c_int32), ("pixaspect", C.c_double), ("matchfields", C.c_int32), ("mirror", C.c_int32),
                ("blur", C.c_int32), ("fields", C.c_int32), ("tff", C.c_int32)]


class DepanCompensateInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "bits", "subsampling_w", "subsampling_h", "num_planes")] + [
        ("plane_width", C.c_int32 * 3), ("plane_height", C.c_int32 * 3), ("intoffset", C.c_int32), ("subpixel", C.c_int32), ("mirror", C.c_int32),
        ("pixel_max", C.c_int32), ("border", C.c_int32 * 3), ("blur", C.c_int32 * 3), ("xcenter", C.c_float), ("ycenter", C.c_float),
        ("offset", C.c_float), ("pixaspect", C.c_float)]


class DepanCompensateJob(C.Structure):
    _fields_ = [("src", C.c_void_p * 3), ("dst", C.c_void_p * 3), ("tr", C.c_float * 6)]


class DepanStabiliseArgs(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("cutoff", "damping", "initzoom", "dxmax", "dymax", "zoommax", "rotmax", "pixaspect", "tzoom")] + [
        (n, C.c_int32) for n in ("addzoom", "prev", "next", "mirror", "blur", "subpixel", "fitlast", "method", "fields")]


class DepanStabiliseInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "bits", "subsampling_w", "subsampling_h", "num_planes")] + [
        ("plane_width", C.c_int32 * 3), ("plane_height", C.c_int32 * 3)] + [
        (n, C.c_int32) for n in ("subpixel", "mirror", "pixel_max", "method", "prev", "next", "nfields", "radius", "wint_size", "winrz_size", "winfz_size")] + [
        ("border", C.c_int32 * 3), ("blur", C.c_int32 * 3)] + [(n, C.c_float) for n in ("fps", "freqnative", "initzoom", "zoommax", "xcenter", "ycenter")] + [
        ("nonlinfactor", C.c_float * 6)]


class DepanStabiliseSource(C.Structure):
    _fields_ = [("used", C.c_int32), ("frame", C.c_int32), ("tr", C.c_float * 6)]


class DepanStabilisePlan(C.Structure):
    _fields_ = [("tr", C.c_float * 6), ("nbase", C.c_int32), ("base", C.c_int32), ("motion", C.c_float * 4), ("prev", DepanStabiliseSource),
                ("next", DepanStabiliseSource)]


class DepanStabiliseJob(C.Structure):
    _fields_ = [("plan", DepanStabilisePlan), ("cur", C.c_void_p * 3), ("prev", C.c_void_p * 3), ("next", C.c_void_p * 3), ("dst", C.c_void_p * 3)]


class DepanAnalyseArgs(C.Structure):
    _fields_ = [("zoom", C.c_int32), ("rot", C.c_int32), ("pixaspect", C.c_double), ("error", C.c_double), ("wrong", C.c_double), ("zerow", C.c_double),
                ("thscd1", C.c_int64), ("thscd2", C.c_int32), ("fields", C.c_int32)]


class DepanMotion(C.Structure):
    _fields_ = [("dx", C.c_float), ("dy", C.c_float), ("zoom", C.c_float), ("rot", C.c_float), ("iter", C.c_int32), ("error", C.c_float)]


class DepanEstimateArgs(C.Structure):
    _fields_ = [("trust", C.c_double), ("zoommax", C.c_double), ("stab", C.c_double), ("pixaspect", C.c_double)] + [
        (n, C.c_int32) for n in ("winx", "winy", "wleft", "wtop", "dxmax", "dymax", "fields", "tff", "float_samples")]


class DepanEstimateInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("winx", "winy", "wleft", "wtop", "dxmax", "dymax", "windows")] + [("spectrum_bytes", C.c_int64)]


class DepanEstimateResult(C.Structure):
    _fields_ = [("dx", C.c_float), ("dy", C.c_float), ("zoom", C.c_float), ("trust", C.c_float)]


class DepanEstimateScan(C.Structure):
    _fields_ = [("max", C.c_float), ("sum", C.c_float), ("imax", C.c_int32), ("jmax", C.c_int32), ("xp", C.c_float), ("xm", C.c_float),
                ("yp", C.c_float), ("ym", C.c_float)]


_lib = None


def lib():
    """Loads libmvtools_amd.so (built by vapoursynth-mvtools_amd/build.py).  Fails loudly when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIBPATH):
            raise MvtoolsError("libmvtools_amd.so not built (%s): run `python vapoursynth-mvtools_amd/build.py`; "
                               "there is no CPU fallback" % _LIBPATH)
        # One HIP runtime per process: PyTorch bundles its own libamdhip64.so.7.  Importing torch first makes the
        # dynamic loader bind our DT_NEEDED libamdhip64.so.7 to that already-loaded copy instead of pulling a second
        # runtime from /opt/rocm (two HSA runtimes in one process cannot both open the device).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(_LIBPATH)
        P = C.POINTER
        L.mvx_last_error.restype = C.c_char_p
        L.mvx_version.restype = C.c_char_p
        L.mvx_super_create.argtypes = [P(SuperArgs), P(C.c_void_p), C.c_char_p]
        L.mvx_super_create_float.argtypes = L.mvx_super_create.argtypes
        L.mvx_super_is_float.argtypes = [C.c_void_p]
        L.mvx_super_destroy.argtypes = [C.c_void_p]
        L.mvx_super_get_info.argtypes = [C.c_void_p, P(SuperInfo)]
        L.mvx_super_frames.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), P(C.c_ssize_t), P(C.c_void_p), P(C.c_ssize_t), C.c_void_p]
        L.mvx_super_pelclip_mode.argtypes = [C.c_void_p, C.c_int, C.c_int, P(C.c_int32), C.c_char_p]
        L.mvx_super_frames_pelclip.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), P(C.c_ssize_t), P(C.c_void_p), P(C.c_ssize_t), C.c_int, P(C.c_void_p),
                                               P(C.c_ssize_t), C.c_void_p]
        L.mvx_super_shadow_copies.argtypes = [C.c_void_p]
        L.mvx_super_shadow_bytes.argtypes = [C.c_void_p, P(C.c_ssize_t), P(C.c_size_t)]
        L.mvx_super_shadow_bytes.restype = None
        L.mvx_super_shadow_frames.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), P(C.c_ssize_t), P(C.c_ssize_t), C.c_void_p]
        L.mvx_analyse_set_ref_shadow.argtypes = [C.c_void_p, P(C.c_ssize_t)]
        L.mvx_degrain_set_ref_shadow.argtypes = [C.c_void_p, P(C.c_ssize_t)]
        L.mvx_super_frames_shadow.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), P(C.c_ssize_t), P(C.c_void_p), P(C.c_ssize_t), P(C.c_ssize_t), C.c_void_p]
        L.mvx_debug_option.argtypes = [C.c_char_p, C.c_int]
        L.mvx_analyse_create.argtypes = [P(AnalyseArgs), C.c_void_p, C.c_int, P(C.c_ssize_t), P(C.c_void_p), C.c_char_p]
        L.mvx_analyse_destroy.argtypes = [C.c_void_p]
        L.mvx_analyse_get_data.argtypes = [C.c_void_p, P(AnalysisData)]
        L.mvx_analyse_blob_size.argtypes = [C.c_void_p]
        L.mvx_analyse_debug_level.argtypes = [C.c_void_p, C.c_int, P(C.c_int64)]
        L.mvx_analyse_frames.argtypes = [C.c_void_p, C.c_int, P(AnalyseJob), C.c_void_p]
        L.mvx_enable_dct_float.argtypes = [C.c_int]
        L.mvx_analyse_dct_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_int, P(C.c_int32), P(C.c_int32), C.c_void_p, C.c_void_p]
        L.mvx_degrain_create.argtypes = [P(DegrainArgs), P(AnalysisData), C.c_void_p, P(C.c_ssize_t), P(C.c_ssize_t), P(C.c_ssize_t),
                                         P(C.c_void_p), C.c_char_p]
        L.mvx_degrain_destroy.argtypes = [C.c_void_p]
        L.mvx_degrain_frames.argtypes = [C.c_void_p, C.c_int, P(DegrainJob), C.c_void_p]
        L.mvx_degrain_n_create.argtypes = [P(DegrainNArgs), P(AnalysisData), C.c_void_p, P(C.c_ssize_t), P(C.c_ssize_t), P(C.c_ssize_t),
                                           P(C.c_void_p), C.c_char_p]
        L.mvx_degrain_n_create_out16.argtypes = L.mvx_degrain_n_create.argtypes
        L.mvx_degrain_n_create_float.argtypes = L.mvx_degrain_n_create.argtypes
        L.mvx_degrain_n_out_bits.argtypes = [C.c_void_p]
        L.mvx_degrain_n_get_info.argtypes = [C.c_void_p, P(DegrainNInfo)]
        L.mvx_degrain_n_get_info.restype = None
        L.mvx_degrain_n_destroy.argtypes = [C.c_void_p]
        L.mvx_degrain_n_frames.argtypes = [C.c_void_p, C.c_int, P(DegrainNJob), C.c_void_p]
        L.mvx_compensate_create.argtypes = [P(CompensateArgs), P(AnalysisData), C.c_void_p, P(C.c_ssize_t), P(C.c_ssize_t),
                                            P(C.c_void_p), C.c_char_p]
        L.mvx_compensate_create_float.argtypes = L.mvx_compensate_create.argtypes
        L.mvx_compensate_destroy.argtypes = [C.c_void_p]
        L.mvx_compensate_frames.argtypes = [C.c_void_p, C.c_int, P(CompensateJob), C.c_void_p]
        L.mvx_analyse_n_create.argtypes = [P(AnalyseArgs), C.c_int, C.c_void_p, C.c_int, P(C.c_ssize_t), P(C.c_void_p), C.c_char_p]
        L.mvx_analyse_n_destroy.argtypes = [C.c_void_p]
        L.mvx_analyse_n_get_data.argtypes = [C.c_void_p, C.c_int, P(AnalysisData)]
        L.mvx_analyse_n_field_size.argtypes = [C.c_void_p]
        L.mvx_analyse_n_field_size.restype = C.c_size_t
        L.mvx_analyse_n_field_stride.argtypes = [C.c_void_p]
        L.mvx_analyse_n_field_stride.restype = C.c_size_t
        L.mvx_analyse_n_blob_size.argtypes = [C.c_void_p]
        L.mvx_analyse_n_blob_size.restype = C.c_size_t
        L.mvx_analyse_n_set_ref_shadow.argtypes = [C.c_void_p, P(C.c_ssize_t)]
        L.mvx_analyse_n_frames.argtypes = [C.c_void_p, C.c_int, P(AnalyseNJob), C.c_void_p]
        L.mvx_compensate_n_create.argtypes = [P(CompensateArgs), C.c_int, P(AnalysisData), C.c_void_p, P(C.c_ssize_t), P(C.c_ssize_t),
                                              P(C.c_void_p), C.c_char_p]
        L.mvx_compensate_n_create_float.argtypes = L.mvx_compensate_n_create.argtypes
        L.mvx_compensate_n_destroy.argtypes = [C.c_void_p]
        L.mvx_compensate_n_map.argtypes = [C.c_void_p, C.c_int, P(C.c_int), P(C.c_int)]
        L.mvx_compensate_n_frames.argtypes = [C.c_void_p, C.c_int, P(CompensateNJob), C.c_void_p]
        L.mvx_finest_size.argtypes = [C.c_void_p, P(C.c_int32), P(C.c_int32)]
        L.mvx_finest_frames.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), P(C.c_ssize_t), P(C.c_void_p), P(C.c_ssize_t), C.c_void_p]
        L.mvx_scdetect.argtypes = [P(AnalysisData), C.c_int64, C.c_int32, C.c_int, P(C.c_void_p), P(C.c_int32), C.c_void_p, C.c_char_p]
        L.mvx_recalculate_create.argtypes = [P(RecalculateArgs), C.c_void_p, P(AnalysisData), P(C.c_ssize_t), P(C.c_void_p), C.c_char_p]
        L.mvx_recalculate_destroy.argtypes = [C.c_void_p]
        L.mvx_recalculate_get_data.argtypes = [C.c_void_p, P(AnalysisData)]
        L.mvx_recalculate_blob_size.argtypes = [C.c_void_p]
        L.mvx_recalculate_frames.argtypes = [C.c_void_p, C.c_int, P(RecalculateJob), C.c_void_p]
        L.mvx_recalculate_n_create.argtypes = [P(RecalculateArgs), C.c_int, C.c_void_p, P(AnalysisData), P(C.c_ssize_t), P(C.c_void_p), C.c_char_p]
        L.mvx_recalculate_n_destroy.argtypes = [C.c_void_p]
        L.mvx_recalculate_n_get_data.argtypes = [C.c_void_p, C.c_int, P(AnalysisData)]
        for f in (L.mvx_recalculate_n_field_size, L.mvx_recalculate_n_field_stride, L.mvx_recalculate_n_blob_size):
            f.argtypes = [C.c_void_p]
            f.restype = C.c_size_t
        L.mvx_recalculate_n_frames.argtypes = [C.c_void_p, C.c_int, P(RecalculateNJob), C.c_void_p]
        L.mvx_scale_vect_create.argtypes = [P(AnalysisData), C.c_int, C.c_void_p, P(C.c_void_p), C.c_char_p]
        L.mvx_scale_vect_destroy.argtypes = [C.c_void_p]
        L.mvx_scale_vect_get_data.argtypes = [C.c_void_p, P(AnalysisData)]
        L.mvx_scale_vect_get_data.restype = None
        L.mvx_scale_vect_frames.argtypes = [C.c_void_p, C.c_int, P(ScaleVectJob), C.c_void_p]
        L.mvx_blockfps_create.argtypes = [P(BlockFPSArgs), P(AnalysisData), P(AnalysisData), C.c_void_p, C.c_int, C.c_int64, C.c_int64, P(C.c_ssize_t),
                                          P(C.c_ssize_t), P(C.c_ssize_t), P(C.c_void_p), C.c_char_p]
        L.mvx_blockfps_create_float.argtypes = L.mvx_blockfps_create.argtypes
        L.mvx_blockfps_destroy.argtypes = [C.c_void_p]
        L.mvx_blockfps_get_info.argtypes = [C.c_void_p, P(BlockFPSInfo)]
        L.mvx_blockfps_map.argtypes = [C.c_void_p, C.c_int, P(C.c_int), P(C.c_int), P(C.c_int)]
        L.mvx_blockfps_frames.argtypes = [C.c_void_p, C.c_int, P(BlockFPSJob), C.c_void_p]
        L.mvx_flowinter_create.argtypes = [P(FlowInterArgs), P(AnalysisData), P(AnalysisData), C.c_void_p, C.c_int, P(C.c_ssize_t), P(C.c_ssize_t),
                                           P(C.c_ssize_t), P(C.c_void_p), C.c_char_p]
        L.mvx_flowfps_create.argtypes = [P(FlowFPSArgs), P(AnalysisData), P(AnalysisData), C.c_void_p, C.c_int, C.c_int64, C.c_int64, P(C.c_ssize_t),
                                         P(C.c_ssize_t), P(C.c_ssize_t), P(C.c_void_p), C.c_char_p]
        L.mvx_flowinter_create_float.argtypes = L.mvx_flowinter_create.argtypes
        L.mvx_flowfps_create_float.argtypes = L.mvx_flowfps_create.argtypes
        L.mvx_flow_destroy.argtypes = [C.c_void_p]
        L.mvx_flow_get_info.argtypes = [C.c_void_p, P(BlockFPSInfo)]
        L.mvx_flow_map.argtypes = [C.c_void_p, C.c_int, P(C.c_int), P(C.c_int), P(C.c_int)]
        L.mvx_flow_frames.argtypes = [C.c_void_p, C.c_int, P(FlowJob), C.c_void_p]
        L.mvx_flowcomp_create.argtypes = [P(FlowCompArgs), P(AnalysisData), C.c_void_p, C.c_int, P(C.c_ssize_t), P(C.c_ssize_t), P(C.c_ssize_t),
                                          P(C.c_void_p), C.c_char_p]
        L.mvx_flowcomp_create_float.argtypes = L.mvx_flowcomp_create.argtypes
        L.mvx_flowcomp_destroy.argtypes = [C.c_void_p]
        L.mvx_flowcomp_ref.argtypes = [C.c_void_p, C.c_int]
        L.mvx_flowcomp_frames.argtypes = [C.c_void_p, C.c_int, P(FlowCompJob), C.c_void_p]
        L.mvx_flowblur_create.argtypes = [P(FlowBlurArgs), P(AnalysisData), P(AnalysisData), C.c_void_p, C.c_int, P(C.c_ssize_t), P(C.c_ssize_t),
                                          P(C.c_ssize_t), P(C.c_void_p), C.c_char_p]
        L.mvx_flowblur_create_float.argtypes = L.mvx_flowblur_create.argtypes
        L.mvx_flowblur_destroy.argtypes = [C.c_void_p]
        L.mvx_flowblur_frames.argtypes = [C.c_void_p, C.c_int, P(FlowBlurJob), C.c_void_p]
        L.mvx_mask_create.argtypes = [P(MaskArgs), P(AnalysisData), P(MaskClip), P(C.c_ssize_t), P(C.c_ssize_t), P(C.c_void_p), C.c_char_p]
        L.mvx_mask_create_deep.argtypes = L.mvx_mask_create.argtypes
        L.mvx_mask_out_bits.argtypes = [C.c_void_p]
        L.mvx_mask_destroy.argtypes = [C.c_void_p]
        L.mvx_mask_get_info.argtypes = [C.c_void_p, P(MaskInfo)]
        L.mvx_mask_get_info.restype = None
        L.mvx_mask_frames.argtypes = [C.c_void_p, C.c_int, P(MaskJob), C.c_void_p]
        L.mvx_depan_compensate_create.argtypes = [P(DepanCompensateArgs), P(DepanClip), C.c_int, C.c_int, P(C.c_ssize_t), P(C.c_ssize_t), P(C.c_void_p), C.c_char_p]
        L.mvx_depan_compensate_create_float.argtypes = L.mvx_depan_compensate_create.argtypes
        L.mvx_depan_compensate_destroy.argtypes = [C.c_void_p]
        L.mvx_depan_compensate_get_info.argtypes = [C.c_void_p, P(DepanCompensateInfo)]
        L.mvx_depan_compensate_get_info.restype = None
        L.mvx_depan_compensate_map.argtypes = [C.c_void_p, C.c_int, P(C.c_int), P(C.c_int), P(C.c_int)]
        L.mvx_depan_motion_to_transform.argtypes = [C.c_void_p, C.c_int, P(C.c_float), C.c_int, C.c_int, P(C.c_float), P(C.c_float), C.c_char_p]
        L.mvx_depan_compensate_frames.argtypes = [C.c_void_p, C.c_int, P(DepanCompensateJob), C.c_void_p]
        L.mvx_depan_stabilise_create.argtypes = [P(DepanStabiliseArgs), P(DepanClip), C.c_int, C.c_int, C.c_int64, C.c_int64, P(C.c_ssize_t), P(C.c_ssize_t),
                                                 P(C.c_void_p), C.c_char_p]
        L.mvx_depan_stabilise_create_float.argtypes = L.mvx_depan_stabilise_create.argtypes
        L.mvx_depan_stabilise_destroy.argtypes = [C.c_void_p]
        L.mvx_depan_stabilise_get_info.argtypes = [C.c_void_p, P(DepanStabiliseInfo)]
        L.mvx_depan_stabilise_get_info.restype = None
        L.mvx_depan_stabilise_get_windows.argtypes = [C.c_void_p, P(C.c_float), P(C.c_float), P(C.c_float)]
        L.mvx_depan_stabilise_get_windows.restype = None
        L.mvx_depan_stabilise_window.argtypes = [C.c_void_p, C.c_int, P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int)]
        L.mvx_depan_stabilise_plan.argtypes = [C.c_void_p, C.c_int, P(C.c_float), P(DepanStabilisePlan), C.c_char_p]
        L.mvx_depan_stabilise_frames.argtypes = [C.c_void_p, C.c_int, P(DepanStabiliseJob), C.c_void_p]
        L.mvx_depan_analyse_create.argtypes = [P(DepanAnalyseArgs), P(AnalysisData), P(DepanClip), P(DepanClip), C.c_int, C.c_int, C.c_int, P(C.c_void_p), C.c_char_p]
        L.mvx_depan_analyse_destroy.argtypes = [C.c_void_p]
        L.mvx_depan_analyse_frames.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), P(C.c_void_p), C.c_ssize_t, P(C.c_int32), P(DepanMotion), C.c_void_p]
        L.mvx_depan_analyse_host.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), P(C.c_void_p), C.c_ssize_t, P(C.c_int32), P(DepanMotion)]
        L.mvx_depan_estimate_create.argtypes = [P(DepanEstimateArgs), P(DepanClip), C.c_int, P(C.c_void_p), C.c_char_p]
        L.mvx_depan_estimate_destroy.argtypes = [C.c_void_p]
        L.mvx_depan_estimate_get_info.argtypes = [C.c_void_p, P(DepanEstimateInfo)]
        L.mvx_depan_estimate_get_info.restype = None
        L.mvx_depan_estimate_spectra.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), C.c_ssize_t, P(C.c_void_p), C.c_void_p]
        L.mvx_depan_estimate_correlate.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), P(C.c_void_p), P(C.c_int32), P(C.c_int32), P(DepanEstimateResult),
                                                   P(DepanEstimateScan), C.c_void_p]
        L.mvx_depan_estimate_correlate_show.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), P(C.c_void_p), P(C.c_int32), P(C.c_int32), P(DepanEstimateResult),
                                                        P(DepanEstimateScan), P(C.c_void_p), C.c_ssize_t, C.c_void_p]
        L.mvx_depan_estimate_host_tail.argtypes = [C.c_void_p, C.c_int, P(DepanEstimateScan), P(C.c_int32), P(C.c_int32), P(DepanEstimateResult)]
        L.mvx_depan_estimate_finish.argtypes = [C.c_void_p, C.c_int, P(DepanEstimateResult), P(DepanMotion)]
        L.mvx_scale_thscd.argtypes = [P(C.c_int64), P(C.c_int32), P(AnalysisData)]
        L.mvx_vectors_size.argtypes = [P(AnalysisData)]
        L.mvx_vectors_size.restype = C.c_int
        _lib = L
        # test switches: the library itself never reads the environment (mvx_debug_option is its one hook);
        # this TEST binding forwards the MVX_* variables the tools/ scripts use
        for env, opt in (("MVX_GENERAL", "general"), ("MVX_SPEC", "spec"), ("MVX_TEAM", "team")):
            if os.environ.get(env) is not None:
                L.mvx_debug_option(opt.encode(), int(os.environ[env]))
        if os.environ.get("MVX_CPW") == "1":
            L.mvx_debug_option(b"cpw1", 1)
    return _lib


def debug_option(name, value):
    """kernel-variant selection for tests / measurements (never changes results): see mvx_debug_option in mvtools_amd.h"""
    _check(lib().mvx_debug_option(name.encode(), int(value)))


_dct_float = False


def enable_dct_float(on=True):
    """dct = 1..4 of Analyse / Recalculate (the float block DCT as luma cost) are opt-in for now: process-wide, off by default
    (mvx_enable_dct_float in mvtools_amd.h).  Returns the previous setting."""
    global _dct_float
    was = _dct_float
    _check(lib().mvx_enable_dct_float(1 if on else 0))
    _dct_float = bool(on)
    return was


def _u(v):
    return UNSET if v is None else int(v)


def _check(rc, err=None):
    if rc:
        msg = err.value.decode() if err is not None and err.value else lib().mvx_last_error().decode()
        raise MvtoolsError(msg)


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise MvtoolsError("no HIP device visible: mvtools_amd has no CPU path")
    return torch


def arena_frames(n, plane_shapes, device="cuda", zero=True, slots=None):
    """n frames x len(plane_shapes) planes (rows, pitch_bytes) carved out of ONE uint8 device allocation (see Super.alloc).
    slots[p] > 1: plane p is followed by slots[p] - 1 further areas of its (256-byte rounded) size: room for the shadow planes."""
    torch = _torch()
    sizes = [r * p for r, p in plane_shapes]
    slots = slots or [1] * len(sizes)
    step = [(sz + 255) // 256 * 256 * k for sz, k in zip(sizes, slots)]
    total = n * sum(step)
    big = torch.zeros(total, dtype=torch.uint8, device=device) if zero else torch.empty(total, dtype=torch.uint8, device=device)
    out, o = [], 0
    for _ in range(n):
        row = []
        for (r, p), sz, st in zip(plane_shapes, sizes, step):
            row.append(big[o:o + sz].view(r, p))
            o += st
        out.append(row)
    return out


def _stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _pitches(planes):
    a = (C.c_ssize_t * 3)()
    for i, p in enumerate(planes):
        a[i] = p.stride(0) * p.element_size()  # bytes (planes are byte tensors everywhere but in a float clip, whose planes may be float32)
    return a


def _pad3(l):
    return (C.c_ssize_t * 3)(*(list(l) + [0] * (3 - len(l))))


def _frame_pitch(sup):
    """the default row pitch of frames of the clip's size (not the super clip's): rows rounded up to 256 bytes"""
    i = sup.info
    w = [i.width] + [i.width // i.xRatioUV] * 2
    return [((w[p] * sup.bps + 255) // 256) * 256 for p in range(sup.nplanes)]


class _Handle:
    """A library object behind self.h, destroyed with the Python object (if its creation got as far as a handle)."""
    _destroy = None  # the name of the library's destroy function

    def __del__(self):
        try:
            if self.h:
                getattr(lib(), self._destroy)(self.h)
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------- frame helpers

def plane_to_device(arr, pitch_align=256, device="cuda"):
    """numpy 2-D uint8/uint16 plane -> torch.uint8 [h, pitch] tensor (row stride = pitch bytes)."""
    torch = _torch()
    a = np.ascontiguousarray(arr)
    h, w = a.shape
    rowbytes = w * a.dtype.itemsize
    pitch = (rowbytes + pitch_align - 1) // pitch_align * pitch_align
    t = torch.zeros((h, pitch), dtype=torch.uint8, device=device)
    t[:, :rowbytes] = torch.from_numpy(a.view(np.uint8).reshape(h, rowbytes)).to(device)
    return t


def frame_to_device(planes, **kw):
    return [plane_to_device(p, **kw) for p in planes]


def plane_to_numpy(t, width, dtype):
    item = np.dtype(dtype).itemsize
    a = t[:, :width * item].contiguous().cpu().numpy()
    return a.view(dtype).reshape(t.shape[0], width)


class Super(_Handle):
    """mv.Super -- MVSuper.c:140-275.  sample_float=True with bits=32: the super clip of a float32 clip (mvx_super_create_float) -- one level, no
    shadow planes, planes of float32; DegrainN, and Compensate / CompensateN / BlockFPS / Flow / FlowBlur / FlowInter / FlowFPS with sample_float=True, consume it."""
    _destroy = "mvx_super_destroy"

    def __init__(self, width, height, bits=8, subsampling=(1, 1), gray=False, hpad=None, vpad=None, pel=None, levels=None,
                 chroma=None, sharp=None, rfilter=None, shadow=None, sample_float=False, pitch=None):
        a = SuperArgs(width, height, bits, subsampling[0], subsampling[1], int(gray), _u(hpad), _u(vpad), _u(pel), _u(levels),
                      _u(chroma), _u(sharp), _u(rfilter))
        self.h = C.c_void_p()
        err = C.create_string_buffer(ERRLEN)
        self.is_float = bool(sample_float)
        create = lib().mvx_super_create_float if self.is_float else lib().mvx_super_create
        _check(create(C.byref(a), C.byref(self.h), err), err)
        self.info = SuperInfo()
        lib().mvx_super_get_info(self.h, C.byref(self.info))
        self.dtype = np.float32 if self.is_float else np.uint8 if bits <= 8 else np.uint16
        self.bps = 4 if self.is_float else 1 if bits <= 8 else 2
        if self.is_float:
            shadow = False
        self.nplanes = self.info.num_planes
        self.pitch = [((self.info.plane_width[p] * self.bps + 255) // 256) * 256 for p in range(self.nplanes)]
        if pitch is not None:  # a caller's row pitches (bytes per plane; mvx_super_frames wants multiples of 16): alloc, the shadow planes and every consumer follow
            if len(pitch) != self.nplanes or any(q % 16 or q < self.info.plane_width[p] * self.bps for p, q in enumerate(pitch)):
                raise ValueError("Super: pitch needs %d multiples of 16 that hold a row of their plane" % self.nplanes)
            self.pitch = [int(q) for q in pitch]
        # developer experiment (r4): row pitch as a number of 128-byte lines that is odd / a given residue -- how the rows of a block and the
        # sub-pel planes spread over the sets of the CU's L1.  MVX_PITCH_LINES="odd" | "<k>" (pitch = smallest number of lines >= the row that is == k mod 64)
        _pl = os.environ.get("MVX_PITCH_LINES")
        if _pl:
            for p in range(self.nplanes):
                n = (self.info.plane_width[p] * self.bps + 127) // 128
                if _pl == "odd":
                    n += 1 - (n & 1)
                else:
                    while n % 64 != int(_pl) % 64:
                        n += 1
                self.pitch[p] = n * 128
        # shadow planes (mvx_super_shadow_frames; clips of more than 8 bits): the luma plane is followed by its copy shifted by one
        # sample, the U plane by the UV-interleaved plane, so that the search only issues dword-aligned loads.  On by default
        # (MVX_SHADOW=0 / shadow=False: the plain layout).
        if shadow is None:
            shadow = os.environ.get("MVX_SHADOW", "1") != "0"
        self.shadow_stride = [(self.info.plane_height[p] * self.pitch[p] + 255) // 256 * 256 for p in range(self.nplanes)]
        extra = (C.c_size_t * 3)()
        if shadow:
            lib().mvx_super_shadow_bytes(self.h, (C.c_ssize_t * 3)(*(self.pitch + [0] * (3 - len(self.pitch)))), extra)
        self.shadow = any(extra)
        self.slots = [1 + (extra[p] + self.shadow_stride[p] - 1) // self.shadow_stride[p] for p in range(self.nplanes)]  # areas per plane: the plane + its shadow data

    def alloc(self, n=1, device="cuda"):
        """n zero-filled super frames (the library only ever writes the defined rectangles)."""
        torch = _torch()
        # ONE allocation for all frames, planes carved at 256-byte granularity: measured +10 % search throughput on 4K16
        # against one allocation per plane (the chains of a launch touch ~20 distinct plane regions each; a single arena
        # is mapped with large page fragments and keeps the TLBs effective).  MVX_ALLOC_ARENA=0 restores per-plane tensors.
        sizes = [self.info.plane_height[p] * self.pitch[p] for p in range(self.nplanes)]
        if os.environ.get("MVX_ALLOC_ARENA", "1") == "0":
            return [[torch.zeros(self.shadow_stride[p] * self.slots[p], dtype=torch.uint8, device=device)[:self.info.plane_height[p] * self.pitch[p]].view(self.info.plane_height[p], self.pitch[p])
                     for p in range(self.nplanes)] for _ in range(n)]
        return arena_frames(n, [(self.info.plane_height[p], self.pitch[p]) for p in range(self.nplanes)], device, slots=self.slots)

    def from_host(self, planes, device="cuda"):
        """a super frame given as host arrays (numpy planes of plane_height x >= plane_width samples, e.g. from another
        implementation) -> device super frame in this object's layout, shadow copies included"""
        torch = _torch()
        fr = self.alloc(1, device=device)[0]
        for p in range(self.nplanes):
            a = np.ascontiguousarray(planes[p][:, :self.info.plane_width[p]])
            fr[p][:, :a.shape[1] * a.dtype.itemsize] = torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], -1)).to(device)
        self._shadows([fr])
        return fr

    def check_room(self, frames, what="super frame"):
        """With shadow planes the kernels write (Super) and read (Analyse) shadow_stride[p] * slots[p] bytes from every plane pointer:
        frames must come from alloc() / build() / from_host() of a Super with this layout.  A plain (height, pitch) tensor is refused
        here instead of being over-run on the device."""
        if not self.shadow:
            return
        seen = set()
        for fr in frames:
            if fr is None or id(fr) in seen:  # (a launch names every frame many times)
                continue
            seen.add(id(fr))
            for p in range(self.nplanes):
                t = fr[p]
                have = t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()
                need = self.shadow_stride[p] * self.slots[p]
                if t.stride(0) != self.pitch[p] or have < need:
                    raise ValueError("%s plane %d: pitch %d with %d bytes behind its first sample, this Super's layout needs pitch %d and %d bytes "
                                     "(the plane and its shadow planes): allocate it with Super.alloc()" % (what, p, t.stride(0), have, self.pitch[p], need))

    def _shadows(self, out):
        """fills the shifted copies behind the planes of freshly built super frames"""
        if not self.shadow:
            return
        self.check_room(out, "output super frame")
        n = len(out)
        pl = (C.c_void_p * (3 * n))()
        for f in range(n):
            for p in range(self.nplanes):
                pl[f * 3 + p] = out[f][p].data_ptr()
        _check(lib().mvx_super_shadow_frames(self.h, n, pl, _pad3(self.pitch), _pad3(self.shadow_stride), _stream()))

    def finest(self, super_frames, out=None):
        """mv.Finest(super) -- MVFinest.c: interleaved sub-pel planes of level 0, one output frame per super frame."""
        torch = _torch()
        n = len(super_frames)
        w, h = C.c_int32(), C.c_int32()
        lib().mvx_finest_size(self.h, C.byref(w), C.byref(h))
        i = self.info
        dims = [(h.value, w.value)] + [(h.value // i.yRatioUV, w.value // i.xRatioUV)] * 2
        pitch = [((dims[p][1] * self.bps + 255) // 256) * 256 for p in range(self.nplanes)]
        if out is None:
            out = arena_frames(n, [(dims[p][0], pitch[p]) for p in range(self.nplanes)], super_frames[0][0].device)
        else:  # the caller's planes, at their pitch
            pitch = [out[0][p].stride(0) for p in range(self.nplanes)]
            assert all(o[p].stride(0) == pitch[p] for o in out for p in range(self.nplanes))
        src = (C.c_void_p * (3 * n))()
        dst = (C.c_void_p * (3 * n))()
        for f in range(n):
            for p in range(self.nplanes):
                src[f * 3 + p] = super_frames[f][p].data_ptr()
                dst[f * 3 + p] = out[f][p].data_ptr()
        _check(lib().mvx_finest_frames(self.h, n, src, _pad3(self.pitch), dst, _pad3(pitch), _stream()))
        return out

    def pelclip_mode(self, pel_width, pel_height):
        """MVSuper.c:229-256: 0 = a pelclip is ignored (pel 1), 1 = plain, 2 = padded; raises on any other size."""
        mode = C.c_int32()
        err = C.create_string_buffer(ERRLEN)
        _check(lib().mvx_super_pelclip_mode(self.h, int(pel_width), int(pel_height), C.byref(mode), err), err)
        return mode.value

    def build(self, frames, out=None, pelclip=None, pelclip_size=None):
        """frames: list of device frames (list of plane tensors sharing pitches) -> list of super frames.
        pelclip: the matching frames of mv.Super's pelclip argument, pelclip_size = its (width, height)."""
        n = len(frames)
        if pelclip is not None:
            mode = self.pelclip_mode(*pelclip_size)
            if out is None:
                out = self.alloc(n, device=frames[0][0].device)
            src = (C.c_void_p * (3 * n))()
            pel = (C.c_void_p * (3 * n))()
            dst = (C.c_void_p * (3 * n))()
            for f in range(n):
                for p in range(self.nplanes):
                    src[f * 3 + p] = frames[f][p].data_ptr()
                    pel[f * 3 + p] = pelclip[f][p].data_ptr()
                    dst[f * 3 + p] = out[f][p].data_ptr()
            _check(lib().mvx_super_frames_pelclip(self.h, n, src, _pitches(frames[0]), pel, _pitches(pelclip[0]), mode, dst, _pitches(out[0]), _stream()))
            self._shadows(out)
            return out
        if out is None:
            out = self.alloc(n, device=frames[0][0].device)
        src = (C.c_void_p * (3 * n))()
        dst = (C.c_void_p * (3 * n))()
        for f in range(n):
            for p in range(self.nplanes):
                src[f * 3 + p] = frames[f][p].data_ptr()
                dst[f * 3 + p] = out[f][p].data_ptr()
                assert frames[f][p].stride(0) == frames[0][p].stride(0) and out[f][p].stride(0) == out[0][p].stride(0)
        if self.shadow:  # one call: the level-0 kernels write the shadow data of level 0 themselves
            self.check_room(out, "output super frame")
            _check(lib().mvx_super_frames_shadow(self.h, n, src, _pitches(frames[0]), dst, _pitches(out[0]), _pad3(self.shadow_stride), _stream()))
        else:
            _check(lib().mvx_super_frames(self.h, n, src, _pitches(frames[0]), dst, _pitches(out[0]), _stream()))
        return out


class Analyse(_Handle):
    """mv.Analyse -- MVAnalyse.c:267-635; keyword names are the reference's argument names."""
    _destroy = "mvx_analyse_destroy"

    def __init__(self, sup, num_frames=1 << 30, **kw):
        self.sup = sup
        a = AnalyseArgs(*([UNSET] * len(ANALYSE_ARGS)))
        for k, v in kw.items():
            k2 = {"lambda": "lambda_", "global": "global_"}.get(k, k)
            if k2 not in ANALYSE_ARGS:
                raise TypeError("Analyse: unknown argument " + k)
            if v is not None:
                setattr(a, k2, int(v))
        pitch = (C.c_ssize_t * 3)(*(sup.pitch + [0] * (3 - len(sup.pitch))))
        self.h = C.c_void_p()
        err = C.create_string_buffer(ERRLEN)
        _check(lib().mvx_analyse_create(C.byref(a), sup.h, int(num_frames), pitch, C.byref(self.h), err), err)
        self.ad = AnalysisData()
        lib().mvx_analyse_get_data(self.h, C.byref(self.ad))
        self.blob_size = lib().mvx_analyse_blob_size(self.h)
        if sup.shadow:  # super frames from sup.alloc / sup.build carry their shifted copies
            _check(lib().mvx_analyse_set_ref_shadow(self.h, (C.c_ssize_t * 3)(*(sup.shadow_stride + [0] * (3 - len(sup.shadow_stride))))))

    def alloc_blobs(self, n, device="cuda"):
        torch = _torch()
        stride = (self.blob_size + 255) // 256 * 256
        buf = torch.zeros((n, stride), dtype=torch.uint8, device=device)
        return [buf[i, :self.blob_size] for i in range(n)]

    def levels(self):
        """test hook (mvx_analyse_debug_level; no device): the search's level table, one list of 24 numbers per level, finest first"""
        out = (C.c_int64 * 24)()
        n = lib().mvx_analyse_debug_level(self.h, 0, out)
        _check(min(n, 0))
        rows = [list(out)]
        for i in range(1, n):
            _check(min(lib().mvx_analyse_debug_level(self.h, i, out), 0))
            rows.append(list(out))
        return rows

    def dct_blocks(self, plane, xs, ys):
        """test hook (dct 1..4): the device transform and quantiser on the blocks at sample xs[i], row ys[i] of a device luma plane (a uint8
        [rows, pitch] tensor, as frame_to_device / Super.build give them) -> numpy [n, blksizev, blksize] in the sample type"""
        torch = _torch()
        bw, bh, n, item = self.ad.nBlkSizeX, self.ad.nBlkSizeY, len(xs), np.dtype(self.sup.dtype).itemsize
        for x, y in zip(xs, ys):
            if not (0 <= x and (x + bw) * item <= plane.shape[1] and 0 <= y and y + bh <= plane.shape[0]):
                raise ValueError("dct_blocks: block (%d, %d) leaves the plane" % (x, y))
        out = torch.zeros((max(n, 1), bh, bw * item), dtype=torch.uint8, device=plane.device)
        ax, ay = (C.c_int32 * max(n, 1))(*xs), (C.c_int32 * max(n, 1))(*ys)
        _check(lib().mvx_analyse_dct_blocks(self.h, plane.data_ptr(), plane.stride(0), n, ax, ay, out.data_ptr(), _stream()))
        return out[:n].cpu().numpy().view(self.sup.dtype).reshape(n, bh, bw)

    def run(self, jobs, blobs=None, field_shift=0):
        """jobs: list of (src_super_frame, ref_super_frame_or_None) -> list of device blobs (MVTools_vectors)."""
        n = len(jobs)
        if blobs is None:
            blobs = self.alloc_blobs(n, device=jobs[0][0][0].device)
        arr = (AnalyseJob * n)()
        self.sup.check_room([f for job in jobs for f in job], "Analyse input")  # (the search reads the shadow planes behind every plane)
        for i, (s, r) in enumerate(jobs):
            for p in range(self.sup.nplanes):
                assert s[p].stride(0) == self.sup.pitch[p]
                arr[i].src[p] = s[p].data_ptr()
                arr[i].ref[p] = r[p].data_ptr() if r is not None else None
            arr[i].blob = blobs[i].data_ptr()
            arr[i].field_shift = field_shift
        _check(lib().mvx_analyse_frames(self.h, n, arr, _stream()))
        return blobs


def multi_refs(n, radius, num_frames):
    """the frames behind the 2 * radius fields of frame n's multi blob, in field order: n+1, n-1, n+2, n-2, ...; None outside the clip"""
    out = []
    for d in range(1, radius + 1):
        out += [m if 0 <= m < num_frames else None for m in (n + d, n - d)]
    return out


def _ref_table(jobs_refs, nr, nplanes, what):
    """the HOST table [job * nr + r][plane] behind the refs pointers of the *N jobs; a None reference stays NULL"""
    table = ((C.c_void_p * 3) * (nr * max(len(jobs_refs), 1)))()
    for i, refs in enumerate(jobs_refs):
        if len(refs) != nr:
            raise ValueError("%s: a job needs %d references" % (what, nr))
        for r, ref in enumerate(refs):
            if ref is not None:
                for p in range(nplanes):
                    table[i * nr + r][p] = ref[p].data_ptr()
    return table


class AnalyseN(_Handle):
    """One source frame against a temporal radius (include/mvtools_amd.h, "the multi blob"): field r of a multi blob is the MVTools_vectors of
    Analyse(isb = r % 2 == 0, delta = r // 2 + 1), byte for byte, at byte r * field_stride.  Keyword names are Analyse's; isb and delta are
    set by the radius."""
    _destroy = "mvx_analyse_n_destroy"

    def __init__(self, sup, radius, num_frames=1 << 30, **kw):
        self.sup = sup
        a = AnalyseArgs(*([UNSET] * len(ANALYSE_ARGS)))
        for k, v in kw.items():
            k2 = {"lambda": "lambda_", "global": "global_"}.get(k, k)
            if k2 not in ANALYSE_ARGS:
                raise TypeError("AnalyseN: unknown argument " + k)
            if v is not None:
                setattr(a, k2, int(v))
        pitch = (C.c_ssize_t * 3)(*(sup.pitch + [0] * (3 - len(sup.pitch))))
        self.h = C.c_void_p()
        err = C.create_string_buffer(ERRLEN)
        _check(lib().mvx_analyse_n_create(C.byref(a), int(radius), sup.h, int(num_frames), pitch, C.byref(self.h), err), err)
        self.radius = int(radius)
        self.field_size = lib().mvx_analyse_n_field_size(self.h)
        self.field_stride = lib().mvx_analyse_n_field_stride(self.h)
        self.blob_size = lib().mvx_analyse_n_blob_size(self.h)
        if sup.shadow:  # super frames from sup.alloc / sup.build carry their shifted copies
            _check(lib().mvx_analyse_n_set_ref_shadow(self.h, (C.c_ssize_t * 3)(*(sup.shadow_stride + [0] * (3 - len(sup.shadow_stride))))))

    def ad(self, r):
        """the MVTools_MVAnalysisData of field r"""
        out = AnalysisData()
        _check(lib().mvx_analyse_n_get_data(self.h, int(r), C.byref(out)))
        return out

    def alloc_blobs(self, n, device="cuda"):
        torch = _torch()
        buf = torch.zeros((n, self.blob_size), dtype=torch.uint8, device=device)
        return [buf[i] for i in range(n)]

    def fields(self, multi_blob):
        """the 2 * radius fields of a multi blob as tensor views: each is a blob any consumer takes"""
        return [multi_blob[r * self.field_stride:r * self.field_stride + self.field_size] for r in range(2 * self.radius)]

    def run(self, jobs, blobs=None, field_shift=0):
        """jobs: list of (src_super_frame, [ref_super_frame or None] * 2r in the order of multi_refs) -> list of multi blobs on the device.
        field_shift: one value, or per job a list of 2r."""
        n, nr = len(jobs), 2 * self.radius
        if blobs is None:
            blobs = self.alloc_blobs(n, device=jobs[0][0][0].device)
        self.sup.check_room([f for s, refs in jobs for f in [s] + list(refs)], "AnalyseN input")  # (the search reads the shadow planes behind every plane)
        arr = (AnalyseNJob * n)()
        table = _ref_table([refs for _, refs in jobs], nr, self.sup.nplanes, "AnalyseN")
        shifts = (C.c_int32 * (nr * n))()
        for i, (s, refs) in enumerate(jobs):
            for p in range(self.sup.nplanes):
                assert s[p].stride(0) == self.sup.pitch[p]
                arr[i].src[p] = s[p].data_ptr()
            arr[i].refs = C.cast(C.byref(table, i * nr * C.sizeof(C.c_void_p * 3)), C.POINTER(C.c_void_p * 3))
            if blobs[i].numel() < self.blob_size:
                raise ValueError("AnalyseN: a multi blob holds %d bytes" % self.blob_size)
            arr[i].blob = blobs[i].data_ptr()
            if isinstance(field_shift, int):
                arr[i].field_shift_all = field_shift
            else:
                shifts[i * nr:(i + 1) * nr] = [int(v) for v in field_shift[i]]
                arr[i].field_shift = C.cast(C.byref(shifts, i * nr * 4), C.POINTER(C.c_int32))
        _check(lib().mvx_analyse_n_frames(self.h, n, arr, _stream()))
        return blobs


class Degrain(_Handle):
    """mv.Degrain1..6 -- MVDegrains.cpp:511-809.  analysis_data = the vector clips' MVTools_MVAnalysisData."""
    _destroy = "mvx_degrain_destroy"

    def __init__(self, radius, sup, analysis_data, src_pitch, dst_pitch=None, thsad=None, thsadc=None, plane=None, limit=None,
                 limitc=None, thscd1=None, thscd2=None):
        self.sup = sup
        self.radius = radius
        a = DegrainArgs(radius, _u(thsad), _u(thsadc), _u(plane), _u(limit), _u(limitc), _u(thscd1), _u(thscd2))
        ad = AnalysisData.from_buffer_copy(bytes(analysis_data))
        dst_pitch = dst_pitch or src_pitch
        self.h = C.c_void_p()
        err = C.create_string_buffer(ERRLEN)
        _check(lib().mvx_degrain_create(C.byref(a), C.byref(ad), sup.h, _pad3(src_pitch), _pad3(sup.pitch), _pad3(dst_pitch), C.byref(self.h), err), err)
        self.src_pitch, self.dst_pitch = list(src_pitch), list(dst_pitch)
        self.ref_shadow = bool(sup.shadow and sup.slots[0] > 1)
        if self.ref_shadow:  # super frames from sup.alloc / sup.build carry the shifted copy of their luma plane (clips of more than 8 bits)
            _check(lib().mvx_degrain_set_ref_shadow(self.h, (C.c_ssize_t * 3)(*(sup.shadow_stride + [0] * (3 - len(sup.shadow_stride))))))

    def run(self, jobs, out=None):
        """jobs: list of (src_frame, [ref_super or None]*2r, [blob]*2r) ordered mvbw, mvfw, mvbw2, mvfw2, ..."""
        torch = _torch()
        n = len(jobs)
        if out is None:
            out = [[torch.empty_like(p) for p in j[0]] for j in jobs]
        arr = (DegrainJob * n)()
        if self.ref_shadow:  # (blocks at odd sample positions are read from the shifted luma copy BEHIND every reference plane: a plain tensor would be over-run)
            self.sup.check_room([r for _, refs, _ in jobs for r in refs], "Degrain reference")
        for i, (src, refs, blobs) in enumerate(jobs):
            for p in range(self.sup.nplanes):
                assert src[p].stride(0) == self.src_pitch[p] and out[i][p].stride(0) == self.dst_pitch[p]
                arr[i].src[p] = src[p].data_ptr()
                arr[i].dst[p] = out[i][p].data_ptr()
            for r in range(2 * self.radius):
                if refs[r] is not None:
                    for p in range(self.sup.nplanes):
                        arr[i].refs[r][p] = refs[r][p].data_ptr()
                arr[i].blobs[r] = blobs[r].data_ptr()
        _check(lib().mvx_degrain_frames(self.h, n, arr, _stream()))
        return out


class DegrainN(_Handle):
    """Degrain at a temporal radius of 1..24 (include/mvtools_amd.h, mv.DegrainN): the reference's templates over the radius (MVDegrains.h:30-53,184-223)
    read at any radius, each reference weighed against the threshold of its temporal distance -- thsad at distance 1 falling to thsad2 at distance
    `radius` (thsad2 / thsadc2 None: no fall-off).  analysis_data = the vector clips' MVTools_MVAnalysisData.
    out16: an 8-bit clip (8-bit super clip and vectors, thresholds in 8-bit units) written as 16-bit planes -- a block's weighted sum before its
    >> 8, see mvx_degrain_n_create_out16; limit / limitc are then 0..65535, and dst_pitch defaults to rows of 16-bit samples rounded up to 256 bytes.
    A float super clip (Super(..., bits=32, sample_float=True)) selects mvx_degrain_n_create_float: float32 clip, super clip and output, vectors and
    thresholds from a search on an 8..16 bit copy, limit / limitc on the 8-bit scale 0..255; out16 with it is refused by the library."""
    _destroy = "mvx_degrain_n_destroy"

    def __init__(self, radius, sup, analysis_data, src_pitch, dst_pitch=None, thsad=None, thsadc=None, thsad2=None, thsadc2=None, plane=None, limit=None,
                 limitc=None, thscd1=None, thscd2=None, out16=False):
        self.sup = sup
        self.radius = radius
        self.out16 = bool(out16)
        self.is_float = bool(getattr(sup, "is_float", False))
        a = DegrainNArgs(radius, _u(thsad), _u(thsadc), _u(thsad2), _u(thsadc2), _u(plane), _u(limit), _u(limitc), _u(thscd1), _u(thscd2))
        ad = AnalysisData.from_buffer_copy(bytes(analysis_data))
        if self.out16:
            dst_pitch = dst_pitch or [(sup.info.plane_width[p] * 2 + 255) // 256 * 256 for p in range(len(src_pitch))]
        dst_pitch = dst_pitch or src_pitch
        self.h = C.c_void_p()
        err = C.create_string_buffer(ERRLEN)
        create = lib().mvx_degrain_n_create_out16 if self.out16 else lib().mvx_degrain_n_create_float if self.is_float else lib().mvx_degrain_n_create
        _check(create(C.byref(a), C.byref(ad), sup.h, _pad3(src_pitch), _pad3(sup.pitch), _pad3(dst_pitch), C.byref(self.h), err), err)
        self.src_pitch, self.dst_pitch = list(src_pitch), list(dst_pitch)

    @property
    def out_bits(self):
        """bits per sample of the planes run() writes: 16 with out16, 32 for a float clip, else the clip's depth"""
        return lib().mvx_degrain_n_out_bits(self.h)

    def info(self):
        """what creation resolved: dict(radius, nrefs, thsad_d, thsadc_d) -- the thresholds per distance 1..radius after the block-size scaling"""
        i = DegrainNInfo()
        lib().mvx_degrain_n_get_info(self.h, C.byref(i))
        return dict(radius=i.radius, nrefs=i.nrefs, thsad_d=list(i.thsad_d[:i.radius]), thsadc_d=list(i.thsadc_d[:i.radius]))

    def run(self, jobs, out=None):
        """jobs: list of (src_frame, [ref_super or None]*2r, [blob]*2r) ordered mvbw, mvfw, mvbw2, mvfw2, ...; in place of the list of blobs a job
        may carry ONE multi blob (AnalyseN.run): a tensor of 2r * field_stride bytes whose field r is blob r"""
        torch = _torch()
        n, nr = len(jobs), 2 * self.radius
        if out is None and self.out16:
            out = [[torch.empty((p.shape[0], self.dst_pitch[i]), dtype=torch.uint8, device=p.device) for i, p in enumerate(j[0])] for j in jobs]
        if out is None:
            out = [[torch.empty_like(p) for p in j[0]] for j in jobs]
        arr = (DegrainNJob * n)()
        refs_all, blobs_all = ((C.c_void_p * 3) * (nr * n))(), (C.c_void_p * (nr * n))()  # the host tables behind the jobs' pointers
        for i, (src, refs, blobs) in enumerate(jobs):
            multi = blobs if hasattr(blobs, "data_ptr") else None
            if multi is not None:  # the fields of a multi blob: base + r * stride
                if multi.dim() != 1 or multi.numel() % (256 * nr):
                    raise ValueError("DegrainN: a multi blob is a one-dimensional tensor of %d fields, each a multiple of 256 bytes" % nr)
                blobs = [multi[r * (multi.numel() // nr):] for r in range(nr)]
            if len(refs) != nr or len(blobs) != nr:
                raise ValueError("DegrainN: a job needs %d references and blobs" % nr)
            for p in range(self.sup.nplanes):
                assert src[p].stride(0) * src[p].element_size() == self.src_pitch[p] and out[i][p].stride(0) * out[i][p].element_size() == self.dst_pitch[p]
                arr[i].src[p] = src[p].data_ptr()
                arr[i].dst[p] = out[i][p].data_ptr()
            for r in range(nr):
                if refs[r] is not None:
                    for p in range(self.sup.nplanes):
                        refs_all[i * nr + r][p] = refs[r][p].data_ptr()
                blobs_all[i * nr + r] = blobs[r].data_ptr() if blobs[r] is not None else None
            arr[i].refs = C.cast(C.byref(refs_all, i * nr * C.sizeof(C.c_void_p * 3)), C.POINTER(C.c_void_p * 3))
            arr[i].blobs = C.cast(C.byref(blobs_all, i * nr * C.sizeof(C.c_void_p)), C.POINTER(C.c_void_p))
        _check(lib().mvx_degrain_n_frames(self.h, n, arr, _stream()))
        return out


def _out_plane(torch, rows, pitch, is_float, device):
    """a zeroed output plane of `rows` rows of `pitch` bytes: bytes, or float32 samples for a float filter (whose pitches are multiples of 4)"""
    if is_float:
        return torch.zeros((rows, pitch // 4), dtype=torch.float32, device=device)
    return torch.zeros((rows, pitch), dtype=torch.uint8, device=device)


class Compensate(_Handle):
    """mv.Compensate -- MVCompensate.c:419-575.  sample_float=True selects mvx_compensate_create_float: a float super clip
    (Super(..., bits=32, sample_float=True)), float32 output planes, vectors and thresholds from a search on an 8..16 bit copy; fields is refused.
    The keyword is explicit: a float super clip without it is refused like by every filter that has no float path."""
    _destroy = "mvx_compensate_destroy"

    def __init__(self, sup, analysis_data, dst_pitch=None, scbehavior=None, thsad=None, time=100.0, thscd1=None, thscd2=None, fields=None, sample_float=False):
        self.sup = sup
        self.is_float = bool(sample_float)
        a = CompensateArgs(_u(scbehavior), _u(thsad), float(time), _u(thscd1), _u(thscd2), _u(fields))
        ad = AnalysisData.from_buffer_copy(bytes(analysis_data))
        if dst_pitch is None:
            dst_pitch = _frame_pitch(sup)
        self.h = C.c_void_p()
        err = C.create_string_buffer(ERRLEN)
        create = lib().mvx_compensate_create_float if self.is_float else lib().mvx_compensate_create
        _check(create(C.byref(a), C.byref(ad), sup.h, _pad3(sup.pitch), _pad3(dst_pitch), C.byref(self.h), err), err)
        self.dst_pitch = list(dst_pitch)

    def run(self, jobs, out=None):
        """jobs: list of (src_super, ref_super_or_None, blob[, field_shift])."""
        torch = _torch()
        i = self.sup.info
        n = len(jobs)
        hs = [i.height] + [i.height // i.yRatioUV] * 2
        if out is None:
            dev = jobs[0][0][0].device
            out = [[_out_plane(torch, hs[p], self.dst_pitch[p], self.is_float, dev) for p in range(self.sup.nplanes)] for _ in range(n)]
        arr = (CompensateJob * n)()
        for k, job in enumerate(jobs):
            s, r, blob = job[:3]
            for p in range(self.sup.nplanes):
                arr[k].src_super[p] = s[p].data_ptr()
                arr[k].ref_super[p] = r[p].data_ptr() if r is not None else None
                arr[k].dst[p] = out[k][p].data_ptr()
            arr[k].blob = blob.data_ptr()
            arr[k].field_shift = int(job[3]) if len(job) > 3 else 0
        _check(lib().mvx_compensate_frames(self.h, n, arr, _stream()))
        return out


class CompensateN(_Handle):
    """The frames n - tr .. n + tr compensated onto frame n from frame n's multi blob (include/mvtools_amd.h, mv.CompensateN): 2 * tr + 1 frames
    per job in temporal order, each compensated one byte for byte what Compensate writes for that pair, the source in the middle.
    analysis_data: of field 0 (AnalyseN.ad(0)).  sample_float=True selects mvx_compensate_n_create_float, as in Compensate: float super clip,
    float32 output planes, the multi blob of a search on an 8..16 bit copy."""
    _destroy = "mvx_compensate_n_destroy"

    def __init__(self, tr, sup, analysis_data, dst_pitch=None, scbehavior=None, thsad=None, time=100.0, thscd1=None, thscd2=None, fields=None, sample_float=False):
        self.sup = sup
        self.is_float = bool(sample_float)
        a = CompensateArgs(_u(scbehavior), _u(thsad), float(time), _u(thscd1), _u(thscd2), _u(fields))
        ad = AnalysisData.from_buffer_copy(bytes(analysis_data))
        if dst_pitch is None:
            dst_pitch = _frame_pitch(sup)
        self.h = C.c_void_p()
        err = C.create_string_buffer(ERRLEN)
        create = lib().mvx_compensate_n_create_float if self.is_float else lib().mvx_compensate_n_create
        _check(create(C.byref(a), int(tr), C.byref(ad), sup.h, _pad3(sup.pitch), _pad3(dst_pitch), C.byref(self.h), err), err)
        self.tr = int(tr)
        self.dst_pitch = list(dst_pitch)

    def map(self, k):
        """output k of a job -> (offset of its frame from n, field of the multi blob that compensates it or -1 for the centre)"""
        off, field = C.c_int(), C.c_int()
        _check(lib().mvx_compensate_n_map(self.h, int(k), C.byref(off), C.byref(field)))
        return off.value, field.value

    def run(self, jobs, out=None):
        """jobs: list of (src_super, [ref_super or None] * 2tr in the order of multi_refs, multi blob[, field_stride]) -> per job 2tr + 1 frames.
        field_stride defaults to the blob's bytes / 2tr (a blob of AnalyseN.alloc_blobs)."""
        torch = _torch()
        i = self.sup.info
        n, nr, no, npl = len(jobs), 2 * self.tr, 2 * self.tr + 1, self.sup.nplanes
        hs = [i.height] + [i.height // i.yRatioUV] * 2
        if out is None:
            dev = jobs[0][0][0].device
            out = [[[_out_plane(torch, hs[p], self.dst_pitch[p], self.is_float, dev) for p in range(npl)] for _ in range(no)] for _ in range(n)]
        arr = (CompensateNJob * n)()
        table = _ref_table([job[1] for job in jobs], nr, npl, "CompensateN")
        dst = ((C.c_void_p * 3) * (no * n))()
        for j, job in enumerate(jobs):
            s, blob = job[0], job[2]
            if len(out[j]) != no:
                raise ValueError("CompensateN: a job writes %d frames" % no)
            for p in range(npl):
                arr[j].src_super[p] = s[p].data_ptr()
                for k in range(no):
                    assert out[j][k][p].stride(0) * out[j][k][p].element_size() == self.dst_pitch[p]
                    dst[j * no + k][p] = out[j][k][p].data_ptr()
            arr[j].refs = C.cast(C.byref(table, j * nr * C.sizeof(C.c_void_p * 3)), C.POINTER(C.c_void_p * 3))
            arr[j].dst = C.cast(C.byref(dst, j * no * C.sizeof(C.c_void_p * 3)), C.POINTER(C.c_void_p * 3))
            arr[j].blob = blob.data_ptr()
            arr[j].field_stride = int(job[3]) if len(job) > 3 else blob.numel() // nr
        _check(lib().mvx_compensate_n_frames(self.h, n, arr, _stream()))
        return out


class BlockFPS(_Handle):
    """mv.BlockFPS(clip, super, mvbw, mvfw, num, den, mode, ml, blend, thscd1, thscd2) -- MVBlockFPS.c:741-1014.
    `fps_num / fps_den` is the input clip's frame rate; `clip_pitch` the row pitch of its device planes.  sample_float=True selects
    mvx_blockfps_create_float: a float super clip (Super(..., bits=32, sample_float=True)), float32 clip and output planes, vectors, thresholds
    and ml from a search on an 8..16 bit copy.  The keyword is explicit: a float super clip without it is refused."""
    _destroy = "mvx_blockfps_destroy"

    def __init__(self, sup, ad_bw, ad_fw, num_frames, clip_pitch, fps_num=24, fps_den=1, num=None, den=None, mode=None, ml=100.0, blend=None, thscd1=None,
                 thscd2=None, dst_pitch=None, sample_float=False):
        self.sup = sup
        self.is_float = bool(sample_float)
        a = BlockFPSArgs(_u(num), _u(den), _u(mode), float(ml), _u(blend), _u(thscd1), _u(thscd2))
        bw = AnalysisData.from_buffer_copy(bytes(ad_bw))
        fw = AnalysisData.from_buffer_copy(bytes(ad_fw))
        self.h = C.c_void_p()
        self.pitch = list(clip_pitch)
        err = C.create_string_buffer(ERRLEN)
        create = lib().mvx_blockfps_create_float if self.is_float else lib().mvx_blockfps_create
        self.dst_pitch = list(dst_pitch or clip_pitch)
        _check(create(C.byref(a), C.byref(bw), C.byref(fw), sup.h, int(num_frames), int(fps_num), int(fps_den), _pad3(sup.pitch), _pad3(clip_pitch),
                      _pad3(self.dst_pitch), C.byref(self.h), err), err)
        self.in_frames = int(num_frames)
        info = BlockFPSInfo()
        lib().mvx_blockfps_get_info(self.h, C.byref(info))
        self.num_frames, self.fps_num, self.fps_den = info.num_frames, info.fps_num, info.fps_den

    def map(self, n):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        lib().mvx_blockfps_map(self.h, n, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def run(self, frames_out, clip, supers, blobs_bw, blobs_fw, out=None):
        """frames_out: output frame numbers; clip / supers: device frames of the input clip and its super clip; blobs_*: per
        input frame device blobs of the two vector clips (mvbw at n, mvfw at n)."""
        torch = _torch()
        n = len(frames_out)
        if out is None and self.is_float:
            out = [[_out_plane(torch, clip[0][p].shape[0], self.dst_pitch[p], True, clip[0][0].device) for p in range(self.sup.nplanes)] for _ in range(n)]
        elif out is None:
            out = arena_frames(n, [tuple(p.shape) for p in clip[0]], clip[0][0].device, zero=False)
        arr = (BlockFPSJob * n)()
        last = self.in_frames - 1
        for k, fo in enumerate(frames_out):
            nl, nr, t = self.map(fo)
            arr[k].time256 = t
            good = nl < self.in_frames and nr < self.in_frames
            L, R = clip[min(nl, last)], clip[min(nr, last)]
            for p in range(self.sup.nplanes):
                arr[k].clip_left[p] = L[p].data_ptr()
                arr[k].clip_right[p] = R[p].data_ptr()
                arr[k].dst[p] = out[k][p].data_ptr()
                if good:
                    arr[k].src_super[p] = supers[nl][p].data_ptr()
                    arr[k].ref_super[p] = supers[nr][p].data_ptr()
            if good:
                arr[k].blob_fw = blobs_fw[nr].data_ptr()
                arr[k].blob_bw = blobs_bw[nl].data_ptr()
        _check(lib().mvx_blockfps_frames(self.h, n, arr, _stream()))
        return out


class _Flow(_Handle):
    """the engine both flow filters share (mvx_flow_*); subclasses create the handle"""
    _destroy = "mvx_flow_destroy"

    def __init__(self, sup, num_frames, create, dst_pitch, sample_float):
        self.sup = sup
        self.is_float = bool(sample_float)
        self.dst_pitch = list(dst_pitch)
        self.h = C.c_void_p()
        err = C.create_string_buffer(ERRLEN)
        _check(create(C.byref(self.h), err), err)
        self.in_frames = int(num_frames)
        info = BlockFPSInfo()
        lib().mvx_flow_get_info(self.h, C.byref(info))
        self.num_frames, self.fps_num, self.fps_den = info.num_frames, info.fps_num, info.fps_den

    def map(self, n):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        lib().mvx_flow_map(self.h, n, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def run(self, ns, clip, supers, blobs_bw, blobs_fw, out=None):
        """ns: output frame numbers, one job each, all in one call; clip / supers: device frames of the input clip and its super clip;
        blobs_bw / blobs_fw: per input frame device blobs of the two vector clips (mvbw at n, mvfw at n).  The main vectors are mvbw at
        nleft and mvfw at nright, the extra ones mvfw at nleft and mvbw at nright."""
        arr, out = self.jobs(ns, clip, supers, blobs_bw, blobs_fw, out)
        self.launch(arr)
        return out

    def launch(self, arr):
        """enqueues a job table made by jobs()"""
        _check(lib().mvx_flow_frames(self.h, len(arr), arr, _stream()))

    def jobs(self, ns, clip, supers, blobs_bw, blobs_fw, out=None):
        """the job table of run() and its output frames, without launching"""
        torch = _torch()
        n = len(ns)
        if out is None:
            out = _flow_out(torch, self, n, clip[0])
        arr = (FlowJob * n)()
        last = self.in_frames - 1
        for k, fo in enumerate(ns):
            nl, nr, t = self.map(fo)
            arr[k].time256 = t
            L, R = clip[min(nl, last)], clip[min(nr, last)]
            for p in range(self.sup.nplanes):
                arr[k].clip_left[p] = L[p].data_ptr()
                arr[k].clip_right[p] = R[p].data_ptr()
                arr[k].dst[p] = out[k][p].data_ptr()
            if nl < self.in_frames and nr < self.in_frames:
                for p in range(self.sup.nplanes):
                    arr[k].super_left[p] = supers[nl][p].data_ptr()
                    arr[k].super_right[p] = supers[nr][p].data_ptr()
                arr[k].blob_fw = blobs_fw[nr].data_ptr()
                arr[k].blob_bw = blobs_bw[nl].data_ptr()
                arr[k].blob_fw_extra = blobs_fw[nl].data_ptr()
                arr[k].blob_bw_extra = blobs_bw[nr].data_ptr()
        return arr, out


class FlowInter(_Flow):
    """mv.FlowInter(clip, super, mvbw, mvfw, time, ml, blend, thscd1, thscd2) -- MVFlowInter.c:473-678.  Output frame n lies `time` percent
    of the way from input frame n to n + delta; `clip_pitch` is the row pitch of the clip's device planes (and of the output).  sample_float=True
    selects mvx_flowinter_create_float: a float super clip (Super(..., bits=32, sample_float=True)), float32 clip and output planes, vectors,
    thresholds and ml from a search on an 8..16 bit copy; the vectors, masks and fetch positions are the integer filter's, the samples are
    mixed in float32.  The keyword is explicit: a float super clip without it is refused."""

    def __init__(self, sup, ad_bw, ad_fw, num_frames, clip_pitch, time=50.0, ml=100.0, blend=None, thscd1=None, thscd2=None, dst_pitch=None,
                 sample_float=False):
        a = FlowInterArgs(float(time), float(ml), _u(blend), _u(thscd1), _u(thscd2))
        bw = AnalysisData.from_buffer_copy(bytes(ad_bw))
        fw = AnalysisData.from_buffer_copy(bytes(ad_fw))
        dst_pitch = list(dst_pitch or clip_pitch)
        create = lib().mvx_flowinter_create_float if sample_float else lib().mvx_flowinter_create
        super().__init__(sup, num_frames, lambda h, err: create(C.byref(a), C.byref(bw), C.byref(fw), sup.h, int(num_frames), _pad3(sup.pitch),
                                                                _pad3(clip_pitch), _pad3(dst_pitch), h, err), dst_pitch, sample_float)


class FlowFPS(_Flow):
    """mv.FlowFPS(clip, super, mvbw, mvfw, num, den, mask, ml, blend, thscd1, thscd2) -- MVFlowFPS.c:565-878.  `fps_num / fps_den` is the
    input clip's frame rate; `clip_pitch` the row pitch of its device planes (and of the output).  sample_float=True selects
    mvx_flowfps_create_float, as in FlowInter: float super clip, float32 clip and output planes; frames at time256 0 / 256 are copied bit for bit."""

    def __init__(self, sup, ad_bw, ad_fw, num_frames, clip_pitch, fps_num=24, fps_den=1, num=None, den=None, mask=None, ml=100.0, blend=None, thscd1=None,
                 thscd2=None, dst_pitch=None, sample_float=False):
        a = FlowFPSArgs(_u(num), _u(den), _u(mask), float(ml), _u(blend), _u(thscd1), _u(thscd2))
        bw = AnalysisData.from_buffer_copy(bytes(ad_bw))
        fw = AnalysisData.from_buffer_copy(bytes(ad_fw))
        dst_pitch = list(dst_pitch or clip_pitch)
        create = lib().mvx_flowfps_create_float if sample_float else lib().mvx_flowfps_create
        super().__init__(sup, num_frames, lambda h, err: create(C.byref(a), C.byref(bw), C.byref(fw), sup.h, int(num_frames), int(fps_num), int(fps_den),
                                                                _pad3(sup.pitch), _pad3(clip_pitch), _pad3(dst_pitch), h, err), dst_pitch, sample_float)


def _flow_out(torch, flt, n, frame):
    """n output frames like the clip frame `frame` for the flow filters: float32 planes of the filter's dst pitch for a float filter"""
    if flt.is_float:
        return [[_out_plane(torch, frame[p].shape[0], flt.dst_pitch[p], True, frame[0].device) for p in range(flt.sup.nplanes)] for _ in range(n)]
    return arena_frames(n, [tuple(p.shape) for p in frame], frame[0].device, zero=False)


class Flow(_Handle):
    """mv.Flow(clip, super, vectors, time, mode, fields, thscd1, thscd2, tff) -- MVFlow.cpp:391-593.  Output frame n is clip frame n compensated
    per sample from the Finest frame of ref(n); `clip_pitch` is the row pitch of the clip's device planes (and of the output).  sample_float=True
    selects mvx_flowcomp_create_float: a float super clip (Super(..., bits=32, sample_float=True)), float32 clip and output planes, vectors and
    thresholds from a search on an 8..16 bit copy; samples are moved bit for bit, fields is refused.  The keyword is explicit: a float super
    clip without it is refused."""
    _destroy = "mvx_flowcomp_destroy"

    def __init__(self, sup, ad, num_frames, clip_pitch, time=100.0, mode=None, fields=None, thscd1=None, thscd2=None, dst_pitch=None, sample_float=False):
        self.sup = sup
        self.is_float = bool(sample_float)
        a = FlowCompArgs(float(time), _u(mode), _u(fields), _u(thscd1), _u(thscd2))
        ad = AnalysisData.from_buffer_copy(bytes(ad))
        self.h = C.c_void_p()
        self.pitch = list(clip_pitch)
        self.num_frames = int(num_frames)
        err = C.create_string_buffer(ERRLEN)
        create = lib().mvx_flowcomp_create_float if self.is_float else lib().mvx_flowcomp_create
        self.dst_pitch = list(dst_pitch or clip_pitch)
        _check(create(C.byref(a), C.byref(ad), sup.h, self.num_frames, _pad3(sup.pitch), _pad3(clip_pitch), _pad3(self.dst_pitch), C.byref(self.h), err), err)

    def ref(self, n):
        """the reference frame of output frame n (MVFlow.cpp:170-176); outside the clip the job passes no super frame"""
        return lib().mvx_flowcomp_ref(self.h, int(n))

    def run(self, jobs, out=None):
        """jobs: list of (clip_frame, ref_super_or_None, blob[, field_shift]); None or a blob of None copies the clip frame"""
        torch = _torch()
        n = len(jobs)
        if out is None:
            out = _flow_out(torch, self, n, jobs[0][0])
        arr = (FlowCompJob * n)()
        for k, job in enumerate(jobs):
            clip, r, blob = job[:3]
            for p in range(self.sup.nplanes):
                arr[k].clip[p] = clip[p].data_ptr()
                arr[k].dst[p] = out[k][p].data_ptr()
                arr[k].ref_super[p] = r[p].data_ptr() if r is not None else None
            arr[k].blob = blob.data_ptr() if blob is not None else None
            arr[k].field_shift = int(job[3]) if len(job) > 3 else 0
        self.launch(arr)
        return out

    def launch(self, arr):
        """enqueues a job table (a ctypes array of FlowCompJob)"""
        _check(lib().mvx_flowcomp_frames(self.h, len(arr), arr, _stream()))


class FlowBlur(_Handle):
    """mv.FlowBlur(clip, super, mvbw, mvfw, blur, prec, thscd1, thscd2) -- MVFlowBlur.c:346-552.  `clip_pitch` is the row pitch of the clip's
    device planes (and of the output).  sample_float=True selects mvx_flowblur_create_float, as in Flow: float super clip, float32 clip and
    output planes, the taps summed in float32 one by one and divided once."""
    _destroy = "mvx_flowblur_destroy"

    def __init__(self, sup, ad_bw, ad_fw, num_frames, clip_pitch, blur=50.0, prec=None, thscd1=None, thscd2=None, dst_pitch=None, sample_float=False):
        self.sup = sup
        self.is_float = bool(sample_float)
        a = FlowBlurArgs(float(blur), _u(prec), _u(thscd1), _u(thscd2))
        bw = AnalysisData.from_buffer_copy(bytes(ad_bw))
        fw = AnalysisData.from_buffer_copy(bytes(ad_fw))
        self.h = C.c_void_p()
        self.pitch = list(clip_pitch)
        self.num_frames = int(num_frames)
        self.delta = bw.nDeltaFrame
        err = C.create_string_buffer(ERRLEN)
        create = lib().mvx_flowblur_create_float if self.is_float else lib().mvx_flowblur_create
        self.dst_pitch = list(dst_pitch or clip_pitch)
        _check(create(C.byref(a), C.byref(bw), C.byref(fw), sup.h, self.num_frames, _pad3(sup.pitch), _pad3(clip_pitch), _pad3(self.dst_pitch), C.byref(self.h), err), err)

    def run(self, ns, clip, supers, blobs_bw, blobs_fw, out=None):
        """ns: output frame numbers, one job each, all in one call; clip / supers: device frames of the input clip and its super clip;
        blobs_bw / blobs_fw: per input frame device blobs of the two vector clips (mvbw at n, mvfw at n).  Frame n reads mvbw at n - delta and
        mvfw at n + delta (MVFlowBlur.c:158-178); where either lies outside the clip it copies clip frame n."""
        arr, out = self.jobs(ns, clip, supers, blobs_bw, blobs_fw, out)
        self.launch(arr)
        return out

    def launch(self, arr):
        """enqueues a job table made by jobs()"""
        _check(lib().mvx_flowblur_frames(self.h, len(arr), arr, _stream()))

    def jobs(self, ns, clip, supers, blobs_bw, blobs_fw, out=None):
        """the job table of run() and its output frames, without launching"""
        torch = _torch()
        n = len(ns)
        if out is None:
            out = _flow_out(torch, self, n, clip[0])
        arr = (FlowBlurJob * n)()
        d = self.delta
        for k, fo in enumerate(ns):
            for p in range(self.sup.nplanes):
                arr[k].clip[p] = clip[fo][p].data_ptr()
                arr[k].dst[p] = out[k][p].data_ptr()
            if fo - d >= 0 and fo + d < self.num_frames:
                for p in range(self.sup.nplanes):
                    arr[k].super[p] = supers[fo][p].data_ptr()
                arr[k].blob_bw = blobs_bw[fo - d].data_ptr()
                arr[k].blob_fw = blobs_fw[fo + d].data_ptr()
        return arr, out


class Mask(_Handle):
    """mv.Mask(clip, vectors, ml, gamma, kind, time, ysc, thscd1, thscd2) -- MVMask.c:227-346.  `width` / `height` / `subsampling` / `gray` /
    `bits` describe the clip argument (which must have the vector clip's geometry); the output is always three 8-bit planes, 4:4:4 for a
    Gray clip.  `clip_pitch` is the row pitch of the clip's device planes (only the luma plane is read, by kind 5); `dst_pitch` the row
    pitches of the output planes (multiples of 16 bytes; default: the plane widths rounded up to 256).
    deep: mvx_mask_create_deep -- a clip of 8 to 16 bits gives planes of its own depth (`out_bits`): above 8 bits run() returns planes of uint16
    samples (byte tensors with rows of 16-bit samples, as everywhere in this package: plane_to_numpy(plane, width, np.uint16)) and kind 5 takes
    the clip's 16-bit luma; all pitches are in bytes, and the defaults are rows of 16-bit samples rounded up to 256 bytes.  ysc stays 0..255.
    include/mvtools_amd.h has the semantics: kinds 0-2 replicate their bits up to the clip's peak, kinds 3-5 scale around the neutral value, and
    kind 1 shifts the SAD right by bits - 8."""
    _destroy = "mvx_mask_destroy"

    def __init__(self, vectors_ad, width, height, subsampling=(1, 1), gray=False, clip_pitch=None, dst_pitch=None, bits=8, ml=100.0, gamma=1.0,
                 kind=None, time=100.0, ysc=None, thscd1=None, thscd2=None, deep=False):
        a = MaskArgs(float(ml), float(gamma), _u(kind), float(time), _u(ysc), _u(thscd1), _u(thscd2))
        ad = AnalysisData.from_buffer_copy(bytes(vectors_ad))
        c = MaskClip(int(width), int(height), int(bits), int(subsampling[0]), int(subsampling[1]), int(bool(gray)))
        sw, sh = (0, 0) if gray else subsampling
        if dst_pitch is None:
            bps = 2 if deep and int(bits) > 8 else 1
            dst_pitch = [((max(int(width) >> s, 1) * bps + 255) // 256) * 256 for s in (0, sw, sw)]
        if clip_pitch is None:
            clip_pitch = [dst_pitch[0]]
        self.h = C.c_void_p()
        self.kind = 0 if kind is None else int(kind)
        self.pitch = list(dst_pitch)
        err = C.create_string_buffer(ERRLEN)
        create = lib().mvx_mask_create_deep if deep else lib().mvx_mask_create
        _check(create(C.byref(a), C.byref(ad), C.byref(c), _pad3(clip_pitch), _pad3(dst_pitch), C.byref(self.h), err), err)
        self.info = MaskInfo()
        lib().mvx_mask_get_info(self.h, C.byref(self.info))

    @property
    def out_bits(self):
        """bits per sample of the planes run() writes: 8, or with deep the clip's depth"""
        return lib().mvx_mask_out_bits(self.h)

    def alloc(self, n, device="cuda"):
        """n output frames of three planes with this filter's pitches (contents undefined)"""
        return arena_frames(n, [(self.info.plane_height[p], self.pitch[p]) for p in range(3)], device, zero=False)

    def run(self, blobs, clip=None, out=None):
        """blobs: per output frame the device blob of the vector clip at that frame (None: unusable); clip: per output frame the clip
        frame (a list of device planes, of which kind 5 reads the luma), or None for kinds 0-4; all frames in one call"""
        arr, out = self.jobs(blobs, clip, out)
        self.launch(arr)
        return out

    def launch(self, arr):
        """enqueues a job table (a ctypes array of MaskJob, e.g. from jobs())"""
        _check(lib().mvx_mask_frames(self.h, len(arr), arr, _stream()))

    def jobs(self, blobs, clip=None, out=None):
        """the job table of run() and its output frames, without launching"""
        _torch()
        n = len(blobs)
        if out is None:
            dev = next((b.device for b in blobs if b is not None), "cuda")
            out = self.alloc(n, dev)
        arr = (MaskJob * n)()
        for k, blob in enumerate(blobs):
            arr[k].blob = blob.data_ptr() if blob is not None else None
            arr[k].clip_luma = clip[k][0].data_ptr() if clip is not None else None
            for p in range(3):
                arr[k].dst[p] = out[k][p].data_ptr()
        return arr, out


class DepanAnalyse(_Handle):
    """mv.DepanAnalyse(clip, vectors, mask, zoom, rot, pixaspect, error, info, wrong, zerow, thscd1, thscd2, fields, tff) -- MVDepan.cpp:473-615.
    `width` / `height` describe the clip; `mask` = (bits,) or (bits, width, height) of the optional mask clip.  The vectors come from a delta-1
    Analyse; for backward vectors the caller passes the blob of frame max(0, n - 1) for frame n (MVDepan.cpp:287).  The estimator runs on the
    host in block order; run() gathers what it reads with one kernel, run_host() takes numpy blobs and mask planes and touches no device."""
    _destroy = "mvx_depan_analyse_destroy"

    def __init__(self, vectors_ad, width, height, bits=8, subsampling=(1, 1), gray=False, mask=None, zoom=None, rot=None, pixaspect=1.0, error=15.0,
                 wrong=10.0, zerow=0.05, thscd1=None, thscd2=None, fields=None, num_frames=1, vector_frames=None, mask_frames=None):
        a = DepanAnalyseArgs(_u(zoom), _u(rot), float(pixaspect), float(error), float(wrong), float(zerow), _u(thscd1), _u(thscd2), _u(fields))
        ad = AnalysisData.from_buffer_copy(bytes(vectors_ad))
        c = DepanClip(int(width), int(height), int(bits), int(subsampling[0]), int(subsampling[1]), int(bool(gray)))
        m = None
        if mask is not None:
            mask = tuple(mask) + (width, height)[len(mask) - 1:] if len(mask) < 3 else tuple(mask)
            m = C.byref(DepanClip(int(mask[1]), int(mask[2]), int(mask[0]), 0, 0, 1))
        self.has_mask = mask is not None
        self.nblk = ad.nBlkX * ad.nBlkY
        self.h = C.c_void_p()
        err = C.create_string_buffer(ERRLEN)
        nf = int(num_frames)
        _check(lib().mvx_depan_analyse_create(C.byref(a), C.byref(ad), C.byref(c), m, nf, nf if vector_frames is None else int(vector_frames),
                                              nf if mask_frames is None else int(mask_frames), C.byref(self.h), err), err)

    @staticmethod
    def _result(out):
        return [dict(dx=m.dx, dy=m.dy, zoom=m.zoom, rot=m.rot, iter=m.iter, error=m.error) for m in out]

    def _fields(self, n, top_field):
        return None if top_field is None else (C.c_int32 * n)(*[int(bool(t)) for t in top_field])

    def run(self, blobs, masks=None, top_field=None):
        """blobs: device blobs (None: unusable); masks: device luma planes of the mask clip; -> one dict per frame"""
        _torch()
        n = len(blobs)
        ptrs = (C.c_void_p * n)(*[b.data_ptr() if b is not None else None for b in blobs])
        mp = (C.c_void_p * n)(*[m.data_ptr() for m in masks]) if masks is not None else None
        out = (DepanMotion * n)()
        _check(lib().mvx_depan_analyse_frames(self.h, n, ptrs, mp, masks[0].stride(0) if masks is not None else 0, self._fields(n, top_field), out, _stream()))
        return self._result(out)

    def run_host(self, blobs, masks=None, top_field=None):
        """the same from numpy uint8 blobs and 2-D numpy uint8 mask planes of one shape; no device"""
        n = len(blobs)
        keep = [np.ascontiguousarray(b, dtype=np.uint8) if b is not None else None for b in blobs]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data if b is not None else None for b in keep])
        mk = [np.ascontiguousarray(m, dtype=np.uint8) for m in masks] if masks is not None else None
        mp = (C.c_void_p * n)(*[m.ctypes.data for m in mk]) if mk is not None else None
        out = (DepanMotion * n)()
        _check(lib().mvx_depan_analyse_host(self.h, n, ptrs, mp, mk[0].strides[0] if mk is not None else 0, self._fields(n, top_field), out))
        return self._result(out)


class DepanEstimate(_Handle):
    """mv.DepanEstimate(clip, trust, winx, winy, wleft, wtop, dxmax, dymax, zoommax, stab, pixaspect, info, show, fields, tff) -- MVDepan.cpp:1271-1503,
    without the `info` overlay.  spectra() is the reference's stage 1 (one or two window spectra per frame), correlate() its stage 2
    (prev against cur: dx, dy, zoom, trust), finish() its stage 3 (host arithmetic); run() does all three for consecutive frames and returns
    what DepanCompensate.transform() takes.  The transforms are HIP kernels; there is no FFTW and no CPU path."""
    _destroy = "mvx_depan_estimate_destroy"

    def __init__(self, width, height, bits=8, trust=4.0, winx=None, winy=None, wleft=None, wtop=None, dxmax=None, dymax=None, zoommax=1.0, stab=1.0,
                 pixaspect=1.0, fields=None, tff=None, num_frames=1 << 30, float_samples=False):
        a = DepanEstimateArgs(float(trust), float(zoommax), float(stab), float(pixaspect), _u(winx), _u(winy), _u(wleft), _u(wtop), _u(dxmax), _u(dymax),
                              _u(fields), _u(tff), int(bool(float_samples)))
        c = DepanClip(int(width), int(height), int(bits), 0, 0, 1)
        self.h = C.c_void_p()
        self.num_frames = int(num_frames)
        err = C.create_string_buffer(ERRLEN)
        _check(lib().mvx_depan_estimate_create(C.byref(a), C.byref(c), self.num_frames, C.byref(self.h), err), err)
        self.info = DepanEstimateInfo()
        lib().mvx_depan_estimate_get_info(self.h, C.byref(self.info))
        self.windows = self.info.windows

    def spectra(self, frames):
        """frames: device luma planes ([h, pitch] uint8 tensors of one pitch) -> one float32 tensor [windows, winy, winx / 2 + 1, 2] per frame"""
        n = len(frames)
        if n == 0:
            _check(lib().mvx_depan_estimate_spectra(self.h, 0, None, 0, None, None))
            return []
        torch = _torch()
        if any(f.stride(0) != frames[0].stride(0) or f.device != frames[0].device for f in frames):
            raise MvtoolsError("DepanEstimate.spectra: the planes of one call must share one pitch and one device")
        i = self.info
        big = torch.empty((n, self.windows, i.winy, i.winx // 2 + 1, 2), dtype=torch.float32, device=frames[0].device)
        out = [big[k] for k in range(n)]
        src = (C.c_void_p * n)(*[f.data_ptr() for f in frames])
        dst = (C.c_void_p * n)(*[o.data_ptr() for o in out])
        _check(lib().mvx_depan_estimate_spectra(self.h, n, src, frames[0].stride(0), dst, _stream()))
        return out

    @staticmethod
    def _ints(n, values):
        return None if values is None else (C.c_int32 * max(n, 1))(*[UNSET if v is None else int(v) for v in values])

    def correlate(self, prev, cur, top_field=None, frame_numbers=None, scans=False, show=None):
        """prev / cur: spectra of frames n - 1 and n; -> one dict(dx, dy, zoom, trust) per pair (with scans=True also the per-window scan results).
        show: the device luma planes of the cur frames ([h, pitch] uint8 tensors of one pitch); copies of them with the correlation surface painted
        into the window(s) are returned last"""
        n = len(cur)
        out = (DepanEstimateResult * max(n, 1))()
        sc = (DepanEstimateScan * max(n * self.windows, 1))()
        if n == 0:
            _check(lib().mvx_depan_estimate_correlate(self.h, 0, None, None, None, None, out, None, None))
            empty = ([],) * (1 + bool(scans) + (show is not None))
            return empty if len(empty) > 1 else []
        _torch()
        pp = (C.c_void_p * n)(*[p.data_ptr() for p in prev])
        cp = (C.c_void_p * n)(*[c.data_ptr() for c in cur])
        painted = None
        if show is None:
            _check(lib().mvx_depan_estimate_correlate(self.h, n, pp, cp, self._ints(n, top_field), self._ints(n, frame_numbers), out, sc, _stream()))
        else:
            if len(show) != n or any(f.stride(0) != show[0].stride(0) or f.device != show[0].device for f in show):
                raise MvtoolsError("DepanEstimate.correlate: show takes one plane per pair, all of one pitch and one device")
            painted = [f.clone() for f in show]
            sp = (C.c_void_p * n)(*[f.data_ptr() for f in painted])
            _check(lib().mvx_depan_estimate_correlate_show(self.h, n, pp, cp, self._ints(n, top_field), self._ints(n, frame_numbers), out, sc, sp,
                                                           painted[0].stride(0), _stream()))
        res = [dict(dx=r.dx, dy=r.dy, zoom=r.zoom, trust=r.trust) for r in out[:n]]
        ret = (res,)
        if scans:
            keys = [f[0] for f in DepanEstimateScan._fields_]
            ret += ([{k: getattr(s, k) for k in keys} for s in sc[:n * self.windows]],)
        if painted is not None:
            ret += (painted,)
        return ret if len(ret) > 1 else res

    def host_tail(self, scans, top_field=None, frame_numbers=None):
        """the host tail alone from windows scan results (dicts) per pair; no device"""
        n = len(scans) // self.windows
        sc = (DepanEstimateScan * max(len(scans), 1))(*[DepanEstimateScan(**s) for s in scans])
        out = (DepanEstimateResult * max(n, 1))()
        _check(lib().mvx_depan_estimate_host_tail(self.h, n, sc, self._ints(n, top_field), self._ints(n, frame_numbers), out))
        return [dict(dx=r.dx, dy=r.dy, zoom=r.zoom, trust=r.trust) for r in out[:n]]

    def finish(self, results):
        """stage 3 over the stage-2 results of frames 0 .. len - 1 of a clip of num_frames -> (dx, dy, zoom, rot) per frame; the neighbours of
        the first and the last frame are clamped as in the reference"""
        n = len(results)
        out = []
        for k in range(n):
            tri = (DepanEstimateResult * 3)(*[DepanEstimateResult(**{f: float(results[q][f]) for f in ("dx", "dy", "zoom", "trust")})
                                             for q in (max(0, k - 1), k, min(k + 1, n - 1))])
            m = DepanMotion()
            _check(lib().mvx_depan_estimate_finish(self.h, k, tri, C.byref(m)))
            out.append((m.dx, m.dy, m.zoom, m.rot))
        return out

    def run(self, frames, top_field=None):
        """all three stages for frames 0 .. len - 1 of a clip: each frame is transformed once; frame 0 gives zeros by the reference's rule"""
        n = len(frames)
        if n == 0:
            return []
        sp = self.spectra(frames)
        res = self.correlate([sp[max(0, k - 1)] for k in range(n)], sp, top_field, list(range(n)))
        return self.finish(res)


class _DepanWarp(_Handle):
    """What DepanCompensate and DepanStabilise share: the clip's format, the default pitches (rows rounded up to 256 bytes), the handle and its
    info struct, the output arena and the launch of a job array.  _name: the stem of the library's functions; _info: the info struct's class.
    sample_float=True with bits=32 selects the *_create_float entry: planes of float32 (4-byte samples in the default pitches), the border
    0.0f luma / 0.5f chroma, nothing clamped; transforms, plans and jobs are the same host arithmetic."""
    _name = _info = None

    def _create(self, sample_float, args, width, height, bits, subsampling, gray, src_pitch, dst_pitch, num_frames, data_frames, *extra):
        """extra: the arguments of the creation function between data_frames and the pitches"""
        c = DepanClip(int(width), int(height), int(bits), int(subsampling[0]), int(subsampling[1]), int(bool(gray)))
        sw = 0 if gray else subsampling[0]
        self.is_float = bool(sample_float)
        bps = 4 if self.is_float else 2 if bits > 8 else 1
        if dst_pitch is None:
            dst_pitch = [((max(int(width) >> s, 1) * bps + 255) // 256) * 256 for s in (0, sw, sw)]
        if src_pitch is None:
            src_pitch = dst_pitch
        self.h = C.c_void_p()
        self.pitch = list(dst_pitch)
        self.dtype = np.float32 if self.is_float else np.uint16 if bits > 8 else np.uint8
        err = C.create_string_buffer(ERRLEN)
        _check(getattr(lib(), self._name + ("_create_float" if self.is_float else "_create"))(C.byref(args), C.byref(c), int(num_frames), int(num_frames if data_frames is None else data_frames), *extra,
                                                      _pad3(src_pitch), _pad3(dst_pitch), C.byref(self.h), err), err)
        self.info = self._info()
        getattr(lib(), self._name + "_get_info")(self.h, C.byref(self.info))
        self.nplanes = self.info.num_planes

    def alloc(self, n, device="cuda"):
        return arena_frames(n, [(self.info.plane_height[p], self.pitch[p]) for p in range(self.nplanes)], device, zero=False)

    def launch(self, arr):
        _check(getattr(lib(), self._name + "_frames")(self.h, len(arr), arr, _stream()))


class DepanCompensate(_DepanWarp):
    """mv.DepanCompensate(clip, data, offset, subpixel, pixaspect, matchfields, mirror, blur, info, fields, tff) -- MVDepan.cpp:2750-2881.
    map(n) says which clip frame to warp and which data frames' motions to sum, transform(motions, ...) sums them (host arithmetic), and a
    job is (src planes, summed transform).  `src_pitch` / `dst_pitch`: row pitches in bytes of the device planes.  sample_float=True with bits=32
    selects mvx_depan_compensate_create_float: float32 planes in and out; the transforms come from motion found on an 8..16 bit copy."""
    _destroy, _name, _info = "mvx_depan_compensate_destroy", "mvx_depan_compensate", DepanCompensateInfo

    def __init__(self, width, height, bits=8, subsampling=(1, 1), gray=False, src_pitch=None, dst_pitch=None, offset=0.0, subpixel=None, pixaspect=1.0,
                 matchfields=None, mirror=None, blur=None, fields=None, tff=None, num_frames=1 << 30, data_frames=None, sample_float=False):
        a = DepanCompensateArgs(float(offset), _u(subpixel), float(pixaspect), _u(matchfields), _u(mirror), _u(blur), _u(fields), _u(tff))
        self._create(sample_float, a, width, height, bits, subsampling, gray, src_pitch, dst_pitch, num_frames, data_frames)

    def map(self, n):
        """(nsrc, start, end) of output frame n: warp clip frame nsrc by the motions of data frames start + 1 .. end; None: return clip frame n"""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        if not lib().mvx_depan_compensate_map(self.h, int(n), C.byref(a), C.byref(b), C.byref(c)):
            return None
        return a.value, b.value, c.value

    def transform(self, motions, top_field=None, ndest=0):
        """motions: (dx, dy, zoom, rot) of data frames start + 1 .. end -> (trsum as six floats, (dx, dy, zoom, rot) of the info string)"""
        flat = [float(v) for m in motions for v in m]
        arr = (C.c_float * max(len(flat), 1))(*flat)
        tr, mo = (C.c_float * 6)(), (C.c_float * 4)()
        err = C.create_string_buffer(ERRLEN)
        _check(lib().mvx_depan_motion_to_transform(self.h, len(motions), arr, int(ndest), UNSET if top_field is None else int(bool(top_field)), tr, mo, err), err)
        return np.array(tr, dtype=np.float32), np.array(mo, dtype=np.float32)

    def run(self, frames, transforms, out=None):
        """frames: per job the device planes of clip frame nsrc; transforms: per job trsum; all jobs in one call"""
        arr, out = self.jobs(frames, transforms, out)
        self.launch(arr)
        return out

    def jobs(self, frames, transforms, out=None):
        _torch()
        n = len(frames)
        if out is None:
            out = self.alloc(n, frames[0][0].device if n else "cuda")
        arr = (DepanCompensateJob * n)()
        for k in range(n):
            for p in range(self.nplanes):
                arr[k].src[p] = frames[k][p].data_ptr()
                arr[k].dst[p] = out[k][p].data_ptr()
            t = np.asarray(transforms[k], dtype=np.float32)
            for i in range(6):
                arr[k].tr[i] = t[i]
        return arr, out


class DepanStabilise(_DepanWarp):
    """mv.DepanStabilise(clip, data, cutoff, damping, initzoom, addzoom, prev, next, mirror, blur, dxmax, dymax, zoommax, rotmax, subpixel, pixaspect,
    fitlast, tzoom, info, method, fields) -- MVDepan.cpp:3909-4208.  window(n) names the data frames whose motion plan(n, motions) reads (host
    arithmetic) and the clip frames its sources lie among; a job is a plan with the planes of the current, prev and next source frames; all jobs
    of a call are one fused launch.  `src_pitch` / `dst_pitch`: row pitches in bytes of the device planes.  Float arguments: None -> the default.
    sample_float=True with bits=32 selects mvx_depan_stabilise_create_float: float32 planes in and out; the motions come from an 8..16 bit copy."""
    _destroy, _name, _info = "mvx_depan_stabilise_destroy", "mvx_depan_stabilise", DepanStabiliseInfo

    def __init__(self, width, height, bits=8, subsampling=(1, 1), gray=False, src_pitch=None, dst_pitch=None, fps=(25, 1), num_frames=1 << 30, cutoff=None,
                 damping=None, initzoom=None, addzoom=None, prev=None, next=None, mirror=None, blur=None, dxmax=None, dymax=None, zoommax=None, rotmax=None,
                 subpixel=None, pixaspect=None, fitlast=None, tzoom=None, method=None, fields=None, data_frames=None, sample_float=False):
        d = lambda v: float(UNSET) if v is None else float(v)
        a = DepanStabiliseArgs(d(cutoff), d(damping), d(initzoom), d(dxmax), d(dymax), d(zoommax), d(rotmax), d(pixaspect), d(tzoom), _u(addzoom), _u(prev),
                               _u(next), _u(mirror), _u(blur), _u(subpixel), _u(fitlast), _u(method), _u(fields))
        self.num_frames = int(num_frames)
        self._create(sample_float, a, width, height, bits, subsampling, gray, src_pitch, dst_pitch, num_frames, data_frames, int(fps[0]), int(fps[1]))

    def windows(self):
        """the cosine windows wint, winrz, winfz: radius + 1 float32 each"""
        n = self.info.radius + 1
        w = [(C.c_float * n)() for _ in range(3)]
        lib().mvx_depan_stabilise_get_windows(self.h, *w)
        return [np.array(v, dtype=np.float32) for v in w]

    def window(self, n):
        """(data_first, data_last, clip_first, clip_last) of output frame n"""
        v = [C.c_int() for _ in range(4)]
        _check(lib().mvx_depan_stabilise_window(self.h, int(n), *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    @staticmethod
    def _motion(m):
        return (m["dx"], m["dy"], m["zoom"], m["rot"]) if isinstance(m, dict) else tuple(m)

    def plan(self, n, motions):
        """motions: (dx, dy, zoom, rot) or the dicts of DepanAnalyse.run / DepanEstimate.run, per data frame data_first .. data_last of window(n)"""
        flat = [float(v) for m in motions for v in self._motion(m)]
        w = self.window(n)
        if len(flat) != 4 * (w[1] - w[0] + 1):
            raise MvtoolsError("DepanStabilise.plan: frame %d needs the motions of data frames %d .. %d" % (n, w[0], w[1]))
        arr = (C.c_float * len(flat))(*flat)
        plan = DepanStabilisePlan()
        err = C.create_string_buffer(ERRLEN)
        _check(lib().mvx_depan_stabilise_plan(self.h, int(n), arr, C.byref(plan), err), err)
        return plan

    def jobs(self, plans, cur, prev=None, next=None, out=None):
        """plans: per job a DepanStabilisePlan; cur / prev / next: per job the device planes of clip frame n, plan.prev.frame, plan.next.frame
        (prev / next entries may be None where the plan does not use them)"""
        _torch()
        n = len(plans)
        if out is None:
            out = self.alloc(n, cur[0][0].device if n else "cuda")
        arr = (DepanStabiliseJob * n)()
        for k in range(n):
            arr[k].plan = plans[k]
            for p in range(self.nplanes):
                arr[k].cur[p] = cur[k][p].data_ptr()
                arr[k].dst[p] = out[k][p].data_ptr()
                if plans[k].prev.used:
                    arr[k].prev[p] = prev[k][p].data_ptr()
                if plans[k].next.used:
                    arr[k].next[p] = next[k][p].data_ptr()
        return arr, out

    def run(self, frames, motions, out=None):
        """a whole clip: frames[n] the device planes of clip frame n, motions[n] the motion of data frame n; every output frame in one call"""
        n = len(frames)
        plans = []
        for k in range(n):
            w = self.window(k)
            plans.append(self.plan(k, motions[w[0]:w[1] + 1]))
        arr, out = self.jobs(plans, frames, [frames[p.prev.frame] if p.prev.used else None for p in plans],
                             [frames[p.next.frame] if p.next.used else None for p in plans], out)
        self.launch(arr)
        return out


class Recalculate(_Handle):
    """mv.Recalculate(super, vectors, thsad, smooth, blksize, ...) -- MVRecalculate.c:263-545."""
    _destroy = "mvx_recalculate_destroy"

    def __init__(self, sup, vectors_ad, **kw):
        self.sup = sup
        a = RecalculateArgs(*([UNSET] * len(RECALC_ARGS)))
        for k, v in kw.items():
            k2 = {"lambda": "lambda_"}.get(k, k)
            if k2 not in RECALC_ARGS:
                raise TypeError("Recalculate: unknown argument " + k)
            if v is not None:
                setattr(a, k2, int(v))
        old = AnalysisData.from_buffer_copy(bytes(vectors_ad))
        self.h = C.c_void_p()
        err = C.create_string_buffer(ERRLEN)
        _check(lib().mvx_recalculate_create(C.byref(a), sup.h, C.byref(old), _pad3(sup.pitch), C.byref(self.h), err), err)
        self.ad = AnalysisData()
        lib().mvx_recalculate_get_data(self.h, C.byref(self.ad))
        self.blob_size = lib().mvx_recalculate_blob_size(self.h)

    def run(self, jobs, blobs=None):
        """jobs: list of (src_super, ref_super_or_None, old_blob) -> list of device blobs."""
        torch = _torch()
        n = len(jobs)
        if blobs is None:
            stride = (self.blob_size + 255) // 256 * 256
            buf = torch.zeros((n, stride), dtype=torch.uint8, device=jobs[0][0][0].device)
            blobs = [buf[i, :self.blob_size] for i in range(n)]
        arr = (RecalculateJob * n)()
        for i, (s, r, ob) in enumerate(jobs):
            for p in range(self.sup.nplanes):
                arr[i].src[p] = s[p].data_ptr()
                arr[i].ref[p] = r[p].data_ptr() if r is not None else None
            arr[i].old_blob = ob.data_ptr()
            arr[i].blob = blobs[i].data_ptr()
        _check(lib().mvx_recalculate_frames(self.h, n, arr, _stream()))
        return blobs


class RecalculateN(_Handle):
    """A multi blob refined field by field (include/mvtools_amd.h, mv.RecalculateN): field r of the result is the MVTools_vectors of
    Recalculate on field r of the old blob, byte for byte, at byte r * field_stride.  vectors_ad: of field 0 of the old blob (AnalyseN.ad(0));
    keyword names are Recalculate's."""
    _destroy = "mvx_recalculate_n_destroy"

    def __init__(self, sup, vectors_ad, radius, **kw):
        self.sup = sup
        a = RecalculateArgs(*([UNSET] * len(RECALC_ARGS)))
        for k, v in kw.items():
            k2 = {"lambda": "lambda_"}.get(k, k)
            if k2 not in RECALC_ARGS:
                raise TypeError("RecalculateN: unknown argument " + k)
            if v is not None:
                setattr(a, k2, int(v))
        old = AnalysisData.from_buffer_copy(bytes(vectors_ad))
        self.h = C.c_void_p()
        err = C.create_string_buffer(ERRLEN)
        _check(lib().mvx_recalculate_n_create(C.byref(a), int(radius), sup.h, C.byref(old), _pad3(sup.pitch), C.byref(self.h), err), err)
        self.radius = int(radius)
        self.field_size = lib().mvx_recalculate_n_field_size(self.h)
        self.field_stride = lib().mvx_recalculate_n_field_stride(self.h)
        self.blob_size = lib().mvx_recalculate_n_blob_size(self.h)

    def get_data(self, r):
        """the MVTools_MVAnalysisData of field r of the result"""
        out = AnalysisData()
        _check(lib().mvx_recalculate_n_get_data(self.h, int(r), C.byref(out)))
        return out

    def alloc_blobs(self, n, device="cuda"):
        torch = _torch()
        buf = torch.zeros((n, self.blob_size), dtype=torch.uint8, device=device)
        return [buf[i] for i in range(n)]

    def fields(self, multi_blob):
        """the 2 * radius fields of a multi blob as tensor views: each is a blob any consumer takes"""
        return [multi_blob[r * self.field_stride:r * self.field_stride + self.field_size] for r in range(2 * self.radius)]

    def run(self, jobs, blobs=None, old_field_stride=None):
        """jobs: list of (src_super_frame, [ref_super_frame or None] * 2r in the order of multi_refs, old_multi_blob) -> list of multi blobs
        on the device.  old_field_stride defaults to the old blob's bytes / 2r (a blob of AnalyseN.alloc_blobs)."""
        n, nr = len(jobs), 2 * self.radius
        if blobs is None:
            blobs = self.alloc_blobs(n, device=jobs[0][0][0].device)
        arr = (RecalculateNJob * n)()
        table = _ref_table([refs for _, refs, _ in jobs], nr, self.sup.nplanes, "RecalculateN")
        for i, (s, refs, ob) in enumerate(jobs):
            for p in range(self.sup.nplanes):
                assert s[p].stride(0) == self.sup.pitch[p]
                arr[i].src[p] = s[p].data_ptr()
            arr[i].refs = C.cast(C.byref(table, i * nr * C.sizeof(C.c_void_p * 3)), C.POINTER(C.c_void_p * 3))
            if ob is None:
                raise ValueError("RecalculateN: a job needs its old multi blob")
            arr[i].old_blob = ob.data_ptr()
            arr[i].old_field_stride = int(old_field_stride) if old_field_stride is not None else ob.numel() // nr
            if blobs[i].numel() < self.blob_size:
                raise ValueError("RecalculateN: a multi blob holds %d bytes" % self.blob_size)
            arr[i].blob = blobs[i].data_ptr()
        _check(lib().mvx_recalculate_n_frames(self.h, n, arr, _stream()))
        return blobs


class ScaleVect(_Handle):
    """The blobs of a vector clip rewritten for a clip `scale` (1, 2 or 4) times its size (include/mvtools_amd.h, mv.ScaleVect): search on a small
    or 8-bit clip, use the vectors on super_clip's.  vectors_data: the small clip's MVTools_MVAnalysisData; .ad: the scaled clip's, which is
    what the consumers (Recalculate, Degrain, Compensate, ...) on super_clip are created with.  The SADs are estimates until a Recalculate."""
    _destroy = "mvx_scale_vect_destroy"

    def __init__(self, vectors_data, super_clip, scale=2):
        self.sup = super_clip
        self.scale = int(scale)
        ad = AnalysisData.from_buffer_copy(bytes(vectors_data))
        self.h = C.c_void_p()
        err = C.create_string_buffer(ERRLEN)
        _check(lib().mvx_scale_vect_create(C.byref(ad), self.scale, super_clip.h, C.byref(self.h), err), err)
        self.ad = AnalysisData()
        lib().mvx_scale_vect_get_data(self.h, C.byref(self.ad))
        self.blob_size = lib().mvx_vectors_size(C.byref(self.ad))

    def run(self, blobs, out=None, fields=1, field_stride=None):
        """blobs: device blobs of the small clip, a list of tensors or the rows of one tensor; all of them in one launch -> the scaled blobs
        (out: the tensors to write, which may be the inputs themselves; default: new ones, laid out like Analyse.alloc_blobs).  fields = 2 *
        radius scales whole multi blobs: field_stride defaults to a blob's bytes / fields, and the bytes between the fields are not touched."""
        torch = _torch()
        blobs = list(blobs)
        n, fields = len(blobs), int(fields)
        if fields < 1:
            raise ValueError("ScaleVect: fields must be at least 1")
        stride = 0 if fields == 1 else int(field_stride) if field_stride is not None else blobs[0].numel() // fields
        need = self.blob_size if fields == 1 else (fields - 1) * stride + self.blob_size
        if out is None:
            row = (self.blob_size + 255) // 256 * 256 if fields == 1 else fields * stride
            buf = torch.zeros((n, row), dtype=torch.uint8, device=blobs[0].device)
            out = [buf[i, :need] for i in range(n)]
        out = list(out)
        if len(out) != n:
            raise ValueError("ScaleVect: %d blobs, %d outputs" % (n, len(out)))
        arr = (ScaleVectJob * max(n, 1))()
        for i, (b, o) in enumerate(zip(blobs, out)):
            if b.numel() < need or o.numel() < need or not b.is_contiguous() or not o.is_contiguous():
                raise ValueError("ScaleVect: a blob is a contiguous tensor of at least %d bytes" % need)
            arr[i].in_, arr[i].out, arr[i].fields, arr[i].field_stride = b.data_ptr(), o.data_ptr(), fields, stride
        _check(lib().mvx_scale_vect_frames(self.h, n, arr, _stream()))
        return out


def scdetect(analysis_data, blobs, thscd1=None, thscd2=None):
    """mv.SCDetection's decision per frame (MVSCDetection.c:43-73): list of 0/1 = value of _SceneChangePrev/_SceneChangeNext."""
    n = len(blobs)
    ad = AnalysisData.from_buffer_copy(bytes(analysis_data))
    ptrs = (C.c_void_p * n)(*[b.data_ptr() for b in blobs])
    out = (C.c_int32 * n)()
    err = C.create_string_buffer(ERRLEN)
    _check(lib().mvx_scdetect(C.byref(ad), _u(thscd1), _u(thscd2), n, ptrs, out, _stream(), err), err)
    return list(out)
