"""ScaleVect restated in numpy (test infrastructure): the contract of include/mvtools_amd.h, "mv.ScaleVect", and DESIGN.md 4.3.3.

    scaled_data(ad, scale, si)                    the MVTools_MVAnalysisData of the scaled clip, or ValueError with the library's message
    scale_blob(blob, ad, out_ad, scale)           one blob rewritten (a copy)
    scale_multi(blob, ad, out_ad, scale, fields, stride)   every field of a multi blob; the bytes between the fields stay

`si` is anything with the fields of mvx_super_info that the contract names (the product's Super.info)."""
import numpy as np

import vector_fields as vf

OK_BLOCKS = ((4, 4), (8, 4), (8, 8), (16, 2), (16, 8), (16, 16), (32, 16), (32, 32), (64, 32), (64, 64), (128, 64), (128, 128))
MOTION_USE_CHROMA_MOTION = 8

E_SCALE = "ScaleVect: scale must be 1, 2 or 4."
E_SIZE = "ScaleVect: the target super clip must be scale times the size of the vectors' clip."
E_CHROMA = "ScaleVect: the target super clip's chroma subsampling or colour data is not that of the vectors."
E_BLOCK = "ScaleVect: the scaled block size must be 4x4, 8x4, 8x8, 16x2, 16x8, 16x16, 32x16, 32x32, 64x32, 64x64, 128x64, or 128x128."
E_PEL = "ScaleVect: scale times the target's pel must be a multiple of the vectors' pel."


def vectors_size(ad):
    """Fakery.c:110-121 through vector_fields.level_span's grids: bytes of a blob"""
    nwb = (ad.nBlkSizeX - ad.nOverlapX) * ad.nBlkX + ad.nOverlapX
    nhb = (ad.nBlkSizeY - ad.nOverlapY) * ad.nBlkY + ad.nOverlapY
    size = 8
    for i in range(ad.nLvCount):
        size += 4 + 16 * (((nwb >> i) - ad.nOverlapX) // (ad.nBlkSizeX - ad.nOverlapX)) * (((nhb >> i) - ad.nOverlapY) // (ad.nBlkSizeY - ad.nOverlapY))
    return size


def scaled_data(ad, scale, si):
    s = scale
    if s not in (1, 2, 4):
        raise ValueError(E_SCALE)
    if si.width != s * ad.nWidth or si.height != s * ad.nHeight or si.super_width - 2 * si.hpad != s * ad.nWidth:
        raise ValueError(E_SIZE)
    if ad.xRatioUV != si.xRatioUV or ad.yRatioUV != si.yRatioUV or (ad.nMotionFlags & MOTION_USE_CHROMA_MOTION and (si.modeYUV & 6) != 6):
        raise ValueError(E_CHROMA)
    if (s * ad.nBlkSizeX, s * ad.nBlkSizeY) not in OK_BLOCKS:
        raise ValueError(E_BLOCK)
    if ad.nPel <= 0 or (s * si.pel) % ad.nPel:
        raise ValueError(E_PEL)
    out = type(ad).from_buffer_copy(bytes(ad))
    for k in ("nBlkSizeX", "nBlkSizeY", "nOverlapX", "nOverlapY", "nWidth", "nHeight"):
        setattr(out, k, s * getattr(ad, k))
    out.nPel, out.bitsPerSample, out.nHPadding, out.nVPadding = si.pel, si.bits, si.hpad, si.vpad
    return out


def scale_blob(blob, ad, out_ad, scale):
    src = np.asarray(blob, dtype=np.uint8)
    out = np.array(src, dtype=np.uint8, copy=True)
    if int(src[4:8].view(np.int32)[0]) == 0:      # an invalid blob: copied
        return out
    m = scale * out_ad.nPel // ad.nPel
    shift = out_ad.bitsPerSample - ad.bitsPerSample
    xmin, xmax, ymin, ymax = vf.legal_rect(out_ad)
    for level in range(ad.nLvCount):
        assert vf.level_span(src, ad, level) == vf.level_span(src, out_ad, level), "the level grids differ"
        ixy, isad = vf.records(src, ad, level)
        oxy, osad = vf.records(out, out_ad, level)
        x, y = ixy[:, :, 0].astype(np.int64) * m, ixy[:, :, 1].astype(np.int64) * m
        if level == 0:
            x = np.minimum(np.maximum(x, xmin[None, :]), xmax[None, :])
            y = np.minimum(np.maximum(y, ymin[:, None]), ymax[:, None])
        oxy[:, :, 0], oxy[:, :, 1] = x.astype(np.int32), y.astype(np.int32)   # (a coarser level keeps the low 32 bits)
        with np.errstate(over="ignore"):
            sad = isad.astype(np.int64) * np.int64(scale * scale)           # 64-bit two's complement: wraps
            osad[:, :] = sad << np.int64(shift) if shift >= 0 else sad >> np.int64(-shift)
    return out


def scale_multi(blob, ad, out_ad, scale, fields, stride):
    out = np.array(blob, dtype=np.uint8, copy=True)
    size = vectors_size(ad)
    for r in range(fields):
        out[r * stride:r * stride + size] = scale_blob(out[r * stride:r * stride + size], ad, out_ad, scale)
    return out
