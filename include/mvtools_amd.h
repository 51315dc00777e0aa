/*
 * mvtools_amd.h -- C ABI of libmvtools_amd.so, the MI355X (gfx950) implementation of the mvtools hot path
 *   mv.Super -> mv.Analyse -> mv.Degrain1..6 / mv.Compensate.
 *
 * This is the drop-in boundary: a VapourSynth filter shell (or any other host) binds exactly these entry
 * points.  Plain pointers and sizes only.  Each entry point names the reference interface it replaces
 * (paths relative to dubhater/vapoursynth-mvtools src/).
 *
 * Conventions
 *   - every image pointer is a DEVICE pointer (HBM) unless the function name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is enqueued
 *     asynchronously on it, the caller synchronises;
 *   - optional filter arguments take MVX_UNSET to mean "not passed" (the reference's defaults apply);
 *   - functions return 0 on success, a negative code on failure; mvx_*_create additionally write the
 *     reference's user-visible error string (e.g. "Super: pel must be 1, 2, or 4.") into `err`.
 *   - there is NO CPU fallback: if no gfx950 device / kernel image is available the call fails.
 *
 * Plane layouts (checked: *_create refuses a pitch, *_frames an address, with MVX_E_ARG and before anything is uploaded or launched)
 *   - Clip-side planes -- src / clip / dst of mvx_degrain, mvx_degrain_n in all its three entries, mvx_compensate and mvx_compensate_n with
 *     their float entries,
 *     mvx_blockfps, mvx_flowinter / mvx_flowfps, mvx_flowcomp and mvx_flowblur, all of these with their float entries: any pitch that holds a row of its plane and is a multiple of
 *     the sample size (1, 2, or 4 bytes for a float clip; out16 writes 2-byte samples), and any plane address that is a multiple of the
 *     sample size.  A tight pitch, an odd pitch for 8-bit samples, a plane inside a wider frame, U and V of different pitch, src and dst of
 *     different pitch are all legal.  A shorter pitch, a pitch or address that is no multiple of the sample size, and a missing plane where
 *     the filter needs one are refused: "<src|clip|dst> pitch of plane P must hold a row of N bytes and be a multiple of the sample size."
 *     (the flow filters put their name in front), "<entry>: <what> plane P must be aligned to N bytes" / "... is required".
 *   - Super planes, for every consumer and for mvx_analyse / mvx_recalculate: what mvx_super_frames writes -- pitches that hold a row of the
 *     super plane and are multiples of 16 bytes, U and V alike, plane addresses that are multiples of 16 bytes ("super pitch of plane P must
 *     hold a row of N bytes and be a multiple of 16 bytes.", with "Analyse: " / "Recalculate: " in front there).
 *   - Only samples are written: the bytes between a plane's width and its pitch, and every byte of a super frame outside the defined
 *     rectangles, are neither written nor read (tests/test_gpu_layouts.py: planes carved out of arenas of two fills).
 *   mvx_super_frames (src: as clip-side planes; dst: super planes) and mvx_finest_frames (both sides as clip-side planes) check the same at their
 *   entries; mv.Mask and the Depan filters state their own rules at theirs.
 */
#ifndef MVTOOLS_AMD_H
#define MVTOOLS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVX_UNSET (-2147483647 - 1)
#define MVX_ERRLEN 256

#define MVX_OK 0
#define MVX_E_ARG (-1)     /* invalid filter argument (message in err) */
#define MVX_E_DEVICE (-2)  /* HIP error (message from mvx_last_error) */
#define MVX_E_NOMEM (-3)

const char *mvx_last_error(void);   /* thread-local text of the last failure */
int mvx_device_count(void);         /* number of visible gfx950 devices, <0 on error */
const char *mvx_version(void);

/* ---- wire formats (byte-identical to the reference) -------------------------------------------- */

/* VECTOR, MVAnalysisData.h:40-44 */
typedef struct mvx_vector { int32_t x, y; int64_t sad; } mvx_vector;

/* MVAnalysisData, MVAnalysisData.h:83-134 == the MVTools_MVAnalysisData frame property (84 bytes) */
typedef struct mvx_analysis_data {
    int32_t nMagicKey, nVersion, nBlkSizeX, nBlkSizeY, nPel, nLvCount, nDeltaFrame, isBackward, nCPUFlags,
        nMotionFlags, nWidth, nHeight, nOverlapX, nOverlapY, nBlkX, nBlkY, bitsPerSample, yRatioUV, xRatioUV,
        nHPadding, nVPadding;
} mvx_analysis_data;

/* ---- mv.Super ------------------------------------------------------------------------------------
 * replaces mvsuperCreate / mvsuperGetFrame, MVSuper.c:140-275 / :43-126 (argument string :279-291)   */

typedef struct mvx_super_args {
    /* the input clip's format (VSVideoInfo) */
    int32_t width, height, bits, subsampling_w, subsampling_h, gray;
    /* filter arguments, MVX_UNSET = default: hpad=16 vpad=16 pel=2 levels=0 chroma=1 sharp=2 rfilter=2 */
    int32_t hpad, vpad, pel, levels, chroma, sharp, rfilter;
} mvx_super_args;

typedef struct mvx_super_info {
    int32_t width, height, bits, xRatioUV, yRatioUV, gray;
    int32_t hpad, vpad, pel, levels, chroma, sharp, rfilter;
    int32_t modeYUV;                    /* Super_modeyuv */
    int32_t super_width, super_height;  /* luma dimensions of the super clip's frames */
    int32_t num_planes;
    int32_t plane_width[3], plane_height[3]; /* samples */
} mvx_super_info;

typedef struct mvx_super mvx_super;

int mvx_super_create(const mvx_super_args *args, mvx_super **out, char *err /* MVX_ERRLEN or NULL */);
void mvx_super_destroy(mvx_super *s);
void mvx_super_get_info(const mvx_super *s, mvx_super_info *info);

/* A super clip of a 32-bit float clip (pinterf's MVTools2 takes float clips in MSuper and MDegrain as long as the vectors come from an integer
 * search; no counterpart in the reference).  It has ONE level: args->bits must be 32 ("Super: a float clip has 32 bits per sample.") and
 * args->levels MVX_UNSET or 1 ("Super: a float super clip has one level (levels=1)."); these two checks come first, every other message is
 * mvx_super_create's in its order.  rfilter is range-checked and then unused.  mvx_super_info.bits is 32, the geometry is what mvx_super_create
 * gives for the same arguments with levels=1, samples are 4 bytes.  mvx_super_frames serves the object (src pitch a multiple of 4 bytes, planes
 * aligned alike) and fills level 0 -- padding, the pel-2 planes, the twelve averaged planes of pel 4 -- with the integer rules operation for
 * operation on float32: no rounding term, every shift a multiplication by the exact power of two, no clamp (samples may overshoot, chroma is
 * centred on 0), nothing fused:
 *   sharp 0   (a + b) * 0.5f; diagonal (((a + b) + c) + d) * 0.25f with the integer code's edge cases
 *   sharp 1   ((s(X) + s(X+1)) * 9.0f - (s(X-1) + s(X+2))) * 0.0625f
 *   sharp 2   m2 = (m2 + m3) * 4; m2 -= (m1 + m4); m2 *= 5; m0 = (m0 + m5) + m2; m0 * 0.03125f
 *   the diagonal plane of sharp 1 and 2 is the horizontal rule on the UNROUNDED vertical plane; pel 4: (a + b) * 0.5f
 * (csrc/mvx_super_float_rule.h).  Samples are assumed finite.  Only the float entries -- mvx_degrain_n_create_float, mvx_compensate_create_float,
 * mvx_compensate_n_create_float, mvx_blockfps_create_float, mvx_flowinter_create_float, mvx_flowfps_create_float, mvx_flowcomp_create_float and
 * mvx_flowblur_create_float -- consume such an object: mvx_super_shadow_copies
 * returns 0, the shadow, pelclip and Finest entries return MVX_E_ARG, and every other *_create that takes an mvx_super refuses it before any
 * other check with "<Name>: float super clips are not supported.".  Touches no device. */
int mvx_super_create_float(const mvx_super_args *args, mvx_super **out, char *err);
int mvx_super_is_float(const mvx_super *s);

/* Builds `nframes` super frames.  src[f*3+p] / dst[f*3+p] are device pointers to plane p of frame f
 * (p >= num_planes ignored); pitches in bytes, shared by all frames.  Only the defined rectangles (every
 * level's padded plane, every sub-pel plane) are written; bytes outside them are never touched, and no
 * entry of this library reads them, so dst planes need no initialisation (a caller that compares or
 * stores whole super frames zero-fills them once when it allocates them).
 * Layouts: dst pitch a multiple of 16 bytes that holds a row of the super plane ("mvx_super_frames: dst
 * pitch must be a multiple of 16 bytes"); src any pitch that holds a row, src and dst planes at any
 * address, all multiples of the sample size ("... src pitch must hold a row and be a multiple of the
 * sample size", "... planes must be aligned to the sample size"; a float clip: src 4, dst 16).  The
 * consumers and the search want dst planes on 16-byte boundaries (head of this file).  Results never
 * depend on the layout, speed does: at pel 2 the rows-in-registers kernels serve a call whose src pitches
 * are multiples of 4 with src planes on 4-byte and dst planes on 16-byte boundaries, the slower tile
 * kernels any other call. */
int mvx_super_frames(mvx_super *s, int nframes, const void *const *src, const ptrdiff_t src_pitch[3],
                     void *const *dst, const ptrdiff_t dst_pitch[3], void *stream);

/* Optional device-side layout extension for search throughput ("shadow planes").  gfx950 serves vector loads at addresses that
 * are not multiples of four several times slower than aligned ones, and a motion search reads reference blocks at arbitrary
 * sample positions.  For clips of more than 8 bits (mvx_super_shadow_copies() == 1) a caller may therefore keep, behind the planes
 * of a super frame, two derived planes that mvx_super_shadow_frames fills from planes mvx_super_frames has written (same stream):
 *   - at luma plane + copy_stride[0]: the whole luma buffer shifted left by one sample (odd sample positions become aligned);
 *   - at U plane + copy_stride[1]: the whole U and V buffers interleaved sample by sample (2 x the chroma size; every chroma
 *     position is aligned, and a block row's U and V samples share one cache line).
 * mvx_super_shadow_bytes gives the bytes to reserve behind each plane.  The shadow planes never leave the device and are not part
 * of the super clip's frame format; a search uses them after mvx_analyse_set_ref_shadow.
 * (no reference counterpart: memory layout only, results are unchanged) */
int mvx_super_shadow_copies(const mvx_super *s);   /* 1: shadow planes pay off for this format (9..16 bits), 0: not (8 bits) */
void mvx_super_shadow_bytes(const mvx_super *s, const ptrdiff_t pitch[3], size_t extra[3]);
int mvx_super_shadow_frames(const mvx_super *s, int nframes, void *const *planes /* [f*3+p] */, const ptrdiff_t pitch[3],
                            const ptrdiff_t copy_stride[3] /* [2] unused */, void *stream);
/* mvx_super_frames followed by mvx_super_shadow_frames, as one call: same results in the planes and in the shadow planes, but for
 * pel 2 the level-0 kernels write their share of the shadow data while they have the samples in registers (about a third of a
 * Super pass's HBM traffic saved).  shadow_stride as copy_stride above. */
int mvx_super_frames_shadow(mvx_super *s, int nframes, const void *const *src, const ptrdiff_t src_pitch[3],
                            void *const *dst, const ptrdiff_t dst_pitch[3], const ptrdiff_t shadow_stride[3], void *stream);

/* mv.Super(pelclip=...): the sub-pel planes of level 0 are taken from the user's upsized clip instead of being interpolated.
 * replaces MVSuper.c:229-256 (mvx_super_pelclip_mode: 0 = ignored because pel is 1, 1 = pelclip is pel x the clip size,
 * 2 = pel x the padded size; other sizes -> MVX_E_ARG with the reference's message) and MVSuper.c:91-102 +
 * mvpRefineExt MVFrame.cpp:1529-1631 (mvx_super_frames_pelclip).  pelclip: [nframes*3] device planes of the clip's format,
 * rows aligned to pel samples.  mode 0 behaves like mvx_super_frames. */
int mvx_super_pelclip_mode(const mvx_super *s, int pelclip_width, int pelclip_height, int32_t *mode, char *err);
int mvx_super_frames_pelclip(mvx_super *s, int nframes, const void *const *src, const ptrdiff_t src_pitch[3],
                             const void *const *pelclip, const ptrdiff_t pelclip_pitch[3], int pelclip_mode,
                             void *const *dst, const ptrdiff_t dst_pitch[3], void *stream);

/* ---- mv.Finest -----------------------------------------------------------------------------------
 * replaces mvfinestGetFrame, MVFinest.c:48-140 (arg string :213-218): the pel^2 sub-pel planes of level 0 of a super frame
 * interleaved into one plane of (width + 2 hpad) * pel x (height + 2 vpad) * pel samples (chroma planes subsampled like
 * the clip).  Planes the super clip does not carry (chroma=0) are not written.  Layouts: super and dst pitches that hold a row of
 * their plane, super and dst planes at any address, all multiples of the sample size; U and V may differ ("mvx_finest_frames: pitches
 * must hold a row of their plane and be multiples of the sample size", "... planes are required and must be aligned to the sample
 * size", MVX_E_ARG before anything is launched).  Only the samples of dst are written. */
void mvx_finest_size(const mvx_super *s, int32_t *width, int32_t *height);
int mvx_finest_frames(const mvx_super *s, int nframes, const void *const *super_frames /* [f*3+p] */, const ptrdiff_t super_pitch[3],
                      void *const *dst /* [f*3+p] */, const ptrdiff_t dst_pitch[3], void *stream);

/* ---- mv.Analyse ----------------------------------------------------------------------------------
 * replaces mvanalyseCreate / mvanalyseGetFrame, MVAnalyse.c:267-635 / :76-254 (argument string :639-671);
 * the search itself is GroupOfPlanes.c:69-125 + PlaneOfBlocks.cpp:419-1131,1447-1636.                */

typedef struct mvx_analyse_args { /* MVX_UNSET = not passed */
    int32_t blksize, blksizev, levels, search, searchparam, pelsearch, isb, lambda, chroma, delta, truemotion,
        lsad, plevel, global, pnew, pzero, pglobal, overlap, overlapv, divide, badsad, badrange, opt, meander,
        trymany, fields, tff, search_coarse, dct;
} mvx_analyse_args;

typedef struct mvx_analyse mvx_analyse;

int mvx_analyse_create(const mvx_analyse_args *args, const mvx_super *super_clip, int num_frames,
                       const ptrdiff_t super_pitch[3], mvx_analyse **out, char *err);
void mvx_analyse_destroy(mvx_analyse *a);
void mvx_analyse_get_data(const mvx_analyse *a, mvx_analysis_data *out); /* MVTools_MVAnalysisData */
int mvx_analyse_blob_size(const mvx_analyse *a);                          /* bytes of MVTools_vectors */

typedef struct mvx_analyse_job {
    const void *src[3]; /* super frame n (device) */
    const void *ref[3]; /* super frame n +/- delta (device); ref[0]==NULL -> frame too close to the clip
                           boundary: the invalid/default blob is written (GroupOfPlanes.c:150-164) */
    void *blob;         /* device, mvx_analyse_blob_size() bytes, 16-byte aligned */
    int32_t field_shift;/* MVAnalyse.c:172-176; 0 unless fields=1 */
    int32_t reserved;
} mvx_analyse_job;

/* The caller promises that the super frames of every job (src and ref) carry their shadow planes (mvx_super_shadow_frames) at
 * plane[0] + copy_stride[0] and plane[1] + copy_stride[1]; NULL or all zero: none (the default).  Only changes which addresses the
 * search loads from, never a result. */
int mvx_analyse_set_ref_shadow(mvx_analyse *a, const ptrdiff_t copy_stride[3]);

/* One chain (frame, direction) per job; all jobs run concurrently in one launch. `jobs` is a HOST array.
 * With divide > 0 the blob carries the extra array of half-size blocks and mvx_analyse_get_data reports the divided
 * geometry (MVAnalyse.c:229, :615-624), which is what readers of the vector clip must use. */
int mvx_analyse_frames(mvx_analyse *a, int njobs, const mvx_analyse_job *jobs, void *stream);

/* dct = 1..4 of mv.Analyse / mv.Recalculate (the reference's FFTW block-DCT cost, DCTFFTW.cpp, PlaneOfBlocks.cpp:117-163) run as a float32
 * block DCT in HIP.  Opt-in for now: process-wide, off by default; while it is off both creates refuse these modes.
 * Call it once, before creating the filters.  Returns MVX_OK.  (Blocks up to 32x32.) */
int mvx_enable_dct_float(int on);

/* ---- mv.Recalculate ------------------------------------------------------------------------------
 * replaces mvrecalculateCreate / mvrecalculateGetFrame, MVRecalculate.c:263-545 / :68-254 (arg string :549-572);
 * the per-block refinement is PlaneOfBlocks.cpp:1158-1424, `divide` GroupOfPlanes.c:177-302.           */

typedef struct mvx_recalculate_args { /* MVX_UNSET = not passed */
    int64_t thsad, smooth, blksize, blksizev, search, searchparam, lambda, chroma, truemotion, pnew, overlap, overlapv,
        divide, meander, fields, dct;
} mvx_recalculate_args;

typedef struct mvx_recalculate mvx_recalculate;

/* `vectors_data`: MVTools_MVAnalysisData of the vector clip being refined */
int mvx_recalculate_create(const mvx_recalculate_args *args, const mvx_super *super_clip, const mvx_analysis_data *vectors_data,
                           const ptrdiff_t super_pitch[3], mvx_recalculate **out, char *err);
void mvx_recalculate_destroy(mvx_recalculate *r);
void mvx_recalculate_get_data(const mvx_recalculate *r, mvx_analysis_data *out); /* MVTools_MVAnalysisData of the result */
int mvx_recalculate_blob_size(const mvx_recalculate *r);

typedef struct mvx_recalculate_job {
    const void *src[3];   /* super frame n */
    const void *ref[3];   /* super frame n +/- delta; ref[0]==NULL -> the default (invalid) blob */
    const void *old_blob; /* MVTools_vectors of the old vector clip at frame n (device, 16-byte aligned) */
    void *blob;           /* out, mvx_recalculate_blob_size() bytes, 16-byte aligned */
} mvx_recalculate_job;

/* one workgroup per BLOCK: blocks of a Recalculate are independent (no spatial predictors) */
int mvx_recalculate_frames(mvx_recalculate *r, int njobs, const mvx_recalculate_job *jobs, void *stream);

/* ---- mv.Degrain1..6 ------------------------------------------------------------------------------
 * replaces mvdegrainCreate<r> / mvdegrainGetFrame<r>, MVDegrains.cpp:511-809 / :85-330 (arg strings :813-932) */

typedef struct mvx_degrain_args {
    int32_t radius;           /* 1..6 */
    int64_t thsad, thsadc;    /* MVX_UNSET -> 400 / thsad */
    int32_t plane, limit, limitc;
    int64_t thscd1; int32_t thscd2;
} mvx_degrain_args;

typedef struct mvx_degrain mvx_degrain;

int mvx_degrain_create(const mvx_degrain_args *args, const mvx_analysis_data *vectors_data /* of mvbw */,
                       const mvx_super *super_clip, const ptrdiff_t src_pitch[3], const ptrdiff_t super_pitch[3],
                       const ptrdiff_t dst_pitch[3], mvx_degrain **out, char *err);
void mvx_degrain_destroy(mvx_degrain *d);
/* The caller promises that every reference super frame of every job carries the shifted copy of its luma plane at plane[0] +
 * copy_stride[0] (mvx_super_shadow_frames; clips of more than 8 bits); NULL or zero: none (the default).  Blocks that start at an odd
 * sample are then read from the copy, at dword-aligned addresses.  Only changes which addresses are loaded, never a result.
 * (no reference counterpart: memory layout only) */
int mvx_degrain_set_ref_shadow(mvx_degrain *d, const ptrdiff_t copy_stride[3]);

typedef struct mvx_degrain_job {
    const void *src[3];          /* clip frame n */
    const void *refs[12][3];     /* super frame n+delta (mvbw), n-delta (mvfw), ... order mvbw,mvfw,mvbw2,mvfw2..;
                                    refs[r][0] may be NULL when that frame is outside the clip */
    const void *blobs[12];       /* MVTools_vectors of vector clip r at frame n (device) */
    void *dst[3];
} mvx_degrain_job;

int mvx_degrain_frames(mvx_degrain *d, int nframes, const mvx_degrain_job *jobs, void *stream);

/* ---- mv.DegrainN: temporal radius 1..24 ------------------------------------------------------------
 * No reference counterpart by name: the reference registers Degrain1..6 only, but its arithmetic is a template over the radius
 * (Degrain_C<radius> MVDegrains.h:30-53, useBlock :192-206, DegrainWeight :184-189, normaliseWeights<radius> :208-223), and this is that
 * template read at any radius, with the frame loop of mvdegrainGetFrame (MVDegrains.cpp:85-330).  Reference r (order mvbw, mvfw, mvbw2,
 * mvfw2, ...) has temporal distance d = r / 2 + 1 and is weighed against the threshold of ITS distance: thsad at d = 1, thsad2 at
 * d = radius, t_d = floor(thsad2 + (thsad - thsad2) * (1 + cos(pi * (d - 1) / (radius - 1))) / 2 + 0.5) in between (MDegrainN's thSAD2;
 * radius 1 or thsad2 == thsad: thsad everywhere), each then scaled like thsad (MVDegrains.cpp:658-661).  With thsad2 / thsadc2 unset and
 * radius <= 6 the output bytes are those of mvx_degrain_frames.  Messages are mvx_degrain_create's with the name DegrainN, in the same order. */

#define MVX_DEGRAIN_N_MAX_RADIUS 24

typedef struct mvx_degrain_n_args {
    int32_t radius;           /* 1..MVX_DEGRAIN_N_MAX_RADIUS */
    int64_t thsad, thsadc;    /* MVX_UNSET -> 400 / thsad, as Degrain */
    int64_t thsad2, thsadc2;  /* threshold at distance `radius`; MVX_UNSET -> thsad / thsadc (no fall-off) */
    int32_t plane, limit, limitc;
    int64_t thscd1; int32_t thscd2;
} mvx_degrain_n_args;

typedef struct mvx_degrain_n_info { /* what creation resolved */
    int32_t radius, nrefs;
    int64_t thsad_d[MVX_DEGRAIN_N_MAX_RADIUS], thsadc_d[MVX_DEGRAIN_N_MAX_RADIUS]; /* per distance 1..radius, AFTER the block-size scaling */
} mvx_degrain_n_info;

typedef struct mvx_degrain_n mvx_degrain_n;

/* touches no device */
int mvx_degrain_n_create(const mvx_degrain_n_args *args, const mvx_analysis_data *vectors_data /* of mvbw */,
                         const mvx_super *super_clip, const ptrdiff_t src_pitch[3], const ptrdiff_t super_pitch[3],
                         const ptrdiff_t dst_pitch[3], mvx_degrain_n **out, char *err);
/* out16 (pinterf's MVTools2 has it as out16=true on MDegrain and MDegrainN; no counterpart in the reference): an 8-bit clip, an 8-bit
 * super clip and vectors analysed on 8-bit samples -- SADs, thsad, thsad2, thscd1 and thscd2 in 8-bit units, the weights those of
 * mvx_degrain_n_create -- written as 16-bit planes; dst_pitch is THEIR pitch.  The output is byte for byte what the 16-bit arithmetic above
 * gives when every source and super sample is shifted left by 8 and every block carries the weights of the 8-bit run:
 *   block value      S = WSrc * src + sum of W_r * ref_r, 0..65280: no + 128, no shift ((128 + 256 * S) >> 8 = S)
 *   overlap 0        out = S
 *   overlap > 0      acc += (S * win) >> 6 in 32 bits (NOT the 16-bit wrap of the 8-bit path); out = min(65535, (acc + 16) >> 5)
 *   limit / limitc   in units of the output: 0..65535, MVX_UNSET -> 65535 (none) / limit; below 65535 out is clamped to
 *                    [(src << 8) - limit, (src << 8) + limit]
 *   passed through   a plane that `plane` leaves out, the strips no block covers, a job without a usable reference: out = src << 8
 * Messages are mvx_degrain_n_create's, and after the frame-size check "DegrainN: out16 needs an 8 bit clip." for any other super clip.
 * Touches no device.  The object is used and destroyed like one of mvx_degrain_n_create. */
int mvx_degrain_n_create_out16(const mvx_degrain_n_args *args, const mvx_analysis_data *vectors_data /* of mvbw */,
                               const mvx_super *super_clip, const ptrdiff_t src_pitch[3], const ptrdiff_t super_pitch[3],
                               const ptrdiff_t dst_pitch[3] /* of the 16-bit planes */, mvx_degrain_n **out, char *err);
/* DegrainN on a 32-bit float clip: the clip, the super clip (mvx_super_create_float) and the output are float32 planes; the vectors come from
 * a search on ANY 8..16 bit clip of the same width, height, pel, padding and subsampling (Analyse / AnalyseN / RecalculateN, or a result of
 * ScaleVect).  thsad, thsad2, thscd1 and thscd2 are in the units of that search and resolved from vectors_data; usable blocks, weights,
 * normalisation and lists are exactly those of mvx_degrain_n_create for these blobs.  Arithmetic of a sample, float32, every operation rounded
 * on its own, s the source sample, the list in its stored order:
 *   block value      S = (float)WSrc * s; for each entry S = S + (float)w_k * ref_k; V = S * (1/256.0f)
 *   overlap 0        out = V
 *   overlap > 0      acc = 0; over the covering blocks (by outer, bx inner, ascending) acc = acc + V * (float)win; out = acc / (float)wsum with
 *                    wsum the integer sum of those same window weights (2047..2049: dividing by it keeps a flat area flat)
 *   limit / limitc   on the 8-bit scale 0..255, MVX_UNSET -> 255 (none) / limit; below 255: L = (float)limit / 255.0f,
 *                    out = max(s - L, min(s + L, out))
 *   passed through   bit for bit: a plane that `plane` leaves out, the strips no block covers, a job without a usable reference
 * Inputs are assumed finite (no NaN, no infinity).  Messages are mvx_degrain_n_create's in its order, and after the frame-size check
 * "DegrainN: the float entry needs a float super clip."; the limits' messages name 255.  Planes and pitches must be multiples of 4 bytes.
 * Touches no device.  The object is used and destroyed like one of mvx_degrain_n_create; mvx_degrain_n_out_bits returns 32. */
int mvx_degrain_n_create_float(const mvx_degrain_n_args *args, const mvx_analysis_data *vectors_data /* of mvbw */,
                               const mvx_super *super_clip /* float */, const ptrdiff_t src_pitch[3], const ptrdiff_t super_pitch[3],
                               const ptrdiff_t dst_pitch[3], mvx_degrain_n **out, char *err);
/* bits per sample of the planes mvx_degrain_n_frames writes: 16 for an out16 object, 32 for a float one, else the clip's depth */
int mvx_degrain_n_out_bits(const mvx_degrain_n *d);
void mvx_degrain_n_get_info(const mvx_degrain_n *d, mvx_degrain_n_info *info);
void mvx_degrain_n_destroy(mvx_degrain_n *d);

typedef struct mvx_degrain_n_job {
    const void *src[3];              /* clip frame n */
    const void *const (*refs)[3];    /* HOST array of 2 * radius entries: super frame n+1 (mvbw), n-1 (mvfw), n+2, n-2, ...;
                                        refs[r][0] NULL = that frame is outside the clip */
    const void *const *blobs;        /* HOST array of 2 * radius device pointers: MVTools_vectors of vector clip r at frame n */
    void *dst[3];
} mvx_degrain_n_job;

/* the host arrays behind refs and blobs are read before the call returns; serves objects of both create functions */
int mvx_degrain_n_frames(mvx_degrain_n *d, int nframes, const mvx_degrain_n_job *jobs, void *stream);

/* ---- mv.Compensate -------------------------------------------------------------------------------
 * replaces mvcompensateCreate / mvcompensateGetFrame, MVCompensate.c:419-575 / :73-374 (arg string :579-592) */

typedef struct mvx_compensate_args {
    int32_t scbehavior;  /* MVX_UNSET -> 1 */
    int64_t thsad;       /* MVX_UNSET -> 10000 */
    double time;         /* 0..100, pass 100.0 for the default */
    int64_t thscd1; int32_t thscd2;
    int32_t fields;      /* MVX_UNSET/0 -> off; 1 needs pel > 1 (MVCompensate.c:514-517) */
} mvx_compensate_args;

typedef struct mvx_compensate mvx_compensate;

int mvx_compensate_create(const mvx_compensate_args *args, const mvx_analysis_data *vectors_data,
                          const mvx_super *super_clip, const ptrdiff_t super_pitch[3], const ptrdiff_t dst_pitch[3],
                          mvx_compensate **out, char *err);
void mvx_compensate_destroy(mvx_compensate *c);

typedef struct mvx_compensate_job {
    const void *src_super[3]; /* super frame n */
    const void *ref_super[3]; /* super frame nref; [0]==NULL if outside the clip */
    const void *blob;         /* MVTools_vectors at frame n */
    void *dst[3];
    int32_t field_shift;      /* MVCompensate.c:188-225: +-pel/2 when fields=1, pel>1, (nref-n) odd and the field parities differ; else 0 */
    int32_t reserved;
} mvx_compensate_job;

/* At most 32767 jobs per call ("mvx_compensate_frames: at most 32767 jobs per call", for a float object with " on float clips" behind it as
 * before; MVX_E_ARG, before a job is looked at): a launch holds
 * (job, chroma plane) in one grid dimension of 65535.  A job whose ref_super[0] is NULL needs no blob. */
int mvx_compensate_frames(mvx_compensate *c, int nframes, const mvx_compensate_job *jobs, void *stream);

/* Compensate on a 32-bit float clip, for ONE vector clip of any isb and delta: the single-field form of mvx_compensate_n_create_float (below),
 * whose arithmetic table, layout rules and notes on the vectors hold here word for word -- one field and one output per job, no centre; the
 * output is bit for bit output k of mvx_compensate_n_frames for the same (source, reference, field).  Messages are mvx_compensate_create's in
 * their order, after the frame-size check "Compensate: the float entry needs a float super clip."; fields = 1 is refused last with
 * "Compensate: fields is not supported on float clips.".  Touches no device.  mvx_compensate_frames and mvx_compensate_destroy serve the
 * object; for it mvx_compensate_frames also refuses a job whose field_shift is not 0 ("mvx_compensate_frames: field_shift is not supported
 * on float clips") and a job without a blob. */
int mvx_compensate_create_float(const mvx_compensate_args *args, const mvx_analysis_data *vectors_data,
                                const mvx_super *super_clip /* float */, const ptrdiff_t super_pitch[3], const ptrdiff_t dst_pitch[3],
                                mvx_compensate **out, char *err);

/* ---- the multi blob, mv.AnalyseN and mv.CompensateN: one source frame against a temporal radius ------
 * No reference counterpart: pinterf's MAnalyse(multi=true, delta=tr) / MCompensate(tr=...) and mvtools-sf's Analyze(radius=...) /
 * Compensate(tr=...) are the models.  Nothing new is computed: every field is one mvx_analyse_frames result and every compensated frame
 * one mvx_compensate_frames result, byte for byte.
 *
 * The multi blob: ONE device buffer per source frame with 2 * radius fields.  Field r has isb = (r % 2 == 0) and delta = r / 2 + 1 --
 * mvbw1, mvfw1, mvbw2, mvfw2, ..., the order of mvx_degrain_n_job -- and starts at byte r * field_stride, where field_stride is
 * mvx_analyse_blob_size rounded up to 256.  Each field is a complete MVTools_vectors blob: blob + r * field_stride can be handed to any
 * consumer of this header unchanged.  The bytes between a field's end and the next field are never written. */

typedef struct mvx_analyse_n mvx_analyse_n;

/* radius 1..MVX_DEGRAIN_N_MAX_RADIUS ("AnalyseN: radius must be between 1 and 24."); args->isb and args->delta must be MVX_UNSET ("AnalyseN:
 * isb and delta are set by the radius."); every other message is mvx_analyse_create's with the name AnalyseN, in the same order, and
 * dct 1..4 stay behind mvx_enable_dct_float.  Touches no device. */
int mvx_analyse_n_create(const mvx_analyse_args *args, int radius, const mvx_super *super_clip, int num_frames,
                         const ptrdiff_t super_pitch[3], mvx_analyse_n **out, char *err);
void mvx_analyse_n_destroy(mvx_analyse_n *a);
/* the MVTools_MVAnalysisData of field r: what an mvx_analyse created with that field's isb and delta reports; MVX_E_ARG for r outside 0..2 * radius - 1 */
int mvx_analyse_n_get_data(const mvx_analyse_n *a, int r, mvx_analysis_data *out);
size_t mvx_analyse_n_field_size(const mvx_analyse_n *a);   /* bytes of one field: mvx_analyse_blob_size */
size_t mvx_analyse_n_field_stride(const mvx_analyse_n *a); /* field_size rounded up to 256 */
size_t mvx_analyse_n_blob_size(const mvx_analyse_n *a);   /* 2 * radius * field_stride */
int mvx_analyse_n_set_ref_shadow(mvx_analyse_n *a, const ptrdiff_t copy_stride[3]); /* as mvx_analyse_set_ref_shadow */

typedef struct mvx_analyse_n_job {
    const void *src[3];              /* super frame n (device) */
    const void *const (*refs)[3];    /* HOST array of 2 * radius entries: super frame n+1, n-1, n+2, n-2, ...; refs[r][0] NULL = that frame is
                                        outside the clip: field r is the invalid blob mvx_analyse_frames writes for a NULL reference */
    void *blob;                      /* device, mvx_analyse_n_blob_size() bytes, 16-byte aligned */
    const int32_t *field_shift;      /* HOST array of 2 * radius values (mvx_analyse_job.field_shift per field), or NULL: field_shift_all everywhere */
    int32_t field_shift_all;
    int32_t reserved;
} mvx_analyse_n_job;

/* All 2 * radius * njobs searches of the call go to the device as ONE mvx_analyse_frames batch (the search picks its launch form from the
 * number of chains in a launch).  `jobs` and the arrays behind refs and field_shift are HOST arrays, read before the call returns. */
int mvx_analyse_n_frames(mvx_analyse_n *a, int njobs, const mvx_analyse_n_job *jobs, void *stream);

typedef struct mvx_compensate_n mvx_compensate_n;

/* tr 1..MVX_DEGRAIN_N_MAX_RADIUS ("CompensateN: tr must be between 1 and 24."); then mvx_compensate_create's messages with the name
 * CompensateN, in the same order; fields = 1 is refused last with "CompensateN: fields is not supported.".  vectors_data: of field 0
 * (every field shares its geometry).  Touches no device. */
int mvx_compensate_n_create(const mvx_compensate_args *args, int tr, const mvx_analysis_data *vectors_data /* of field 0 */,
                            const mvx_super *super_clip, const ptrdiff_t super_pitch[3], const ptrdiff_t dst_pitch[3],
                            mvx_compensate_n **out, char *err);
void mvx_compensate_n_destroy(mvx_compensate_n *c);
/* output k (0..2 * tr) of a job in temporal order: *offset = k - tr (the frame n + offset), *field = the field of the multi blob that
 * compensates it -- mvfw of distance tr - k before the centre, mvbw of distance k - tr behind it --, -1 for the centre.  MVX_E_ARG for k outside. */
int mvx_compensate_n_map(const mvx_compensate_n *c, int k, int *offset, int *field);

typedef struct mvx_compensate_n_job {
    const void *src_super[3];        /* super frame n */
    const void *const (*refs)[3];    /* HOST array of 2 * tr entries in the order of mvx_analyse_n_job; refs[r][0] NULL = outside the clip */
    const void *blob;                /* the multi blob of frame n (device) */
    size_t field_stride;             /* mvx_analyse_n_field_stride of the object that wrote it */
    void *const (*dst)[3];           /* HOST array of 2 * tr + 1 frames, output k in temporal order */
} mvx_compensate_n_job;

/* Output k != tr is byte for byte what mvx_compensate_frames writes for (src_super, refs[field], blob + field * field_stride) with the same
 * scbehavior, thsad, time, thscd1 and thscd2 -- a reference outside the clip and a scene change per scbehavior included.  Output tr is the
 * source: the unpadded pel-0 window of the finest level of src_super, copied.  One usable pass and one plan pass over all fields of all
 * jobs, then one output kernel per plane class whose grid covers the 2 * tr + 1 planes of every job (csrc/mvx_compensate.hip, the engine
 * of mvx_compensate_frames too). */
int mvx_compensate_n_frames(mvx_compensate_n *c, int njobs, const mvx_compensate_n_job *jobs, void *stream);

/* CompensateN on a 32-bit float clip: the super clip (mvx_super_create_float) and the outputs are float32 planes; vectors_data and the multi
 * blob come from a search on ANY 8..16 bit clip of the same width, height, pel, padding and subsampling (AnalyseN / RecalculateN, or fields
 * that ScaleVect wrote).  thsad, thscd1 and thscd2 are in the units of that search and resolved from vectors_data; which fields are usable,
 * where a block comes from (its vector scaled by time, or its own place at sad >= thsad) and the output -> field map are exactly those of
 * mvx_compensate_n_create for the same blob.  A sample, float32, every operation rounded on its own:
 *   centre output                a plain load and store of the unpadded pel-0 window of src_super, bit for bit
 *   unusable field               (scene change per thscd1 / thscd2, invalid blob, reference outside the clip) the same plain copy: the
 *                                reference at scbehavior 0 where there is one, else the source
 *   strips no block covers       the same plain copy: the source at scbehavior 1, the reference at 0
 *   blocks side by side          (overlap 0) the same plain copy of the block's samples from where its vector points
 *   overlapped blocks            acc = 0; over the covering blocks (by outer, bx inner, ascending) acc = acc + v * (float)win; out = acc /
 *                                (float)wsum with wsum the integer sum of those same window weights (2047..2049), as in
 *                                mvx_degrain_n_create_float: no >> 6 per term, no rounding term, no clamp, no 16-bit wrap
 *   a cell cut by the frame's edge   sample by sample, the same values
 * Copies move bytes and never look at them; samples may be negative or overshoot.  Inputs of overlapped blocks are assumed finite.
 * Messages are mvx_compensate_n_create's in their order, after the frame-size check "CompensateN: the float entry needs a float super clip.",
 * and "CompensateN: fields is not supported." stays last.  Touches no device.  mvx_compensate_n_map, mvx_compensate_n_frames and
 * mvx_compensate_n_destroy serve the object.  Layouts in mvx_compensate_n_frames: dst planes at any pitch that holds a row and any address,
 * both multiples of 4; super planes with pitches and addresses that are multiples of 16; everything else is refused before a launch. */
int mvx_compensate_n_create_float(const mvx_compensate_args *args, int tr, const mvx_analysis_data *vectors_data /* of field 0 */,
                                  const mvx_super *super_clip /* float */, const ptrdiff_t super_pitch[3], const ptrdiff_t dst_pitch[3],
                                  mvx_compensate_n **out, char *err);

/* ---- mv.RecalculateN: a multi blob refined field by field -------------------------------------------
 * No reference counterpart: pinterf's MRecalculate(tr=...) is the model.  Field r of the new multi blob is one mvx_recalculate_frames result
 * on field r of the old one, byte for byte.  As in AnalyseN a field's isb and delta only label its MVTools_MVAnalysisData, so ONE
 * mvx_recalculate serves every field. */

typedef struct mvx_recalculate_n mvx_recalculate_n;

/* radius 1..MVX_DEGRAIN_N_MAX_RADIUS ("RecalculateN: radius must be between 1 and 24."); vectors_data: of field 0 of the old multi blob, so
 * backward with delta 1 ("RecalculateN: vectors_data must be field 0 of a multi blob."); every other message is mvx_recalculate_create's with
 * the name RecalculateN, in the same order, and dct 1..4 stay behind mvx_enable_dct_float.  Touches no device. */
int mvx_recalculate_n_create(const mvx_recalculate_args *args, int radius, const mvx_super *super_clip, const mvx_analysis_data *vectors_data,
                             const ptrdiff_t super_pitch[3], mvx_recalculate_n **out, char *err);
void mvx_recalculate_n_destroy(mvx_recalculate_n *r);
/* the MVTools_MVAnalysisData of field r of the result: what an mvx_recalculate created on field r's old data reports; MVX_E_ARG for r
 * outside 0..2 * radius - 1 */
int mvx_recalculate_n_get_data(const mvx_recalculate_n *rn, int r, mvx_analysis_data *out);
size_t mvx_recalculate_n_field_size(const mvx_recalculate_n *r);   /* bytes of one field: mvx_recalculate_blob_size */
size_t mvx_recalculate_n_field_stride(const mvx_recalculate_n *r); /* field_size rounded up to 256 */
size_t mvx_recalculate_n_blob_size(const mvx_recalculate_n *r);    /* 2 * radius * field_stride */

typedef struct mvx_recalculate_n_job {
    const void *src[3];              /* super frame n (device) */
    const void *const (*refs)[3];    /* HOST array of 2 * radius entries in the order of mvx_analyse_n_job; refs[r][0] NULL = that frame is
                                        outside the clip: field r is the invalid blob mvx_recalculate_frames writes for a NULL reference */
    const void *old_blob;            /* the old multi blob of frame n (device, 16-byte aligned) */
    size_t old_field_stride;         /* field stride of the object that wrote it (a multiple of 16) */
    void *blob;                      /* device, mvx_recalculate_n_blob_size() bytes, 16-byte aligned */
} mvx_recalculate_n_job;

/* All 2 * radius * njobs refinements of the call go to the device as ONE mvx_recalculate_frames call.  `jobs` and the arrays behind refs are
 * HOST arrays, read before the call returns.  The bytes between a field's end and the next field are never written. */
int mvx_recalculate_n_frames(mvx_recalculate_n *r, int njobs, const mvx_recalculate_n_job *jobs, void *stream);

/* ---- mv.ScaleVect: the vectors of a small clip rewritten for a clip 1, 2 or 4 times its size --------------
 * No reference counterpart: pinterf's MScaleVect is the model (search on a small clip, or on an 8-bit copy of a 16-bit clip, and use the
 * vectors at full size).  The target clip is named by its mvx_super, so no consumer can be handed a vector that points outside that super
 * clip's padding.  With s = scale, `in` the vectors' MVTools_MVAnalysisData and si the target's mvx_super_info, creation refuses, in this
 * order:
 *   "ScaleVect: scale must be 1, 2 or 4."
 *   "ScaleVect: the target super clip must be scale times the size of the vectors' clip."    si.width != s * nWidth, si.height != s * nHeight or
 *                                                                                            si.super_width - 2 * si.hpad != s * nWidth
 *   "ScaleVect: the target super clip's chroma subsampling or colour data is not that of the vectors."   xRatioUV / yRatioUV differ, or the SADs
 *                                                                                            include chroma (nMotionFlags) and the super clip carries none
 *   "ScaleVect: the scaled block size must be 4x4, 8x4, ..."                                 s * nBlkSizeX x s * nBlkSizeY is not in mvx_recalculate_create's list
 *   "ScaleVect: scale times the target's pel must be a multiple of the vectors' pel."        the vector factor m = s * si.pel / nPel is no positive integer
 * The data of the scaled clip (mvx_scale_vect_get_data): nBlkSizeX/Y, nOverlapX/Y, nWidth and nHeight times s; nPel = si.pel; bitsPerSample =
 * si.bits; nHPadding / nVPadding = si.hpad / si.vpad; every other field copied (magic key, version, nLvCount, nDeltaFrame, isBackward, both
 * flag words, nBlkX/Y, the ratios).  It is what mvx_analyse_create reports on the target super clip with blksize * s, overlap * s and the
 * same levels, isb and delta.  The block grid of EVERY level is that of `in`, so mvx_vectors_size is unchanged and a scaled blob has the
 * layout of its input byte for byte (checked at creation).
 * A blob whose validity word is 0 is copied.  In a valid blob the two header words and the per-level size words are copied and every
 * record of every level becomes
 *   x' = x * m, y' = y * m                     (in 64 bits)
 *   sad' = sad * s * s << (si.bits - bitsPerSample)   (64-bit two's complement; an arithmetic shift to the right where the difference is negative)
 * and on level 0 x' and y' are then clamped into the block's legal rectangle on the target super clip, -(pos + pad) * pel ..
 * (size + pad - pos - blk) * pel - 1 per axis (PlaneOfBlocks.cpp's nDxMin .. nDxMax - 1).  The clamp changes nothing when the target's
 * padding is at least s times the small clip's; when it is not it is what keeps Degrain, Compensate and Flow inside the super frame.
 * Coarser levels are scaled and not clamped: no consumer of this header reads them.  The scaled SADs are ESTIMATES (a SAD of the small clip
 * times the area ratio and the depth ratio): mvx_recalculate_frames at full size replaces them with true SADs and refines the vectors, which
 * is the usual chain.  Vector clips made with divide > 0 are not supported: their level sizes are not those of the level formula.
 * Touches no device at creation. */

typedef struct mvx_scale_vect mvx_scale_vect;

int mvx_scale_vect_create(const mvx_analysis_data *in, int scale, const mvx_super *target, mvx_scale_vect **out, char *err);
void mvx_scale_vect_destroy(mvx_scale_vect *h);
void mvx_scale_vect_get_data(const mvx_scale_vect *h, mvx_analysis_data *out); /* MVTools_MVAnalysisData of the scaled clip */

typedef struct mvx_scale_vect_job {
    const void *in;       /* device: a blob of mvx_vectors_size(in) bytes, or a multi blob; 4-byte aligned */
    void *out;            /* device, as large as in; out == in scales in place, any other overlap is not allowed */
    int32_t fields;       /* 1: an ordinary blob; 2 * radius: every field of a multi blob */
    size_t field_stride;  /* of the multi blob, the same on both sides (a multiple of 4; unused when fields is 1); the bytes between a
                             field's end and the next field are neither read nor written */
} mvx_scale_vect_job;

/* ONE launch for all fields of all jobs (csrc/mvx_scale_vect.hip), asynchronous on `stream`; `jobs` is a HOST array, read before the call
 * returns.  As in RecalculateN a field's isBackward and nDeltaFrame only label its MVTools_MVAnalysisData: ONE object serves every field of
 * a multi blob, and the caller reads the labels off the object that produced the field (mvx_analyse_n_get_data). */
int mvx_scale_vect_frames(mvx_scale_vect *h, int njobs, const mvx_scale_vect_job *jobs, void *stream);

/* ---- mv.BlockFPS ---------------------------------------------------------------------------------
 * replaces mvblockfpsCreate / mvblockfpsGetFrame, MVBlockFPS.c:741-1014 / :229-676 (arg string :1017-1033);
 * masks MaskFun.cpp:63-166, mask upsizer SimpleResize.cpp:27-121.                                     */

typedef struct mvx_blockfps_args {
    int64_t num, den;        /* MVX_UNSET -> 25 / 1; 0 -> double the input rate */
    int32_t mode;            /* 0..8, MVX_UNSET -> 3 */
    double ml;               /* pass 100.0 for the default */
    int32_t blend;           /* MVX_UNSET -> 1 */
    int64_t thscd1; int32_t thscd2;
} mvx_blockfps_args;

typedef struct mvx_blockfps_info { int32_t num_frames; int64_t fps_num, fps_den; } mvx_blockfps_info; /* of the output clip */

typedef struct mvx_blockfps mvx_blockfps;

/* fps_num / fps_den: frame rate of the input clip (the reference refuses clips without one) */
int mvx_blockfps_create(const mvx_blockfps_args *args, const mvx_analysis_data *mvbw, const mvx_analysis_data *mvfw,
                        const mvx_super *super_clip, int num_frames, int64_t fps_num, int64_t fps_den,
                        const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3],
                        mvx_blockfps **out, char *err);
void mvx_blockfps_destroy(mvx_blockfps *b);
void mvx_blockfps_get_info(const mvx_blockfps *b, mvx_blockfps_info *info);
/* output frame n -> the two input frames it lies between and its time position (MVBlockFPS.c:245-254,278-292) */
void mvx_blockfps_map(const mvx_blockfps *b, int n, int *nleft, int *nright, int *time256);

typedef struct mvx_blockfps_job {
    int32_t time256;             /* from mvx_blockfps_map; 0 / 256 copy clip_left / clip_right */
    int32_t reserved;
    const void *src_super[3];    /* super frame nleft  } all four NULL when nleft or nright lies outside the clip */
    const void *ref_super[3];    /* super frame nright }   (then, or when the vectors are unusable: blend / copy */
    const void *blob_fw;         /* mvfw vectors at nright }   of clip_left and clip_right, MVBlockFPS.c:640-673) */
    const void *blob_bw;         /* mvbw vectors at nleft  } */
    const void *clip_left[3];    /* clip frame min(nleft, last)  */
    const void *clip_right[3];   /* clip frame min(nright, last) */
    void *dst[3];
} mvx_blockfps_job;

int mvx_blockfps_frames(mvx_blockfps *b, int nframes, const mvx_blockfps_job *jobs, void *stream);

/* BlockFPS on a 32-bit float clip: the clip, the super clip (mvx_super_create_float) and the outputs are float32 planes; mvbw, mvfw and the
 * blobs come from a search on ANY 8..16 bit clip of the same width, height, pel, padding and subsampling.  thscd1, thscd2 and ml are in the
 * units of that search: which jobs are usable, the plan (the vectors scaled by the time position, divided by the subsampling ratio) and the
 * occlusion / SAD masks -- 8-bit integers, SADs shifted by mvbw's bitsPerSample - 8, upsized with the reference's integer tables -- are
 * exactly those of mvx_blockfps_create for the same blobs.  A sample, float32, nothing fused, every operation rounded on its own
 * (csrc/mvx_blockfps_float_rule.h), with t = time256, ft = (float)t, fu = (float)(256 - t), K = 1 / 256, sVal / rVal the level-0 samples of
 * the left / right super frame at the output position, b the fetch from the right super frame along the backward vector, fw the fetch from
 * the left one along the forward vector, mF, mB, mO the upsized masks (0..255), med(a, b, c) = max(min(a, b), min(max(a, b), c)) and
 * mix(m, p, q) = ((float)m * p + (float)(255 - m) * q) / 255, bb = mix(mB, fw, b), ff = mix(mF, b, fw):
 *   mode 0                       (b * ft + fw * fu) * K
 *   mode 1                       med(rVal, sVal, (b * ft + fw * fu) * K)
 *   mode 2                       med((rVal * ft + sVal * fu) * K, b, fw)
 *   mode 3, 6                    (bb * ft + ff * fu) * K
 *   mode 4, 7                    mix(mO, (rVal * ft + sVal * fu) * K, (bb * ft + ff * fu) * K)
 *   mode 5, 8                    (float)mO / 255 on every plane (the integer path writes mO << (bits - 8) to every plane too)
 *   blocks side by side          (overlap 0) the value itself
 *   overlapped blocks            acc = 0; over the covering blocks (by outer, bx inner, ascending) acc = acc + V * (float)win; out = acc /
 *                                (float)wsum with wsum the integer sum of those same window weights, as in mvx_degrain_n_create_float: no
 *                                >> 6 per term, no rounding term, no clamp, no 16-bit wrap
 *   strips no block covers       (sVal * fu + rVal * ft) * K
 *   job not usable               (time256 0 or 256, a scene change per thscd1 / thscd2, an invalid blob, a frame outside the clip) t <= 0, or
 *                                t < 256 at blend 0: clip_left, a plain load and store, bit for bit (NaN payloads survive); t >= 256:
 *                                clip_right likewise; otherwise (l * fu + r * ft) * K
 * The mask mixes divide by 255, the weights' own sum, where the reference's (... + 255) >> 8 is 8-bit arithmetic.  Minimum and maximum are
 * comparisons that return their second operand when neither is smaller / larger.  Inputs are assumed finite; samples may be negative or
 * overshoot.  Messages are mvx_blockfps_create's in their order; after the frame-size check "BlockFPS: the float entry needs a float super
 * clip."; then the library's own geometry and pitch checks.  mvx_blockfps_create itself keeps refusing a float super clip first of all.
 * Touches no device.  mvx_blockfps_get_info, mvx_blockfps_map, mvx_blockfps_frames and mvx_blockfps_destroy serve the object.  Layouts:
 * clip_left, clip_right and dst planes at any pitch that holds a row and any address, both multiples of 4; super planes with pitches and
 * addresses that are multiples of 16; mvx_blockfps_frames refuses everything else before a launch. */
int mvx_blockfps_create_float(const mvx_blockfps_args *args, const mvx_analysis_data *mvbw, const mvx_analysis_data *mvfw,
                              const mvx_super *super_clip /* float */, int num_frames, int64_t fps_num, int64_t fps_den,
                              const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3],
                              mvx_blockfps **out, char *err);

/* ---- mv.FlowInter / mv.FlowFPS -------------------------------------------------------------------
 * per-sample ("flow") interpolation between two frames; both filters share one handle type and one engine.
 * mvx_flowinter_create replaces mvflowinterCreate, MVFlowInter.c:473-678 (arg string :697-710);
 * mvx_flowfps_create replaces mvflowfpsCreate, MVFlowFPS.c:565-878 (arg string :889-903);
 * mvx_flow_frames replaces mvflowinterGetFrame / mvflowfpsGetFrame + FlowFPSHelper, MVFlowInter.c:80-452,
 * MVFlowFPS.c:86-524, MVFlowFPSHelper.c:49-93; masks and fields MaskFun.cpp:38-203, formulas MaskFun.cpp:349-555,
 * upsizers SimpleResize.cpp:27-121.  The super clip is read directly: no mv.Finest frame is needed.
 * Deliberate divergences: FlowFPS rejects vectors with absolute frame references (delta <= 0), which the reference
 * accepts and then reads negative frame numbers with; both reject frames less than two blocks wide or high, where the
 * reference's upsizer reads outside its buffers. */

typedef struct mvx_flowinter_args {
    double time;             /* percent of the way from frame n to n + delta, 0..100 (a float argument in the reference); pass 50.0 for the default */
    double ml;               /* mask scale (a float argument in the reference); pass 100.0 for the default */
    int32_t blend;           /* MVX_UNSET -> 1 */
    int64_t thscd1; int32_t thscd2;
} mvx_flowinter_args;

typedef struct mvx_flowfps_args {
    int64_t num, den;        /* MVX_UNSET -> 25 / 1; 0 -> double the input rate */
    int32_t mask;            /* 0..2, MVX_UNSET -> 2 */
    double ml;               /* pass 100.0 for the default */
    int32_t blend;           /* MVX_UNSET -> 1 */
    int64_t thscd1; int32_t thscd2;
} mvx_flowfps_args;

typedef struct mvx_flow_info { int32_t num_frames; int64_t fps_num, fps_den; } mvx_flow_info; /* of the output clip; FlowInter: 0 / 0 = the input's rate */

typedef struct mvx_flow mvx_flow;

int mvx_flowinter_create(const mvx_flowinter_args *args, const mvx_analysis_data *mvbw, const mvx_analysis_data *mvfw,
                         const mvx_super *super_clip, int num_frames, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3],
                         const ptrdiff_t dst_pitch[3], mvx_flow **out, char *err);
/* fps_num / fps_den: frame rate of the input clip (the reference refuses clips without one) */
int mvx_flowfps_create(const mvx_flowfps_args *args, const mvx_analysis_data *mvbw, const mvx_analysis_data *mvfw,
                       const mvx_super *super_clip, int num_frames, int64_t fps_num, int64_t fps_den,
                       const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3],
                       mvx_flow **out, char *err);
void mvx_flow_destroy(mvx_flow *h);
void mvx_flow_get_info(const mvx_flow *h, mvx_flow_info *info);
/* output frame n -> the two input frames it lies between and its time position: FlowInter (n, n + delta, time256),
 * MVFlowInter.c:86-100; FlowFPS as BlockFPS, MVFlowFPS.c:92-99,125-134 */
void mvx_flow_map(const mvx_flow *h, int n, int *nleft, int *nright, int *time256);

typedef struct mvx_flow_job {
    int32_t time256;             /* from mvx_flow_map; FlowFPS copies clip_left / clip_right at 0 / 256 (MVFlowFPS.c:138-142) */
    int32_t reserved;
    const void *super_left[3];   /* super frame nleft  } all four NULL when nright lies outside the clip (then, or when the */
    const void *super_right[3];  /* super frame nright }   vectors are unusable: Blend of clip_left and clip_right when */
    const void *blob_fw;         /* mvfw at nright     }   blend = 1, else clip_left, MVFlowInter.c:403-446) */
    const void *blob_bw;         /* mvbw at nleft      } */
    const void *blob_fw_extra;   /* mvfw at nleft  (NULL = unusable); read by FlowInter and FlowFPS mask = 2 only */
    const void *blob_bw_extra;   /* mvbw at nright (NULL = unusable) */
    const void *clip_left[3];    /* clip frame min(nleft, last)  */
    const void *clip_right[3];   /* clip frame min(nright, last) */
    void *dst[3];
} mvx_flow_job;

/* nframes jobs of one handle in one batch on `stream`: three small per-job kernels and a memset, then two gather launches that cover
 * all jobs: one for the luma planes, one for both chroma planes (Gray: the luma launch only) */
int mvx_flow_frames(mvx_flow *h, int nframes, const mvx_flow_job *jobs, void *stream);

/* FlowInter and FlowFPS on a 32-bit float clip: clip_left, clip_right and dst are float32 planes, super_left / super_right frames of a
 * mvx_super_create_float clip; mvbw, mvfw and the blobs come from a search on ANY 8..16 bit clip of the same width, height, pel, padding and
 * subsampling.  thscd1, thscd2 and ml are in the units of that search.  The reference has no float path; the arithmetic is the library's own.
 * Everything above the sample is the integer filter's, value for value, for the same blobs: which jobs are usable and which formula a job
 * takes (fl_state: FlowInter Regular or Extra; FlowFPS Simple at mask 0, Regular at mask 1, Extra at mask 2 and Simple where the extra vectors
 * are not usable), the occlusion masks, the padded cells, the int16 upsizer and the 8-bit mask upsizer at each sample, the fetch positions,
 * time256 and the FlowFPS rate map.  A sample, float32, nothing fused, every operation rounded on its own (csrc/mvx_flow_float_rule.h), with
 * t = time256, dF the fetch from the LEFT super frame along the forward vector scaled by t, dB the fetch from the RIGHT one along the backward
 * vector scaled by 256 - t, dF0 / dB0 the left / right super sample at the output position, dFF / dBB the Extra fetches (the forward vectors
 * at nleft on the left frame, the backward vectors at nright on the right one), mF / mB the upsized masks (0..255),
 * time(r, l, t) = (r * (float)t + l * (float)(256 - t)) * (1 / 256) and mix(m, p, q) = ((float)m * p + (float)(255 - m) * q) / 255:
 *   Simple  (MaskFun.cpp:493-551) time(mix(mB, dF, dB), mix(mF, dB, dF), t) at EVERY t.  There is no special formula at t = 128: the
 *                                reference's own, ((dF + dB) * 256 + (dB - dF) * (mF - mB)) >> 9, is the general one with its shifts merged
 *                                and 256 for the masks' 255 -- within peak / 512 of it before rounding -- and float32 has no shift to save
 *   Regular (:374-414)           a = mix(mF, mix(mB, dF0, dB), dF); b = mix(mB, mix(mF, dB0, dF), dB); time(b, a, t)
 *   Extra   (:417-490)           lo = min(dB, dF), hi = max(dB, dF), medBB = max(lo, min(dBB, hi)), medFF = max(lo, min(dFF, hi));
 *                                time(mix(mB, medFF, dB), mix(mF, medBB, dF), t)
 *   job not usable, blend 1      (a scene change per thscd1 / thscd2, an invalid blob, a frame outside the clip) time(r, l, t) on the clip
 *                                frames
 *   job not usable, blend 0      clip_left, a plain load and store of the 32 bits: NaN payloads and signed zeros survive
 *   FlowFPS t <= 0 / t >= 256    clip_left / clip_right likewise, bit for bit
 * The mask mixes divide by 255, the weights' own sum, where the reference's (... + 255) >> 8 is 8-bit arithmetic; there is no rounding term
 * and no clamp to a sample range.  Minimum and maximum are comparisons that return their second operand when neither is smaller / larger.
 * Inputs are assumed finite; samples may be negative or overshoot.  Messages are mvx_flowinter_create's / mvx_flowfps_create's, the
 * reference's, in their order -- arguments, thscd1, the two vector clips, for FlowFPS the frame rate and the two frame-size checks, "wrong
 * source or super clip frame size", for FlowFPS "inconsistent clips frame size" --; then "FlowInter: the float entry needs a float super
 * clip." / "FlowFPS: the float entry needs a float super clip."; then the library's own geometry and pitch checks ("at least two blocks
 * wide", U and V super pitch, super / clip / dst pitches with 4-byte samples), which the integer entries say before their frame-size checks.
 * mvx_flowinter_create and mvx_flowfps_create themselves keep refusing a float super clip first of all.  Touch no device.
 * mvx_flow_frames, mvx_flow_map, mvx_flow_get_info and mvx_flow_destroy serve the objects; the job struct is the same.  Layouts: clip_left,
 * clip_right and dst planes at any pitch that holds a row and any address, both multiples of 4; super planes with pitches and addresses that
 * are multiples of 16; mvx_flow_frames refuses everything else before a launch.  Samples are produced in segments of 4, 2 or 1 (the widest
 * that divides the plane width).  Not registered in the VapourSynth shell. */
int mvx_flowinter_create_float(const mvx_flowinter_args *args, const mvx_analysis_data *mvbw, const mvx_analysis_data *mvfw,
                               const mvx_super *super_clip /* float */, int num_frames, const ptrdiff_t super_pitch[3],
                               const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], mvx_flow **out, char *err);
int mvx_flowfps_create_float(const mvx_flowfps_args *args, const mvx_analysis_data *mvbw, const mvx_analysis_data *mvfw,
                             const mvx_super *super_clip /* float */, int num_frames, int64_t fps_num, int64_t fps_den,
                             const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3],
                             mvx_flow **out, char *err);

/* ---- mv.Flow / mv.FlowBlur ------------------------------------------------------------------------
 * per-sample motion compensation and motion blur on the flow machinery above (int16 vector upsizing per sample, the super clip
 * read as the Finest frame).
 * mvx_flowcomp_create replaces mvflowCreate, MVFlow.cpp:391-593; mvx_flowcomp_frames replaces mvflowGetFrame, MVFlow.cpp:163-370
 * (fetch :93-116, shift :119-148).  mvx_flowblur_create replaces mvflowblurCreate, MVFlowBlur.c:346-552; mvx_flowblur_frames replaces
 * mvflowblurGetFrame, MVFlowBlur.c:143-326 (RealFlowBlur :72-130).
 * Deliberate divergence: both reject frames less than two blocks wide or high, where the reference's upsizer reads outside its buffers. */

typedef struct mvx_flowcomp_args {
    double time;             /* percent of the vector, 0..100 (a double argument in the reference: time256 is formed in double); pass 100.0 for the default */
    int32_t mode;            /* 0 fetch, 1 shift; MVX_UNSET -> 0 */
    int32_t fields;          /* MVX_UNSET -> 0; the caller computes each job's field_shift from it */
    int64_t thscd1; int32_t thscd2;
} mvx_flowcomp_args;

typedef struct mvx_flowcomp mvx_flowcomp;

/* accepts vectors with absolute frame references (delta <= 0) */
int mvx_flowcomp_create(const mvx_flowcomp_args *args, const mvx_analysis_data *vectors, const mvx_super *super_clip, int num_frames,
                        const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], mvx_flowcomp **out, char *err);
void mvx_flowcomp_destroy(mvx_flowcomp *h);
/* the reference frame of output frame n: n +- delta by isb, or -delta for absolute references (MVFlow.cpp:170-176) */
int mvx_flowcomp_ref(const mvx_flowcomp *h, int n);

typedef struct mvx_flowcomp_job {
    const void *ref_super[3];    /* super frame mvx_flowcomp_ref(n); NULL (nref outside the clip) = copy clip */
    const void *blob;            /* vectors at n; NULL = copy clip; unusable vectors copy clip too (MVFlow.cpp:364-368) */
    const void *clip[3];         /* clip frame n */
    void *dst[3];
    int32_t field_shift;         /* MVFlow.cpp:264-302: +-pel/2 when fields=1, pel>1, (nref-n) odd and the field parities differ; else 0 */
    int32_t reserved;
} mvx_flowcomp_job;

/* nframes jobs of one handle in one batch on `stream`: two small per-job kernels, then one launch per kernel and plane class (luma / both
 * chroma planes) over all jobs.  Mode 1 (shift) scatters into a winner buffer of 8 bytes per sample and job, held by the handle and grown
 * to the largest call. */
int mvx_flowcomp_frames(mvx_flowcomp *h, int nframes, const mvx_flowcomp_job *jobs, void *stream);

typedef struct mvx_flowblur_args {
    double blur;             /* percent, 0..200 (a float argument in the reference: blur256 is formed in float); pass 50.0 for the default */
    int32_t prec;            /* >= 1; MVX_UNSET -> 1 */
    int64_t thscd1; int32_t thscd2;
} mvx_flowblur_args;

typedef struct mvx_flowblur mvx_flowblur;

int mvx_flowblur_create(const mvx_flowblur_args *args, const mvx_analysis_data *mvbw, const mvx_analysis_data *mvfw, const mvx_super *super_clip,
                        int num_frames, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], mvx_flowblur **out,
                        char *err);
void mvx_flowblur_destroy(mvx_flowblur *h);

typedef struct mvx_flowblur_job {
    const void *super[3];        /* super frame n; NULL = copy clip */
    const void *blob_bw;         /* mvbw at n - delta } NULL when n - delta < 0 or n + delta >= num_frames = copy clip; */
    const void *blob_fw;         /* mvfw at n + delta }   unusable vectors copy clip too (MVFlowBlur.c:158-178,318-322) */
    const void *clip[3];         /* clip frame n */
    void *dst[3];
} mvx_flowblur_job;

/* nframes jobs in one batch on `stream`: two small per-job kernels, then one launch for the luma planes and one for both chroma planes */
int mvx_flowblur_frames(mvx_flowblur *h, int nframes, const mvx_flowblur_job *jobs, void *stream);

/* Flow and FlowBlur on a 32-bit float clip: the clip, the super clip (mvx_super_create_float) and the outputs are float32 planes; the vector
 * clips and the blobs come from a search on ANY 8..16 bit clip of the same width, height, pel, padding and subsampling, and thscd1 / thscd2
 * are in the units of that search.  The reference has no float path; the arithmetic is the library's own.  Everything on the vector side is
 * the integer filter's, value for value, for the same blobs: which jobs are usable, the int16 cells, field_shift, the upsized vx / vy with
 * the resizer's limits, time256, blur256, prec, the tap count m and the tap positions.  Only how a sample is fetched, carried and averaged
 * differs, with s(X, Y) the float super sample at pel position (X, Y) (the super frame read as the Finest frame) and lp = log2(pel):
 *   Flow mode 0 (fetch)          out(x, y) = s((x << lp) + ((vx * time256 + 128) >> 8), (y << lp) + ((vy * time256 + 128) >> 8)), the 32 bits
 *                                copied as they are: no arithmetic at all
 *   Flow mode 1 (shift)          source sample s(x << lp, y << lp) goes to the integer filter's destination, and the last writer in raster
 *                                order wins as there: an atomic maximum of the key ((raster index + 1) << 32) | bits of the sample (the
 *                                index fits 32 bits: a legal plane has fewer than 2^32 samples).  The winner's bits are stored as they are;
 *                                where no source landed, the top of the plane's nominal range -- 1.0f on luma, 0.5f on chroma (centred on
 *                                0, as in mvx_super_create_float) -- stands where the integer filter writes pixel_max
 *   FlowBlur                     sum = s(X, Y); for the F taps, then the B taps, in the integer kernel's order: sum = sum + tap, float32,
 *                                each addition rounded on its own; out = sum / (float)(mF + mB + 1): one division, no reciprocal, nothing
 *                                fused, no clamp.  mF + mB == 0 gives the sample itself bit for bit (x / 1.0f)
 *   job not usable               (a scene change per thscd1 / thscd2, an invalid blob, a NULL super frame or blob) the clip frame, a plain
 *                                load and store, bit for bit: NaN payloads survive
 * Messages are mvx_flowcomp_create's / mvx_flowblur_create's in their order; after the frame-size check "Flow: the float entry needs a float
 * super clip." / "FlowBlur: the float entry needs a float super clip."; then the library's own geometry and pitch checks; fields = 1 is
 * refused last with "Flow: fields is not supported on float clips.".  mvx_flowcomp_create and mvx_flowblur_create themselves keep refusing a
 * float super clip first of all.  Touch no device.  mvx_flowcomp_frames / _ref / _destroy and mvx_flowblur_frames / _destroy serve the
 * objects; the job structs are the same.  Layouts: clip and dst planes at any pitch that holds a row and any address, both multiples of 4;
 * super planes with pitches and addresses that are multiples of 16; *_frames refuses everything else before a launch.  Samples are moved in
 * segments of 4, 2 or 1 (the widest that divides the plane width).  Not registered in the VapourSynth shell. */
int mvx_flowcomp_create_float(const mvx_flowcomp_args *args, const mvx_analysis_data *vectors, const mvx_super *super_clip /* float */,
                              int num_frames, const ptrdiff_t super_pitch[3], const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3],
                              mvx_flowcomp **out, char *err);
int mvx_flowblur_create_float(const mvx_flowblur_args *args, const mvx_analysis_data *mvbw, const mvx_analysis_data *mvfw,
                              const mvx_super *super_clip /* float */, int num_frames, const ptrdiff_t super_pitch[3],
                              const ptrdiff_t clip_pitch[3], const ptrdiff_t dst_pitch[3], mvx_flowblur **out, char *err);

/* ---- mv.Mask --------------------------------------------------------------------------------------
 * motion, SAD and occlusion masks from one vector clip, as an 8-bit three-plane clip.
 * mvx_mask_create replaces mvmaskCreate, MVMask.c:227-346 (arg string :349-363); mvx_mask_frames replaces mvmaskGetFrame,
 * MVMask.c:75-211 (mvmaskLength :66-72); masks MaskFun.cpp:85-166 (ByteOccMask, MakeVectorOcclusionMaskTime, ByteNorm,
 * MakeSADMaskTime), upsizer SimpleResize.cpp:27-121.  No super clip is needed; creation touches no device.
 * kind: 0 vector length, 1 SAD, 2 occlusion, 3 / 4 the x / y component (+128), 5 x in U and y in V with the clip's luma kept.
 * U and V are equal for kinds 0-4.  A frame whose vectors are unusable (scene change, invalid, NULL blob) is filled with ysc (kind 5:
 * chroma only).  Only the samples of each plane are written: bytes between a plane's width and its pitch are never touched (the
 * reference's memset / memcpy fallbacks write them).
 * The reference's `opt` chooses between C and AVX2 forms that compute the same bytes; it has no counterpart here.
 * 255 * pow(...) is the device's double-precision pow where the reference calls the C library's; the two may differ in the last
 * places, which changes a byte only where the product lies within that distance of an integer.  An exponent of exactly 1 (kinds 1 and
 * 2 at gamma 1, kind 0 at gamma 2) takes no pow at all, and is exact.
 * Deliberate divergences, each rejected at creation with a message of the library's own unless stated otherwise:
 *   1. fewer than two blocks wide or high: the reference's upsizer then reads before its buffer (as Flow);
 *   2. a clip whose size or chroma ratios differ from the vector clip's nWidth / nHeight / xRatioUV / yRatioUV (Gray counts as
 *      1 / 1): the reference does not check this, and then writes planes of the wrong size;
 *   3. (not rejected) where 255 * pow(...) of the occlusion mask exceeds the int range the reference's cast is undefined -- on
 *      x86 it yields INT_MIN, so the cell keeps its old value; the library saturates: the cell becomes 255.
 *
 * Deep masks (mvx_mask_create_deep): a clip of B = 9..16 bits gives three planes of B bits in 16-bit containers, so that a mask can be
 * merged by at the depth of the clip it was made for.  The semantics are the library's own; the reference refuses such clips
 * (MVMask.c:321), and no parity with any other MVTools is claimed.  With s = B - 8:
 *   - the block-resolution masks stay bytes, computed as above, except that kind 1 shifts the int64 SAD right by s (arithmetic) before
 *     it becomes a double: MakeSADMaskTime's own `sad >> (bitsPerSample - 8)`, MaskFun.cpp:162, which the reference's format check
 *     keeps from ever seeing anything but 0.  s comes from the clip argument; the vector clip's depth is not consulted (nor is it by
 *     mvx_mask_create, which never shifts: a 16-bit vector clip's SADs saturate an 8-bit mask);
 *   - the upsizer, its tables, the edge replication and the usability test work on bytes and give an 8-bit value m per sample;
 *   - each sample is stored as E(m).  Kinds 0-2 are weights, full at the clip's peak as merging filters read them, so they replicate
 *     their bits: E(m) = m << s | m >> (8 - s), monotone, 0 -> 0, 255 -> 2^B - 1.  Kinds 3-4 and kind 5's U and V are offsets from a
 *     neutral value, so they scale: E(m) = m << s, 128 -> 2^(B-1).  Two rules, because a replicated 128 would no longer be neutral and a
 *     scaled 255 would no longer be full.  Kind 5's luma is the clip's own, two bytes a sample;
 *   - ysc stays 0..255, in 8-bit units: an unusable frame is filled with E(ysc) by the rule of the plane filled.
 * Pitches are in bytes (clip_pitch[0] too), dst planes 16-byte aligned; only the samples are written, two bytes each.  At B = 8 a deep
 * object behaves byte for byte like mvx_mask_create's. */

typedef struct mvx_mask_args {
    double ml, gamma;        /* pass 100.0 / 1.0 for the defaults; float arguments in the reference: every factor is formed in float */
    int32_t kind;            /* 0..5, MVX_UNSET -> 0 */
    double time;             /* 0..100 (a double argument in the reference: time256 is formed in double); pass 100.0 for the default */
    int32_t ysc;             /* 0..255, MVX_UNSET -> 0 */
    int64_t thscd1; int32_t thscd2;
} mvx_mask_args;

/* the format of the clip argument (VSVideoInfo) */
typedef struct mvx_mask_clip { int32_t width, height, bits, subsampling_w, subsampling_h, gray; } mvx_mask_clip;

/* the output clip: always 3 planes, of 8 bits (of mvx_mask_out_bits for a deep object); a Gray input gives 4:4:4 (MVMask.c:328-329).  The remaining fields are what creation
 * derived from the arguments (MVMask.c:304-307,334), for hosts and tests that want to see the rounding. */
typedef struct mvx_mask_info {
    int32_t width, height, subsampling_w, subsampling_h, num_planes;
    int32_t plane_width[3], plane_height[3];
    int32_t time256;
    float fMaskNormFactor, fMaskNormFactor2, fHalfGamma;
} mvx_mask_info;

typedef struct mvx_mask mvx_mask;

/* clip_pitch[0]: row pitch of the clip's luma plane (read by kind 5 only); dst_pitch: multiples of 16 bytes, U and V alike */
int mvx_mask_create(const mvx_mask_args *args, const mvx_analysis_data *vectors, const mvx_mask_clip *clip, const ptrdiff_t clip_pitch[3],
                    const ptrdiff_t dst_pitch[3], mvx_mask **out, char *err);
/* the same checks in the same order with the same messages, except the format check: 8 to 16 bits, subsampling 0..1 on each axis, else
 * "Mask: input clip must be Gray or YUV (4:2:0, 4:2:2, 4:4:0, 4:4:4) of 8 to 16 bits, with constant dimensions."  The output has the
 * clip's depth (see "Deep masks" above); mvx_mask_info keeps its layout and describes the planes in samples. */
int mvx_mask_create_deep(const mvx_mask_args *args, const mvx_analysis_data *vectors, const mvx_mask_clip *clip, const ptrdiff_t clip_pitch[3],
                         const ptrdiff_t dst_pitch[3], mvx_mask **out, char *err);
/* bits per sample of the planes mvx_mask_frames writes: 8, or a deep object's clip depth (above 8: 16-bit containers) */
int mvx_mask_out_bits(const mvx_mask *m);
void mvx_mask_destroy(mvx_mask *m);
void mvx_mask_get_info(const mvx_mask *m, mvx_mask_info *info);

typedef struct mvx_mask_job {
    const void *blob;        /* vectors at n; NULL = unusable */
    const void *clip_luma;   /* luma plane of clip frame n; read by kind 5 only (a deep object above 8 bits: 16-bit samples) */
    void *dst[3];            /* 16-byte aligned */
} mvx_mask_job;

/* nframes jobs in one batch on `stream`: two or three small kernels over all jobs (usability, the block-resolution masks), then one
 * launch for the luma planes of all jobs and one for both chroma planes of all jobs */
int mvx_mask_frames(mvx_mask *m, int nframes, const mvx_mask_job *jobs, void *stream);

/* ---- mv.DepanCompensate / mv.DepanAnalyse ----------------------------------------------------------
 * global motion: DepanAnalyse fits a pan / zoom / rotation model to the block vectors of a delta-1 vector clip, DepanCompensate warps
 * a frame by the model summed over the frames between source and destination.  Neither needs FFTW (only DepanEstimate does).
 * mvx_depan_compensate_create replaces depanCompensateCreate, MVDepan.cpp:2750-2881; mvx_depan_compensate_map and
 * mvx_depan_motion_to_transform replace the frame selection and the transform sum of depanCompensateGetFrame, :2594-2675;
 * mvx_depan_compensate_frames replaces :2678-2715 with compensate_plane_nearest / _bilinear / _bicubic, :1626-2585.
 * mvx_depan_analyse_create replaces depanAnalyseCreate, :473-615; mvx_depan_analyse_frames / _host replace depanAnalyseGetFrame,
 * :237-430 (TrasformUpdate :145-199, RejectBadBlocks :203-234).  Creation touches no device.  Only the samples of each plane are written,
 * never the bytes between a plane's width and its pitch.
 * The estimator runs on the host (csrc/mvx_depan_host.h): each of its sums is a serial float chain in block order, and another order
 * gives another result.  The GPU gathers what it reads: the verdict of fgopIsUsable, the level-0 vectors and the mask bytes.
 * Deliberate divergences:
 *   1. the sign of a near-zero dx: where |dx| < 0.01 the reference draws the sign of 0.011 from rand() (:397-398); the library always
 *      returns +0.011f;
 *   2. (not rejected) reads and writes outside a row.  Wherever the reference's own index falls outside [0, row_size) of its row the
 *      library writes the plane's border value (0 for luma, half range for chroma), and it never writes outside the row:
 *        a. translation and zoom forms of all three interpolators, left mirror (srcp[w0 - rowleft] and the blur run that ends there):
 *           -rowleft >= row_size;
 *        b. the same forms, right mirror (srcp[w0 + 2 * row_size - rowleft - 2] and the blur run that starts there):
 *           rowleft > 2 * row_size - 2;
 *        c. the translation form of bilinear: its tail loop starts at rowgoodendpaired - 1 (:1971), so with fewer than two "good"
 *           columns (inttr0 >= row_size - 2, or inttr0 <= 1 - row_size) the reference reads before the row, writes dstp[-1], or runs its
 *           "bad" loop past either end of the row.  Every sample inside the row ends with the value of the per-sample rule -- interpolate
 *           where 0 <= rowleft < row_size - 1, else mirror (a, b), else border -- and that is what the library writes; nothing else;
 *   3. plane sizes: every plane must be at least 2 x 2 samples, rejected at creation otherwise.  With one column bicubic's edge test
 *      rowleft == row_size - 2 reads srcp[-1]; with one row its near-edge rows (hlow == 0) read the row below the plane and the zoom
 *      form's bottom row reads the row above it;
 *   4. a frame larger than 32767 x 32767 is rejected: a blur run is summed in int as in the reference, and stays exact up to there;
 *   5. (not rejected) positions that are NaN or not inside (-2^30, 2^30): the reference's float -> int conversion or its mirror
 *      arithmetic is undefined there.  The library writes the border value for such a sample (for the whole row where the row's ysrc
 *      is such a value in the translation and zoom forms), and faults on none;
 *   6. DepanAnalyse with a mask clip has no ignored border, and the reference's comparison of a vector with its eight neighbours
 *      (blockDx[n - 1 - nBlkX] .. blockDx[n + 1 + nBlkX], :211-221) then reads before and after its arrays.  The library skips that
 *      comparison for a block with a neighbour index outside the array.  (At the sides the indices wrap into the adjoining row, inside
 *      the array: those reads are kept as they are.);
 *   7. `info` overlays are the shell's business; the numbers they print are returned (mvx_depan_motion_to_transform's `motion`,
 *      mvx_depan_motion's iter and error). */

/* the format of a clip argument (VSVideoInfo) */
typedef struct mvx_depan_clip { int32_t width, height, bits, subsampling_w, subsampling_h, gray; } mvx_depan_clip;

typedef struct mvx_depan_compensate_args {
    double offset;           /* -10..10; a float argument in the reference.  Required */
    int32_t subpixel;        /* 0 nearest, 1 bilinear, 2 bicubic; MVX_UNSET -> 2 */
    double pixaspect;        /* > 0; pass 1.0 for the default (a float argument in the reference) */
    int32_t matchfields;     /* MVX_UNSET -> 1 */
    int32_t mirror;          /* bits: 1 top, 2 bottom, 4 left, 8 right; MVX_UNSET -> 0 */
    int32_t blur;            /* >= 0, MVX_UNSET -> 0; chroma planes of 4:2:0 and 4:2:2 take blur / 2 */
    int32_t fields;          /* MVX_UNSET -> 0 */
    int32_t tff;             /* MVX_UNSET = not passed */
} mvx_depan_compensate_args;

typedef struct mvx_depan_compensate_info {
    int32_t width, height, bits, subsampling_w, subsampling_h, num_planes;
    int32_t plane_width[3], plane_height[3];
    int32_t intoffset;       /* ceilf(offset) for offset > 0, else floorf(offset), :2835-2838; 0: every frame passes through */
    int32_t subpixel, mirror, pixel_max;
    int32_t border[3], blur[3];
    float xcenter, ycenter, offset, pixaspect;
} mvx_depan_compensate_info;

typedef struct mvx_depan_compensate mvx_depan_compensate;

/* num_frames / data_frames: the lengths of clip and data.  Pitches in bytes, multiples of the sample size */
int mvx_depan_compensate_create(const mvx_depan_compensate_args *args, const mvx_depan_clip *clip, int num_frames, int data_frames,
                                const ptrdiff_t src_pitch[3], const ptrdiff_t dst_pitch[3], mvx_depan_compensate **out, char *err);
/* DepanCompensate on a 32-bit float clip: the same arguments, checks and messages in the same order, but clip->bits must be 32 ("...: the
 * float path takes a 32-bit float clip; ..." where the format message sits; the format message itself remains for the subsampling) and the
 * pitches multiples of 4.  Touches no device.  The object is served by every mvx_depan_compensate_* function and
 * mvx_depan_motion_to_transform, which are host arithmetic and the same for it; mvx_depan_compensate_frames reads and writes planes of
 * float32.  info.bits is 32; info.pixel_max and info.border[] are 0: the border value is 0.0f for luma and 0.5f for chroma (the float
 * Flow's hole values), and nothing is clamped.
 * The float rule (csrc/mvx_depan_sample_float.h).  Where a sample comes from is the integer path's decision, value for
 * value: the form, the chain, rowleft / hlow, the 32nds of bilinear and the 256ths of bicubic, mirror bits, blur runs, edge rows and
 * columns, and divergences 2 and 5 above.  What is written there: a copy moves the sample's 32 bits (nearest, an unblurred mirror column,
 * bicubic's edge columns, the bottom-row copies: NaN payloads, denormals and -0.0f survive); a blur run is the float32 sum in index order
 * divided by its length; bilinear is ((32 - ky) * ((32 - kx) * a + kx * b) + ky * ((32 - kx) * c + kx * d)) * (1.0f / 1024) in all three
 * forms; bicubic is four row sums and their column sum over the integer table, divided once by the product of the two coefficient totals,
 * in all three forms (the translation form's sixteen truncated products are not restated); its near-edge rows are the reference's
 * expression in float32 and the zoom form's bottom row is (a + b) * 0.5f.  Nothing is fused.
 * The motion side has no float path and needs none: DepanAnalyse reads vectors, which come from the integer search on an 8..16 bit copy
 * of the clip as everywhere in the float family, and DepanEstimate is given the same copy (its entries refuse a float clip). */
int mvx_depan_compensate_create_float(const mvx_depan_compensate_args *args, const mvx_depan_clip *clip, int num_frames, int data_frames,
                                      const ptrdiff_t src_pitch[3], const ptrdiff_t dst_pitch[3], mvx_depan_compensate **out, char *err);
void mvx_depan_compensate_destroy(mvx_depan_compensate *h);
void mvx_depan_compensate_get_info(const mvx_depan_compensate *h, mvx_depan_compensate_info *info);
/* output frame ndest: returns 1 with *nsrc = ndest - intoffset, the clip frame to warp, and the motions of data frames *start + 1 ..
 * *end to sum; or 0 (intoffset == 0, or nsrc outside the clip): the caller returns clip frame ndest itself */
int mvx_depan_compensate_map(const mvx_depan_compensate *h, int ndest, int *nsrc, int *start, int *end);
/* the summed luma transform of output frame ndest from `count` motions (dx, dy, zoom, rot each: Depan_dx, Depan_dy, Depan_zoom, Depan_rot of
 * data frames start + 1 .. end, in that order): trsum = dxc, dxx, dxy, dyc, dyx, dyy; motion = dx, dy, zoom, rot of the info string
 * (transform2motion).  top_field: the _Field property of clip frame ndest, MVX_UNSET when absent; read with fields and matchfields only.
 * Host arithmetic, no device. */
int mvx_depan_motion_to_transform(const mvx_depan_compensate *h, int count, const float *motions, int ndest, int top_field,
                                  float trsum[6], float motion[4], char *err);

typedef struct mvx_depan_compensate_job {
    const void *src[3];      /* planes of clip frame nsrc */
    void *dst[3];
    float tr[6];             /* trsum; the library derives each plane's transform, border value and blur, :2683-2700 */
} mvx_depan_compensate_job;

/* nframes jobs in one batch on `stream`: a small pre-pass for the rotation form of nearest and bilinear, then one launch for all planes of
 * all jobs */
int mvx_depan_compensate_frames(mvx_depan_compensate *h, int nframes, const mvx_depan_compensate_job *jobs, void *stream);

typedef struct mvx_depan_analyse_args {
    int32_t zoom, rot;       /* MVX_UNSET -> 1 */
    double pixaspect, error, wrong, zerow; /* float arguments in the reference; pass 1.0 / 15.0 / 10.0 / 0.05 for the defaults */
    int64_t thscd1; int32_t thscd2;
    int32_t fields;          /* MVX_UNSET -> 0 */
} mvx_depan_analyse_args;

/* dx == 0.0f marks a frame without a result (scene change, unusable vectors, error too large), as in the reference */
typedef struct mvx_depan_motion { float dx, dy, zoom, rot; int32_t iter; float error; } mvx_depan_motion;

typedef struct mvx_depan_analyse mvx_depan_analyse;

/* mask: the format of the optional mask clip, NULL = none; *_frames: the lengths of the three clips */
int mvx_depan_analyse_create(const mvx_depan_analyse_args *args, const mvx_analysis_data *vectors, const mvx_depan_clip *clip,
                             const mvx_depan_clip *mask, int num_frames, int vector_frames, int mask_frames, mvx_depan_analyse **out, char *err);
void mvx_depan_analyse_destroy(mvx_depan_analyse *h);
/* n frames: blobs[i] the DEVICE blob of the vector clip at frame i (backward vectors: at max(0, i - 1)), NULL = unusable; masks[i] the
 * DEVICE luma plane of the mask clip (with a mask clip only); top_field[i] read with fields only (may be NULL otherwise).  One gather
 * kernel for all frames, then the estimator on the host.  Synchronous. */
int mvx_depan_analyse_frames(mvx_depan_analyse *h, int n, const void *const *blobs, const void *const *masks, ptrdiff_t mask_pitch,
                             const int32_t *top_field, mvx_depan_motion *out, void *stream);
/* the same from HOST blobs and HOST mask planes; touches no device */
int mvx_depan_analyse_host(const mvx_depan_analyse *h, int n, const void *const *blobs, const void *const *masks, ptrdiff_t mask_pitch,
                           const int32_t *top_field, mvx_depan_motion *out);

/* ---- mv.DepanEstimate -------------------------------------------------------------------------------
 * global motion without a vector clip: pan (and zoom, from two windows) between frame n - 1 and frame n from the peak of the
 * cross-correlation of a luma window, computed with a power-of-two real 2-D FFT in HIP (csrc/mvx_depan_fft.hip; no FFTW).  The three
 * entry points mirror the reference's three chained filters: mvx_depan_estimate_spectra replaces depanEstimateStage1GetFrame,
 * MVDepan.cpp:956-997 (frame_data2d :651-678 and the r2c transform); mvx_depan_estimate_correlate replaces depanEstimateStage2GetFrame,
 * :1000-1151 (mult_conj_data2d :681-697, the c2r transform, get_motion_vector :700-883, the zoom of :1110-1121, the frame-0 rule);
 * mvx_depan_estimate_finish replaces depanEstimateStage3GetFrame, :1154-1243.  mvx_depan_estimate_create replaces
 * depanEstimateCreate, :1271-1433, and touches no device.
 * The transforms cannot be byte-exact against FFTW, whose order of summation is its own: the spectrum is held to the error bound of a
 * single-precision radix FFT against a double-precision one, the discrete results (peak position, scene-change decision, zoom branch) are
 * exact on cases whose margins exceed that error, and dx, dy, zoom and trust are held to a measured multiple of the distance between two
 * independent FFTs.  Everything after the scan of the correlation surface is host arithmetic in the reference's order
 * (csrc/mvx_depan_estimate_host.h), bit-exact given the same scan results; the sum behind the mean of the search area is the reference's float
 * chain in scan order, on the device.  No float atomics: results are identical from run to run and
 * for any batch size.
 * Deliberate divergences, continuing the list above:
 *   8. samples are read in the clip's own type.  The reference passes bytesPerSample (1, 2, 4) to frame_data2d, which compares it with 8
 *      and 32 (:657-668), so every clip goes through its uint16_t branch: right for 9..16 bits, but an 8-bit clip is read as pairs of
 *      bytes over 2 * winx bytes per row, past the window and on the last rows past the frame.  The library reads bytes for 8 bits and
 *      words for 9..16 bits;
 *   9. float clips are refused at creation.  Of the Depan family only the two warps have float entries (mvx_depan_compensate_create_float,
 *      mvx_depan_stabilise_create_float): a float pipeline estimates on the 8..16 bit copy its search reads -- the transform here is
 *      single precision anyway -- and warps the float clip by the result;
 *  10. winx (after the halving for zoom) and winy must be powers of two from 8 to 8192, refused at creation otherwise; the automatic
 *      sizes always qualify on a frame of at least 8 x 8 (16 x 8 with zoom).  A window that leaves the frame -- the second window of
 *      zoommax != 1 starts at wleft + width / 2, which the reference does not check -- is refused too;
 *  11. a result with |dx| < 0.01 becomes +0.011f where the reference draws the sign from rand() (:878-879), as in divergence 1;
 *  12. the `info` overlay is not built; the numbers of `info` are returned.  `show` is mvx_depan_estimate_correlate_show;
 *  13. show on a surface whose maximum equals its minimum: the reference multiplies 0 by pixel_max / 0 and converts the NaN to int
 *      (showcorrelation, :920, :937), which is undefined; the library paints 0 over the whole window. */

typedef struct mvx_depan_estimate_args {
    double trust;            /* 0..100; float arguments in the reference: pass 4.0 / 1.0 / 1.0 / 1.0 for the defaults of trust, zoommax, stab, pixaspect */
    double zoommax, stab, pixaspect;
    int32_t winx, winy;      /* MVX_UNSET or 0 -> the largest power of two that fits, up to 8192 */
    int32_t wleft, wtop;     /* MVX_UNSET or < 0 -> centred */
    int32_t dxmax, dymax;    /* MVX_UNSET or < 0 -> winx / 4, winy / 4 */
    int32_t fields;          /* MVX_UNSET -> 0 */
    int32_t tff;             /* MVX_UNSET = not passed */
    int32_t float_samples;   /* 1: the clip's sample type is float (refused after the reference's own checks) */
} mvx_depan_estimate_args;

typedef struct mvx_depan_estimate_info {
    int32_t winx, winy, wleft, wtop, dxmax, dymax;
    int32_t windows;         /* 1, or 2 with zoommax != 1 */
    int64_t spectrum_bytes;  /* of one window: winy * (winx / 2 + 1) complex floats, the reference's padded layout */
} mvx_depan_estimate_info;

/* Depan_dx, Depan_dy, Depan_zoom of stage 2 and its trust; dx == 0.0f marks a scene change */
typedef struct mvx_depan_estimate_result { float dx, dy, zoom, trust; } mvx_depan_estimate_result;

/* what the scan of one correlation surface leaves (get_motion_vector :717-767): the first maximum in scan order and the sum over the four
 * corners, both unnormalised, the position of the maximum, and the surface at (imax + 1, jmax), (imax - 1, jmax), (imax, jmax + 1),
 * (imax, jmax - 1), wrapped */
typedef struct mvx_depan_estimate_scan { float max, sum; int32_t imax, jmax; float xp, xm, yp, ym; } mvx_depan_estimate_scan;

typedef struct mvx_depan_estimate mvx_depan_estimate;

int mvx_depan_estimate_create(const mvx_depan_estimate_args *args, const mvx_depan_clip *clip, int num_frames, mvx_depan_estimate **out, char *err);
void mvx_depan_estimate_destroy(mvx_depan_estimate *h);
void mvx_depan_estimate_get_info(const mvx_depan_estimate *h, mvx_depan_estimate_info *info);
/* stage 1: luma_planes[i] the DEVICE luma plane of frame i (pitch in bytes), spectra_out[i] DEVICE room for windows * spectrum_bytes
 * (8-byte aligned; the second window's spectrum follows the first).  Two launches for all frames; asynchronous on `stream`. */
int mvx_depan_estimate_spectra(mvx_depan_estimate *h, int nframes, const void *const *luma_planes, ptrdiff_t pitch, void *const *spectra_out, void *stream);
/* stage 2: pair i is frame frame_numbers[i] (cur) against the frame before it (prev), both as written by stage 1.  top_field[i]: the
 * _Field property of cur, MVX_UNSET when absent; read with fields only (NULL: absent everywhere).  frame_numbers NULL: no pair is
 * frame 0.  scans_out: NULL, or room for npairs * windows scan results.  Three launches for all pairs, then the host tail.  Synchronous. */
int mvx_depan_estimate_correlate(mvx_depan_estimate *h, int npairs, const void *const *prev_spectra, const void *const *cur_spectra,
                                 const int32_t *top_field, const int32_t *frame_numbers, mvx_depan_estimate_result *out,
                                 mvx_depan_estimate_scan *scans_out, void *stream);
/* stage 2 with `show` (showcorrelation, :895-953, as called at :1072-1077 and :1123-1124): the same arguments, results and scan results, bit for
 * bit, and show_planes[i], a DEVICE luma plane of pair i in the clip's sample type (a copy of frame cur, the caller's; show_pitch in bytes), gets
 * the correlation surface painted into its window rectangle(s): (int)((c - min) * (pixel_max / (max - min))) at (wleft + i, wtop + j), the
 * second window of zoommax != 1 at wleft + width / 2.  Nothing else of the plane is touched.  Frame 0 is painted like any other pair.  The scan
 * reads the kept rows as above; every row of the surface is computed a second time for the paint (four more launches).  Synchronous. */
int mvx_depan_estimate_correlate_show(mvx_depan_estimate *h, int npairs, const void *const *prev_spectra, const void *const *cur_spectra,
                                      const int32_t *top_field, const int32_t *frame_numbers, mvx_depan_estimate_result *out,
                                      mvx_depan_estimate_scan *scans_out, void *const *show_planes, ptrdiff_t show_pitch, void *stream);
/* the host tail alone, from npairs * windows scan results of the caller; touches no device */
int mvx_depan_estimate_host_tail(const mvx_depan_estimate *h, int npairs, const mvx_depan_estimate_scan *scans, const int32_t *top_field,
                                 const int32_t *frame_numbers, mvx_depan_estimate_result *out);
/* stage 3 for frame n: results of frames max(0, n - 1), n, min(n + 1, num_frames - 1) -> Depan_dx, Depan_dy, Depan_zoom, Depan_rot = 0
 * (iter and error are 0).  Host arithmetic. */
int mvx_depan_estimate_finish(const mvx_depan_estimate *h, int n, const mvx_depan_estimate_result results_prev_cur_next[3], mvx_depan_motion *motion);

/* ---- mv.DepanStabilise ------------------------------------------------------------------------------
 * smooths the global motion of a clip (the Depan_* values of DepanAnalyse or DepanEstimate) and warps every frame by the difference
 * between its smoothed and its own cumulative motion; the border that opens can be filled from a previous and a following frame.
 * mvx_depan_stabilise_create replaces depanStabiliseCreate, MVDepan.cpp:3909-4163, and touches no device; mvx_depan_stabilise_window
 * gives the request sets of :3571-3591 (method 0) and :3720-3763 (method 1); mvx_depan_stabilise_plan replaces the host part of
 * depanStabiliseGetFrame0 / 1, :3567-3666 / :3717-3841 (Inertial :2945-3115, Average :3118-3246, InertialLimit :3249-3329) and the
 * source selection of fillBorderPrev :3398-3419 and fillBorderNext :3461-3502 (csrc/mvx_depan_stab_host.h: float arithmetic in the
 * reference's order); mvx_depan_stabilise_frames replaces the up to three painting passes of :3679-3693 (fillBorderPrev, fillBorderNext,
 * compensateFrame, :3356-3546) with one kernel that selects per sample and stores once (csrc/mvx_depan_sample.h: ds_sample on top of
 * DepanCompensate's interpolators).  Only the samples of each plane are written.
 * Per sample the result is: the current frame where its position is inside it; else the next source where that is inside; else what the
 * first pass wrote, with its mirror, blur or border value.  With prev = next = 0 it is DepanCompensate's pass with the plan's transform.
 * What the reference does and the library keeps, surprising as it is:
 *   a. fillBorderPrev always reads clip frame nprev = max(nbase, ndest - prev), with the transform summed over nprev + 1 .. ndest: the
 *      assignment of :3412 is unconditional, its "most centred and nearest" test selects nothing;
 *   b. fillBorderNext chooses its frame (the most centred and nearest, :3494-3497) but warps it by the transform accumulated over every
 *      frame its walk passed, also where it chose an earlier one; a bad frame (dx == 0.0f) ends the walk at the frame before it, which
 *      may be ndest itself;
 *   c. data frame 0 is never read: its motion is dx = dy = rot = 0, zoom = 1 from creation (:4075-4078), so frame 0 always counts as bad;
 *   d. method 1 with fps < 4 * cutoff has radius 0 and Average divides 0 by 0: the transform is NaN, and by divergence 5 of
 *      DepanCompensate every sample of the current frame's pass takes that pass's border value;
 *   e. sqrt / fabs of InertialLimit and of the selections are the float overloads (the reference is C++ and includes <math.h>).
 * The divergences of DepanCompensate hold for each pass (2 to 5 above).  Deliberate divergences of its own:
 *   1. chroma of the fill passes.  fillBorderPrev and fillBorderNext assign only tr[0] (:3405-3406, :3467-3468) and warp the chroma planes
 *      by tr[1] and tr[2], which are indeterminate (for 4:4:4 nothing is ever assigned to them).  The library derives the chroma
 *      transform of each fill pass from that pass's own luma transform, by the rule of compensateFrame (:3366-3379).  Chroma samples that
 *      come from a fill source therefore have no counterpart in the reference;
 *   2. `info`: the overlay is the shell's business; mvx_depan_stabilise_plan returns its four numbers and the BASE! flag;
 *   3. creation rejects what the reference leaves undefined: a clip without frames, a negative frame rate, fps / (4 * cutoff) not below
 *      1048576 (its (int) conversion and the window tables), a negative or NaN tzoom (winrzsize < 0 writes before winrz, :4155);
 *   4. (int)(ndest - 10 * fps / cutoff) of method 0 (:3567) is undefined below -2^31; the library takes 0 there as for every
 *      negative value; fitlast + ndest + 1 (:3654) is summed in 64 bits;
 *   5. method 1 with next > radius: fillBorderNext reads data frames up to ndest + next which the reference never requested (the loop
 *      of :3757 is empty); mvx_depan_stabilise_window includes them;
 *   6. NaN coefficients.  IEEE 754 leaves the sign and payload of a NaN result open, and a compiler may commute the operands of an addition
 *      or a product, so which NaN the reference's arithmetic ends on depends on its build.  Where a coefficient of a plan is NaN it is
 *      the positive quiet NaN (0x7FC00000).  Whether a coefficient is NaN is the arithmetic's own outcome, and no finite value depends
 *      on a NaN's bits. */

typedef struct mvx_depan_stabilise_args {
    /* float arguments of the reference, passed as doubles and rounded to float; (double)MVX_UNSET -> the default */
    double cutoff;           /* > 0; -> 1.0 */
    double damping;          /* -> 0.9 */
    double initzoom;         /* -> 1.0 */
    double dxmax, dymax;     /* -> 60 / 30; negative: reset to the base instead of the soft limit */
    double zoommax, rotmax;  /* -> 1.05 / 1.0 */
    double pixaspect;        /* > 0; -> 1.0 */
    double tzoom;            /* >= 0; -> 3.0 */
    int32_t addzoom;         /* MVX_UNSET -> 0 */
    int32_t prev, next;      /* >= 0; MVX_UNSET -> 0 */
    int32_t mirror;          /* bits: 1 top, 2 bottom, 4 left, 8 right; MVX_UNSET -> 0 */
    int32_t blur;            /* >= 0, MVX_UNSET -> 0; chroma planes of 4:2:0 and 4:2:2 take blur / 2 */
    int32_t subpixel;        /* 0 nearest, 1 bilinear, 2 bicubic; MVX_UNSET -> 2 */
    int32_t fitlast;         /* MVX_UNSET -> 0 */
    int32_t method;          /* 0 inertial, 1 average; MVX_UNSET -> 0 */
    int32_t fields;          /* MVX_UNSET -> 0 */
} mvx_depan_stabilise_args;

typedef struct mvx_depan_stabilise_info {
    int32_t width, height, bits, subsampling_w, subsampling_h, num_planes;
    int32_t plane_width[3], plane_height[3];
    int32_t subpixel, mirror, pixel_max, method, prev, next, nfields;
    int32_t radius;          /* (int)(fps / (4 * cutoff)), :4140 */
    int32_t wint_size, winrz_size, winfz_size; /* each table has radius + 1 entries; the sizes say where its zeros begin */
    int32_t border[3], blur[3];
    float fps, freqnative, initzoom /* 1 / the argument */, zoommax /* after :4061 */, xcenter, ycenter;
    float nonlinfactor[6];   /* dxc dxx dxy dyc dyx dyy, :4112-4135 */
} mvx_depan_stabilise_info;

typedef struct mvx_depan_stabilise_source {
    int32_t used;            /* 0: the filter has no such pass */
    int32_t frame;           /* the clip frame to read */
    float tr[6];             /* its luma transform: dxc dxx dxy dyc dyx dyy */
} mvx_depan_stabilise_source;

typedef struct mvx_depan_stabilise_frame_plan {
    float tr[6];             /* the luma transform of clip frame n */
    int32_t nbase;           /* the base after the scan for bad frames, the symmetric cut of method 1 and InertialLimit */
    int32_t base;            /* nbase == n: "BASE!" in the info string */
    float motion[4];         /* dx, dy, zoom, rot of the info string (transform2motion of tr, :3700) */
    mvx_depan_stabilise_source prev, next;
} mvx_depan_stabilise_frame_plan;

typedef struct mvx_depan_stabilise mvx_depan_stabilise;

/* num_frames / data_frames: the lengths of clip and data; fps_num / fps_den: the clip's frame rate.  The reference's error texts come
 * first, in its order; then the library's own.  Pitches in bytes, multiples of the sample size */
int mvx_depan_stabilise_create(const mvx_depan_stabilise_args *args, const mvx_depan_clip *clip, int num_frames, int data_frames,
                               int64_t fps_num, int64_t fps_den, const ptrdiff_t src_pitch[3], const ptrdiff_t dst_pitch[3],
                               mvx_depan_stabilise **out, char *err);
/* DepanStabilise on a 32-bit float clip, as mvx_depan_compensate_create_float: the same arguments, checks and messages in the same order,
 * clip->bits must be 32, pitches multiples of 4, no device touched; window, plan, get_info and get_windows serve the object unchanged and
 * mvx_depan_stabilise_frames paints planes of float32 by the float rule.  info.bits is 32, info.pixel_max and info.border[] are 0 (the
 * border value is 0.0f luma, 0.5f chroma).  A float sample may be negative, so the selection carries a painted flag per pass where the
 * integer path reads "negative" as "not painted": a negative sample of the current frame is never overpainted by a fill source. */
int mvx_depan_stabilise_create_float(const mvx_depan_stabilise_args *args, const mvx_depan_clip *clip, int num_frames, int data_frames,
                                     int64_t fps_num, int64_t fps_den, const ptrdiff_t src_pitch[3], const ptrdiff_t dst_pitch[3],
                                     mvx_depan_stabilise **out, char *err);
void mvx_depan_stabilise_destroy(mvx_depan_stabilise *h);
void mvx_depan_stabilise_get_info(const mvx_depan_stabilise *h, mvx_depan_stabilise_info *info);
/* the cosine windows of :4140-4160, radius + 1 floats each (any may be NULL) */
void mvx_depan_stabilise_get_windows(const mvx_depan_stabilise *h, float *wint, float *winrz, float *winfz);
/* output frame n: the data frames *data_first .. *data_last whose motion mvx_depan_stabilise_plan reads, and the clip frames
 * *clip_first .. *clip_last among which its sources lie (n is one of them) */
int mvx_depan_stabilise_window(const mvx_depan_stabilise *h, int n, int *data_first, int *data_last, int *clip_first, int *clip_last);
/* motions: dx, dy, zoom, rot (Depan_dx, Depan_dy, Depan_zoom, Depan_rot) per data frame of the window, data_first first; dx == 0.0f marks
 * a bad frame.  Host arithmetic, no device. */
int mvx_depan_stabilise_plan(const mvx_depan_stabilise *h, int n, const float *motions, mvx_depan_stabilise_frame_plan *plan, char *err);

typedef struct mvx_depan_stabilise_job {
    mvx_depan_stabilise_frame_plan plan;
    const void *cur[3];      /* planes of clip frame n */
    const void *prev[3];     /* planes of clip frame plan.prev.frame; read only where plan.prev.used */
    const void *next[3];     /* planes of clip frame plan.next.frame; read only where plan.next.used */
    void *dst[3];
} mvx_depan_stabilise_job;

/* nframes jobs in one batch on `stream`: a small pre-pass for the sources whose rotation form walks its rows (every fill source, and the
 * current frame with nearest and bilinear), then one launch for all planes of all jobs.  All sources share src_pitch. */
int mvx_depan_stabilise_frames(mvx_depan_stabilise *h, int nframes, const mvx_depan_stabilise_job *jobs, void *stream);

/* ---- mv.SCDetection -------------------------------------------------------------------------------
 * replaces the decision of mvscdetectionGetFrame, MVSCDetection.c:43-73 (arg string :137-145): scene_change[i] (HOST array) =
 * !usable(blobs[i]) for n device blobs of one vector clip, i.e. the value of _SceneChangePrev (forward vectors) or
 * _SceneChangeNext (backward vectors); thscd1 / thscd2 as passed by the user (MVX_UNSET -> 400 / 130). Synchronous. */
int mvx_scdetect(const mvx_analysis_data *vectors_data, int64_t thscd1, int32_t thscd2, int n, const void *const *blobs,
                 int32_t *scene_change, void *stream, char *err);

/* ---- vector blob helpers (reader side: Fakery.c, MVAnalysisData.c:7-31) -------------------------- */
void mvx_scale_thscd(int64_t *thscd1, int32_t *thscd2, const mvx_analysis_data *ad);
/* bytes of the MVTools_vectors property of a vector clip with this analysis data (Fakery.c:110-121 level geometry,
 * GroupOfPlanes.c:127-148 array layout) */
int mvx_vectors_size(const mvx_analysis_data *ad);

/* ---- test hook: selects among kernel variants that compute identical results, so that the parity suite can run its cases
 * through each of them.  Options: "general" = 1 keeps the default search out of its lean and speculative kernels; "cpw1" = 1
 * runs the general kernels one chain per workgroup; "spec" picks the default search's kernel (0 the lean serial one, 1 the
 * library's choice, 2 speculative with every block live, 3 speculative without runs, 5 speculative wherever it can run);
 * "team" = waves per chain of the speculative kernel's team form (0 never, 2..8 always, -1 the library's choice);
 * "scratch_poison" = 0 off, 1..255 the byte every fresh allocation of handle-owned device scratch is filled with (headroom included).  The
 * library never reads the environment; a production host never needs this call. */
int mvx_debug_option(const char *name, int value);
/* the last search launch of this process: out[0] = chains per SIMD of the default-search kernel (0: the general kernel ran), out[1] = chains
 * per workgroup (team form: waves per chain), out[2] = barrier interval in blocks, out[3] = job-table entries, out[4] = which default-search kernel:
 * 0 the serial lean kernel (or the general one), 2 the speculative kernel with one wave per chain, 3 its team form (the waves of a workgroup walk one
 * chain; the library's choice for launches that leave wave slots empty).  Tests use it to assert which build a batch took. */
void mvx_debug_last_launch(int out[5]);
/* test hook: the search's own table of level `level` (0 = finest) of a created mv.Analyse, no device involved.  out[0..10] = nBlkX, nBlkY, pel,
 * padded width, padded height, hpad, vpad and the chroma plane's padded width, padded height, hpad, vpad; out[11..13] = byte offset of the level's
 * first sub-pel plane inside super plane 0 / 1 / 2; out[14..16] = byte distance between its sub-pel planes; out[17..19] = the row pitches;
 * out[20..22] = the shadow strides set by mvx_analyse_set_ref_shadow (the 8-bit layout has none for luma); out[23] = which search takes the
 * default launch: 2 the lean / speculative kernels can, 1 the specialised general kernels, 0 the generic kernel (64-bit addresses).  Returns
 * the number of levels, or MVX_E_ARG.  tests/test_search_addressing.py audits the kernels' 32-bit reference offsets against it. */
int mvx_analyse_debug_level(const mvx_analyse *a, int level, int64_t out[24]);
/* test hook of the dct 1..4 modes: the device transform and quantiser alone.  `a` was created with dct 1..4; `plane` is a device luma plane, block i
 * starts at sample xs[i] of row ys[i] (HOST arrays; the caller keeps the blocks inside the plane); out_bytes (device) receives blksize * blksizev
 * quantised coefficients per block, row-major, in the sample type.  Synchronises the stream. */
int mvx_analyse_dct_blocks(mvx_analyse *a, const void *plane, ptrdiff_t pitch, int n, const int32_t *xs, const int32_t *ys, void *out_bytes, void *stream);

/* ---- small device-memory helpers so that a C host (e.g. the VapourSynth shell) needs no HIP headers */
void *mvx_dev_alloc(size_t bytes);            /* zero-filled */
void *mvx_dev_alloc_uninit(size_t bytes);     /* contents undefined (scratch, upload targets) */
void mvx_dev_free(void *p);                   /* goes to a size-keyed free list (no device synchronisation); wait for the work that uses p first */
void mvx_dev_pool_limit(size_t bytes);        /* bytes the free list may hold (default 24 GiB) */
void mvx_dev_pool_trim(void);                 /* returns the whole free list to the driver */
int mvx_dev_mem_info(size_t *free_bytes, size_t *total_bytes); /* of the current device; the free list counts as free */
void *mvx_stream_create(void);                /* a non-blocking stream for the `stream` arguments; NULL on failure */
void *mvx_stream_create_priority(int level);  /* < 0 lowest, 0 default, > 0 highest priority; different priorities never share a hardware queue */
void mvx_stream_destroy(void *stream);
int mvx_copy_to_device(void *dst, ptrdiff_t dst_pitch, const void *src_host, ptrdiff_t src_pitch, size_t row_bytes, size_t rows, void *stream);
int mvx_copy_to_host(void *dst_host, ptrdiff_t dst_pitch, const void *src, ptrdiff_t src_pitch, size_t row_bytes, size_t rows, void *stream);
int mvx_stream_sync(void *stream);
void *mvx_host_alloc_pinned(size_t bytes);    /* page-locked host memory for asynchronous mvx_copy_to_host targets; NULL on failure */
void mvx_host_free_pinned(void *p);
/* Synchronous 2-D transfers for hosts whose frames live in ordinary (pageable) memory: staged through a small set of pinned buffers
 * inside the library (a linear PCIe copy + a row-by-row memcpy on the calling thread) -- several times faster than the pageable 2-D
 * copies above for large planes, and safe to call from many threads.  Complete on return; work already enqueued on `stream` runs
 * before the copy. */
int mvx_upload_2d(void *dst, ptrdiff_t dst_pitch, const void *src_host, ptrdiff_t src_pitch, size_t row_bytes, size_t rows, void *stream);
int mvx_download_2d(void *dst_host, ptrdiff_t dst_pitch, const void *src, ptrdiff_t src_pitch, size_t row_bytes, size_t rows, void *stream);
int mvx_dev_memset(void *dst, int value, size_t bytes, void *stream); /* asynchronous on `stream` */
int mvx_set_device(int ordinal);
/* Start-up work a host can take off its first frame (r6; the VapourSynth shell calls it from a background thread when the plugin is loaded): brings the HIP runtime up on the
 * current device, loads this library's code objects (a first kernel launch pays ~0.1 s for that) and page-locks `staging_buffers` of the 16 MiB buffers mvx_upload_2d /
 * mvx_download_2d go through (`staging_buffers` < 0: the runtime only) (page-locking is slow -- ~20 ms per buffer -- and stalls every other HIP call of the process while it lasts).  Idempotent, thread-safe; MVX_OK,
 * or MVX_E_DEVICE when there is no usable device (nothing else fails because of it). */
int mvx_warmup(int staging_buffers);

#ifdef __cplusplus
}
#endif
#endif /* MVTOOLS_AMD_H */
