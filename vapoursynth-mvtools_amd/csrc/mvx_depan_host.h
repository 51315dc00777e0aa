// mvx_depan_host.h -- the host arithmetic of the Depan filters, without HIP so that a stand-alone program can include it: the transform
// algebra (MVDepan.cpp:63-142 setNull / transform2motion / inversetransform, :1554-1615 motion2transform / sumtransform), DepanCompensate's
// summed transform (:2616-2675) and DepanAnalyse's estimator (:145-234 TrasformUpdate / RejectBadBlocks, :279-399 the iteration).
// Every expression is the reference's, in its order, in float: build with -ffp-contract=off.  The transcendental functions are the C
// library's float functions, as in the reference.  Every accumulator of the estimator is a serial float chain over the blocks in block
// order; reordering the sums changes the result, so the estimator is host code on purpose and not a GPU reduction.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#define DEPAN_MOTIONBAD 0.0f

struct DepanTransform { float dxc, dxx, dxy, dyc, dyx, dyy; };

static inline void depan_set_null(DepanTransform *tr) { tr->dxc = 0.0f; tr->dxx = 1.0f; tr->dxy = 0.0f; tr->dyc = 0.0f; tr->dyx = 0.0f; tr->dyy = 1.0f; }

// MVDepan.cpp:88-122
static inline void depan_transform2motion(const DepanTransform *tr, int forward, float xcenter, float ycenter, float pixaspect, float *dx, float *dy, float *rot, float *zoom) {
    const float PI = 3.1415926535897932384626433832795f;
    float rotradian, sinus, cosinus;
    rotradian = -atanf(pixaspect * tr->dxy / tr->dxx);
    *rot = rotradian * 180 / PI;
    sinus = sinf(rotradian);
    cosinus = cosf(rotradian);
    *zoom = tr->dxx / cosinus;
    if (forward) {
        *dx = tr->dxc - xcenter - (-xcenter * cosinus + ycenter / pixaspect * sinus) * (*zoom);
        *dy = tr->dyc / pixaspect - ycenter / pixaspect - ((-ycenter) / pixaspect * cosinus + (-xcenter) * sinus) * (*zoom);
    } else {
        *dx = tr->dxc / (*zoom) * cosinus + tr->dyc / (*zoom) / pixaspect * sinus - xcenter / (*zoom) * cosinus + xcenter - ycenter / (*zoom) / pixaspect * sinus;
        *dy = -tr->dxc / (*zoom) * sinus + tr->dyc / (*zoom) / pixaspect * cosinus + xcenter / (*zoom) * sinus - (-ycenter / pixaspect) - ycenter / (*zoom) / pixaspect * cosinus;
    }
}

// MVDepan.cpp:128-142
static inline void depan_inversetransform(const DepanTransform *ta, DepanTransform *tinv) {
    float pixaspect;
    if (ta->dxy != 0.0f)
        pixaspect = sqrtf(-ta->dyx / ta->dxy);
    else
        pixaspect = 1.0f;
    tinv->dxx = ta->dxx / ((ta->dxx) * ta->dxx + ta->dxy * ta->dxy * pixaspect * pixaspect);
    tinv->dyy = tinv->dxx;
    tinv->dxy = -tinv->dxx * ta->dxy / ta->dxx;
    tinv->dyx = -tinv->dxy * pixaspect * pixaspect;
    tinv->dxc = -tinv->dxx * ta->dxc - tinv->dxy * ta->dyc;
    tinv->dyc = -tinv->dyx * ta->dxc - tinv->dyy * ta->dyc;
}

// MVDepan.cpp:1554-1591
static inline void depan_motion2transform(float dx1, float dy1, float rot, float zoom1, float pixaspect, float xcenter, float ycenter, int forward, float fractoffset, DepanTransform *tr) {
    const float PI = 3.1415926535897932384626433832795f;
    float rotradian, sinus, cosinus, dx, dy, zoom;
    dx = fractoffset * dx1;
    dy = fractoffset * dy1;
    rotradian = fractoffset * rot * PI / 180;
    if (fabsf(rotradian) < 1e-6f)
        rotradian = 0.0f;
    zoom = expf(fractoffset * logf(zoom1));
    if (fabsf(zoom - 1.0f) < 1e-6f)
        zoom = 1.0f;
    sinus = sinf(rotradian);
    cosinus = cosf(rotradian);
    if (forward) {
        tr->dxc = xcenter + (-xcenter * cosinus + ycenter / pixaspect * sinus) * zoom + dx;
        tr->dxx = cosinus * zoom;
        tr->dxy = -sinus / pixaspect * zoom;
        tr->dyc = ycenter + (((-ycenter) / pixaspect * cosinus + (-xcenter) * sinus) * zoom + dy) * pixaspect;
        tr->dyx = sinus * zoom * pixaspect;
        tr->dyy = cosinus * zoom;
    } else {
        tr->dxc = xcenter + ((-xcenter + dx) * cosinus - ((-ycenter) / pixaspect + dy) * sinus) * zoom;
        tr->dxx = cosinus * zoom;
        tr->dxy = -sinus / pixaspect * zoom;
        tr->dyc = ycenter + (((-ycenter) / pixaspect + dy) * cosinus + (-xcenter + dx) * sinus) * zoom * pixaspect;
        tr->dyx = sinus * zoom * pixaspect;
        tr->dyy = cosinus * zoom;
    }
}

// MVDepan.cpp:1599-1615
static inline void depan_sumtransform(const DepanTransform *ta, const DepanTransform *tb, DepanTransform *tba) {
    DepanTransform temp;
    temp.dxc = tb->dxc + tb->dxx * ta->dxc + tb->dxy * ta->dyc;
    temp.dxx = tb->dxx * ta->dxx + tb->dxy * ta->dyx;
    temp.dxy = tb->dxx * ta->dxy + tb->dxy * ta->dyy;
    temp.dyc = tb->dyc + tb->dyx * ta->dxc + tb->dyy * ta->dyc;
    temp.dyx = tb->dyx * ta->dxx + tb->dyy * ta->dyx;
    temp.dyy = tb->dyx * ta->dxy + tb->dyy * ta->dyy;
    memcpy(tba, &temp, sizeof(temp));
}

// MVDepan.cpp:2616-2675: the summed luma transform of one output frame of DepanCompensate.  motions: count x (dx, dy, zoom, rot) of the
// data frames start + 1 .. end; halfline: 0, or with fields and matchfields -0.5f for a top field and +0.5f for a bottom field.
static inline void depan_compensate_transform(const float *motions, int count, float offset, int intoffset, int fields, float pixaspect, float xcenter, float ycenter,
                                              float halfline, DepanTransform *trsum, float motion[4]) {
    const int forward = intoffset > 0;
    float fractoffset = offset;
    fractoffset += forward ? 1 : -1;
    fractoffset -= intoffset;
    const int nfields = fields ? 2 : 1;
    depan_set_null(trsum);
    for (int k = 0; k < count; k++) {
        const float *m = motions + 4 * k;
        if (m[0] == DEPAN_MOTIONBAD) { depan_set_null(trsum); break; }
        DepanTransform tr;
        depan_motion2transform(m[0], m[1], m[3], m[2], pixaspect / nfields, xcenter, ycenter, forward, fractoffset, &tr);
        depan_sumtransform(trsum, &tr, trsum);
    }
    if (halfline != 0.0f) trsum->dyc += halfline;
    motion[0] = 0.0f; motion[1] = 0.0f; motion[3] = 0.0f; motion[2] = 1.0f; // dx, dy, zoom, rot
    depan_transform2motion(trsum, forward, xcenter, ycenter, pixaspect / nfields, &motion[0], &motion[1], &motion[3], &motion[2]);
}

// MVDepan.cpp:145-199
static inline void depan_transform_update(DepanTransform *tr, const float *blockDx, const float *blockDy, const int *blockX, const int *blockY, const float *blockWeight,
                                          int nBlkX, int nBlkY, float safety, int ifZoom1, int ifRot1, float *error1, float pixaspect) {
    DepanTransform trderiv;
    int n = nBlkX * nBlkY;
    trderiv.dxc = 0; trderiv.dxx = 0; trderiv.dxy = 0; trderiv.dyc = 0; trderiv.dyx = 0; trderiv.dyy = 0;
    float norm = 0.1f;
    float x2 = 0.1f;
    float y2 = 0.1f;
    float error2 = 0.1f;
    for (int i = 0; i < n; i++) {
        float bw = blockWeight[i];
        float xdif = (tr->dxc + tr->dxx * blockX[i] + tr->dxy * blockY[i] - blockX[i] - blockDx[i]);
        trderiv.dxc += 2 * xdif * bw;
        if (ifZoom1)
            trderiv.dxx += 2 * blockX[i] * xdif * bw;
        if (ifRot1)
            trderiv.dxy += 2 * blockY[i] * xdif * bw;
        float ydif = (tr->dyc + tr->dyx * blockX[i] + tr->dyy * blockY[i] - blockY[i] - blockDy[i]);
        trderiv.dyc += 2 * ydif * bw;
        if (ifRot1)
            trderiv.dyx += 2 * blockX[i] * ydif * bw;
        if (ifZoom1)
            trderiv.dyy += 2 * blockY[i] * ydif * bw;
        norm += bw;
        x2 += blockX[i] * blockX[i] * bw;
        y2 += blockY[i] * blockY[i] * bw;
        error2 += (xdif * xdif + ydif * ydif) * bw;
    }
    trderiv.dxc /= norm * 2;
    trderiv.dxx /= x2 * 2 * 1.5f;
    trderiv.dxy /= y2 * 2 * 3;
    trderiv.dyc /= norm * 2;
    trderiv.dyx /= x2 * 2 * 3;
    trderiv.dyy /= y2 * 2 * 1.5f;
    error2 /= norm;
    *error1 = sqrtf(error2);
    tr->dxc -= safety * trderiv.dxc;
    if (ifZoom1)
        tr->dxx -= safety * 0.5f * (trderiv.dxx + trderiv.dyy);
    tr->dxy -= safety * 0.5f * (trderiv.dxy - trderiv.dyx / (pixaspect * pixaspect));
    tr->dyc -= safety * trderiv.dyc;
    if (ifZoom1)
        tr->dyy = tr->dxx;
    tr->dyx = -pixaspect * pixaspect * tr->dxy;
}

// MVDepan.cpp:203-234
static inline void depan_reject_bad_blocks(const DepanTransform *tr, const float *blockDx, const float *blockDy, const int64_t *blockSAD, const int *blockX, const int *blockY,
                                           float *blockWeight, int nBlkX, int nBlkY, float wrongDif, float globalDif, int64_t thSCD1, float zeroWeight,
                                           const float *blockWeightMask, int ignoredBorder) {
    for (int j = 0; j < nBlkY; j++) {
        for (int i = 0; i < nBlkX; i++) {
            int n = j * nBlkX + i;
            // without the ignored border (a mask clip) the reference reads neighbours outside the arrays; the library skips the test there
            const bool inside = n - 1 - nBlkX >= 0 && n + 1 + nBlkX < nBlkX * nBlkY;
            if (i < ignoredBorder || i >= nBlkX - ignoredBorder || j < ignoredBorder || j >= nBlkY - ignoredBorder) {
                blockWeight[n] = 0;
            } else if (blockSAD[n] > thSCD1) {
                blockWeight[n] = 0;
            } else if (i > 0 && i < (nBlkX - 1) && inside && (fabsf((blockDx[n - 1 - nBlkX] + blockDx[n - nBlkX] + blockDx[n + 1 - nBlkX] +
                                                          blockDx[n - 1] + blockDx[n + 1] +
                                                          blockDx[n - 1 + nBlkX] + blockDx[n + nBlkX] + blockDx[n + 1 + nBlkX]) / 8 - blockDx[n]) > wrongDif)) {
                blockWeight[n] = 0;
            } else if (j > 0 && j < (nBlkY - 1) && inside && (fabsf((blockDy[n - 1 - nBlkX] + blockDy[n - nBlkX] + blockDy[n + 1 - nBlkX] +
                                                          blockDy[n - 1] + blockDy[n + 1] +
                                                          blockDy[n - 1 + nBlkX] + blockDy[n + nBlkX] + blockDy[n + 1 + nBlkX]) / 8 - blockDy[n]) > wrongDif)) {
                blockWeight[n] = 0;
            } else if (fabsf(tr->dxc + tr->dxx * blockX[n] + tr->dxy * blockY[n] - blockX[n] - blockDx[n]) > globalDif) {
                blockWeight[n] = 0;
            } else if (fabsf(tr->dyc + tr->dyx * blockX[n] + tr->dyy * blockY[n] - blockY[n] - blockDy[n]) > globalDif) {
                blockWeight[n] = 0;
            } else if (blockDx[n] == 0.0f && blockDy[n] == 0.0f) {
                blockWeight[n] = zeroWeight * blockWeightMask[n];
            } else {
                blockWeight[n] = blockWeightMask[n];
            }
        }
    }
}

struct DepanAnalyseParams {
    int nBlkX, nBlkY, nBlkSizeX, nBlkSizeY, stepX, stepY, nPel, nLvCount, isBackward;
    int width, height;
    int zoom, rot, fields, hasMask;
    float pixaspect, error, wrong, zerow;
    int64_t thscd1; int thscd2;
};
struct DepanMotion { float dx, dy, zoom, rot; int iter; float error; };
// what DepanAnalyse reads of one frame: the verdict of fgopIsUsable, and per block of level 0 the vector, its SAD and the mask byte under
// the block's centre (-1: no mask, or a centre outside the frame: weight 1.0f, MVDepan.cpp:309-312)
struct DepanGather { int x, y; long long sad; };

// MVDepan.cpp:279-399 for one frame.  rec: nBlkX * nBlkY level-0 records (read only when usable); maskv: per block the mask byte or -1.
// top_field is read with fields only.  Where |dx| < 0.01 the reference draws the sign of 0.011 from rand(); this returns +0.011f.
static inline void depan_estimate(const DepanAnalyseParams &P, bool usable, const DepanGather *rec, const int *maskv, int top_field, DepanMotion *out) {
    const int nb = P.nBlkX * P.nBlkY;
    const int nFields = P.fields ? 2 : 1;
    std::vector<float> blockDx(nb), blockDy(nb), blockWeight(nb), blockWeightMask(nb);
    std::vector<int64_t> blockSAD(nb);
    std::vector<int> blockX(nb), blockY(nb);
    DepanTransform tr;
    depan_set_null(&tr);
    float errorcur = P.error * 2;
    int iter = 0;
    if (usable) {
        const float dPel = 1.0f / P.nPel;
        for (int j = 0; j < P.nBlkY; j++) {
            for (int i = 0; i < P.nBlkX; i++) {
                int n = j * P.nBlkX + i;
                blockDx[n] = rec[n].x * dPel;
                blockDy[n] = rec[n].y * dPel;
                blockSAD[n] = rec[n].sad;
                blockX[n] = i * P.stepX + P.nBlkSizeX / 2;
                blockY[n] = j * P.stepY + P.nBlkSizeY / 2;
                if (P.hasMask && maskv[n] >= 0)
                    blockWeightMask[n] = maskv[n];
                else
                    blockWeightMask[n] = 1.0f;
                blockWeight[n] = blockWeightMask[n];
            }
        }
        float safety = 0.3f;
        int ifRot0 = 0;
        int ifZoom0 = 0;
        float globalDif0 = 1000.0f;
        int ignoredBorder = P.hasMask ? 0 : 4;
        for (; iter < 5; iter++) {
            depan_transform_update(&tr, blockDx.data(), blockDy.data(), blockX.data(), blockY.data(), blockWeight.data(), P.nBlkX, P.nBlkY, safety, ifZoom0, ifRot0, &errorcur, P.pixaspect / nFields);
            depan_reject_bad_blocks(&tr, blockDx.data(), blockDy.data(), blockSAD.data(), blockX.data(), blockY.data(), blockWeight.data(), P.nBlkX, P.nBlkY, P.wrong, globalDif0, P.thscd1, P.zerow,
                                    blockWeightMask.data(), ignoredBorder);
        }
        const float errordif = 0.01f;
        for (; iter < 100; iter++) {
            if (iter < 8)
                safety = 0.3f;
            else if (iter < 10)
                safety = 0.6f;
            else
                safety = 1.0f;
            float errorprev = errorcur;
            depan_transform_update(&tr, blockDx.data(), blockDy.data(), blockX.data(), blockY.data(), blockWeight.data(), P.nBlkX, P.nBlkY, safety, P.zoom, P.rot, &errorcur, P.pixaspect / nFields);
            if (((errorprev - errorcur) < errordif * 0.5f && iter > 9) || errorcur < errordif)
                break;
            float globalDif = errorcur * 2;
            depan_reject_bad_blocks(&tr, blockDx.data(), blockDy.data(), blockSAD.data(), blockX.data(), blockY.data(), blockWeight.data(), P.nBlkX, P.nBlkY, P.wrong, globalDif, P.thscd1, P.zerow,
                                    blockWeightMask.data(), ignoredBorder);
        }
    }
    float xcenter = (float)P.width / 2;
    float ycenter = (float)P.height / 2;
    float motionx = 0.0f, motiony = 0.0f, motionrot = 0.0f, motionzoom = 1.0f;
    if (errorcur < P.error) {
        if (P.isBackward) {
            DepanTransform trinv;
            depan_inversetransform(&tr, &trinv);
            depan_transform2motion(&trinv, 0, xcenter, ycenter, P.pixaspect / nFields, &motionx, &motiony, &motionrot, &motionzoom);
        } else
            depan_transform2motion(&tr, 1, xcenter, ycenter, P.pixaspect / nFields, &motionx, &motiony, &motionrot, &motionzoom);
        if (P.fields) {
            float yadd = top_field ? 0.5f : -0.5f;
            yadd = yadd * 2;
            motiony += yadd;
        }
        if (fabsf(motionx) < 0.01f)
            motionx = 0.011f; // the reference: (rand() > RAND_MAX / 2) ? 0.011f : -0.011f
    }
    out->dx = motionx; out->dy = motiony; out->zoom = motionzoom; out->rot = motionrot; out->iter = iter; out->error = errorcur;
}

// the level-0 records and the verdict of fgopIsUsable (Fakery.c:52-58,103-107,144-146) of a host blob; NULL: not usable
static inline bool depan_gather_host(const DepanAnalyseParams &P, const unsigned char *blob, const unsigned char *mask, long long mask_pitch, DepanGather *rec, int *maskv) {
    const int nb = P.nBlkX * P.nBlkY;
    bool usable = false;
    if (blob) {
        const unsigned char *p = blob + 8;
        for (int i = P.nLvCount - 1; i >= 1; i--) { int sz; memcpy(&sz, p, 4); p += sz; }
        memcpy(rec, p + 4, (size_t)nb * sizeof(DepanGather));
        int valid; memcpy(&valid, blob + 4, 4);
        int over = 0;
        for (int n = 0; n < nb; n++) over += rec[n].sad > P.thscd1 ? 1 : 0;
        usable = valid == 1 && !(over > P.thscd2);
    }
    for (int j = 0; j < P.nBlkY; j++)
        for (int i = 0; i < P.nBlkX; i++) {
            const int bx = i * P.stepX + P.nBlkSizeX / 2, by = j * P.stepY + P.nBlkSizeY / 2;
            maskv[j * P.nBlkX + i] = (mask && bx < P.width && by < P.height) ? mask[bx + by * mask_pitch] : -1;
        }
    return usable;
}
