// depan_warp_emu.cpp -- test infrastructure: the per-sample text of DepanCompensate and DepanStabilise with the host side of its records
// (csrc/mvx_depan_sample.h: what the GPU kernel runs per thread, and the record fill the library's *_frames functions call) and
// DepanStabilise's host planner (csrc/mvx_depan_stab_host.h), compiled for the host, one plane per call, so that tests/test_depan_ref.py
// and tests/test_depan_stab_ref.py can hold them to the restatements without a GPU.  With -DDEPAN_EMU_MAIN it is a stand-alone program.
#include <string.h>
#include <vector>
#include "mvx_depan_stab_host.h"
#include "mvx_depan_sample.h"

template <typename T, int NSRC> static void paint(const DCPlane *S, const DCCommon &C, int sub) {
    for (int h = 0; h < S[DS_CUR].H; h++)
        for (int row = 0; row < S[DS_CUR].W; row++) {
            if (sub == 0) dc_store<T, 0, NSRC>(S, C, h, row);
            else if (sub == 1) dc_store<T, 1, NSRC>(S, C, h, row);
            else dc_store<T, 2, NSRC>(S, C, h, row);
        }
}

// one plane p of a frame with subsampling ssw / ssh, through nsrc records filled as the library fills them
static void plane(int nsrc, const unsigned char *const *srcs, long long spitch, int W, int H, int bps, int sub, int mirror, int pixel_max, int border, int blur,
                  int ssw, int ssh, int p, const float *trs, unsigned char *dst, long long dpitch) {
    DCClip G;
    memset(&G, 0, sizeof(G));
    G.ssw = ssw; G.ssh = ssh; G.subpixel = sub;
    G.W[p] = W; G.H[p] = H; G.border[p] = border; G.blur[p] = blur; G.spitch[p] = spitch; G.dpitch[p] = dpitch;
    DCPlane S[DS_SOURCES];
    memset(S, 0, sizeof(S));
    std::vector<float> chain[DS_SOURCES];
    for (int s = 0; s < nsrc; s++) {
        if (!srcs[s]) continue;
        chain[s].resize(dc_fill(G, p, srcs[s], dst, trs + 6 * s, s != DS_CUR, &S[s]));
        if (chain[s].empty()) continue;
        S[s].chain = chain[s].data();
        for (int h = 0; h < H; h++) dc_chain_row(S[s], h);
    }
    if (nsrc == DS_SOURCES) ds_borders(S, border);
    const DCCommon C = { mirror, pixel_max, 1 };
    if (nsrc == 1) { if (bps == 1) paint<unsigned char, 1>(S, C, sub); else paint<unsigned short, 1>(S, C, sub); }
    else { if (bps == 1) paint<unsigned char, DS_SOURCES>(S, C, sub); else paint<unsigned short, DS_SOURCES>(S, C, sub); }
}

// DepanCompensate: tr is the plane's own transform
extern "C" void depan_emu_plane(const unsigned char *src, long long spitch, int W, int H, int bps, int sub, int mirror, int pixel_max, int border, int blur,
                                const float *tr, unsigned char *dst, long long dpitch) {
    plane(1, &src, spitch, W, H, bps, sub, mirror, pixel_max, border, blur, 0, 0, 0, tr, dst, dpitch);
}

// DepanStabilise.  srcs: the current, next and prev source planes (NULL: that pass does not exist), all W x H with pitch spitch; trs: their
// luma transforms, 6 floats each; border / blur: the plane's
extern "C" void depan_stab_emu_plane(const unsigned char *const srcs[3], long long spitch, int W, int H, int bps, int sub, int mirror, int pixel_max, int border, int blur,
                                     int ssw, int ssh, int p, const float *trs, unsigned char *dst, long long dpitch) {
    plane(DS_SOURCES, srcs, spitch, W, H, bps, sub, mirror, pixel_max, border, blur, ssw, ssh, p, trs, dst, dpitch);
}

// ints: width height num_frames addzoom prev next mirror blur subpixel fitlast method fields; floats: cutoff damping initzoom dxmax dymax zoommax
// rotmax pixaspect tzoom.  motions: of the data frames of the window of ndest.  out: the 28 words of DepanStabPlan
extern "C" void depan_stab_emu_plan(const int *ints, const float *floats, long long fps_num, long long fps_den, int ndest, const float *motions, unsigned *out) {
    DepanStabParams P;
    P.width = ints[0]; P.height = ints[1]; P.num_frames = ints[2]; P.addzoom = ints[3]; P.prev = ints[4]; P.next = ints[5]; P.mirror = ints[6]; P.blur = ints[7];
    P.subpixel = ints[8]; P.fitlast = ints[9]; P.method = ints[10]; P.fields = ints[11];
    P.cutoff = floats[0]; P.damping = floats[1]; P.initzoom = floats[2]; P.dxmax = floats[3]; P.dymax = floats[4]; P.zoommax = floats[5]; P.rotmax = floats[6];
    P.pixaspect = floats[7]; P.tzoom = floats[8];
    depan_stab_init(&P, fps_num, fps_den);
    DepanStabPlan plan;
    depan_stab_plan(&P, ndest, motions, &plan);
    static_assert(sizeof(plan) == 28 * 4, "DepanStabPlan is 28 words");
    memcpy(out, &plan, sizeof(plan));
}

#ifdef DEPAN_EMU_MAIN
// The same three functions as a stand-alone program, so that the tests can run them under AddressSanitizer and UBSan without loading
// anything into python.  Sources and destination are heap blocks of exactly the plane's size, so that a sanitizer sees any index outside them.
//   depan_warp_emu compensate IN OUT -> OUT: the destination plane
//     IN: W H bps sub mirror pixel_max border blur as ints, six floats, the source plane without padding
//   depan_warp_emu plane IN OUT      -> OUT: the destination plane
//     IN: W H bps sub mirror pixel_max border blur ssw ssh p has_next has_prev as ints, 18 floats (the luma transforms of cur, next, prev), then
//     the source planes present, without padding
//   depan_warp_emu plan IN           -> the 28 words of the plan as hex
//     IN: 12 ints and 9 floats as depan_stab_emu_plan takes them, fps_num and fps_den as int64, ndest and the number of motions as ints, the motions
#include <stdio.h>
int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 2;
    if (!strcmp(argv[1], "plan")) {
        int ints[12], tail[2];
        float floats[9];
        long long fps[2];
        if (fread(ints, 4, 12, f) != 12 || fread(floats, 4, 9, f) != 9 || fread(fps, 8, 2, f) != 2 || fread(tail, 4, 2, f) != 2 || tail[1] < 1) return 2;
        std::vector<float> motions((size_t)tail[1] * 4);
        if (fread(motions.data(), 4, motions.size(), f) != motions.size()) return 2;
        fclose(f);
        unsigned w[28];
        depan_stab_emu_plan(ints, floats, fps[0], fps[1], tail[0], motions.data(), w);
        for (int i = 0; i < 28; i++) printf("%x%c", w[i], i == 27 ? '\n' : ' ');
        return 0;
    }
    const bool stab = !strcmp(argv[1], "plane");
    if ((!stab && strcmp(argv[1], "compensate")) || argc != 4) return 2;
    int hd[13] = { 0 };
    float trs[18];
    if (fread(hd, 4, stab ? 13 : 8, f) != (stab ? 13u : 8u) || fread(trs, 4, stab ? 18 : 6, f) != (stab ? 18u : 6u)) return 2;
    const size_t n = (size_t)hd[0] * hd[1] * hd[2];
    std::vector<unsigned char> src[3], dst(n);
    const unsigned char *srcs[3] = { nullptr, nullptr, nullptr };
    for (int s = 0; s < 3; s++) {
        if (s && !hd[10 + s]) continue;
        src[s].resize(n);
        if (fread(src[s].data(), 1, n, f) != n) return 2;
        srcs[s] = src[s].data();
    }
    fclose(f);
    const long long pitch = (long long)hd[0] * hd[2];
    if (stab) depan_stab_emu_plane(srcs, pitch, hd[0], hd[1], hd[2], hd[3], hd[4], hd[5], hd[6], hd[7], hd[8], hd[9], hd[10], trs, dst.data(), pitch);
    else depan_emu_plane(srcs[0], pitch, hd[0], hd[1], hd[2], hd[3], hd[4], hd[5], hd[6], hd[7], trs, dst.data(), pitch);
    f = fopen(argv[3], "wb");
    if (!f || fwrite(dst.data(), 1, n, f) != n) return 2;
    fclose(f);
    return 0;
}
#endif
