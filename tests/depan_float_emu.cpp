// depan_float_emu.cpp -- test infrastructure: the per-sample text of DepanCompensate and DepanStabilise on float clips
// (csrc/mvx_depan_sample_float.h: what depan_warp_kernel<float, ...> runs per thread) with the host side of its records (dc_fill, ds_borders
// of csrc/mvx_depan_sample.h, as the library's *_frames functions call them), compiled for the host, one plane per call, so that
// tests/test_depan_float_ref.py can hold it to tests/depan_float_ref.py without a GPU.  With -DDEPAN_EMU_MAIN it is a stand-alone program.
#include <string.h>
#include <vector>
#include "mvx_depan_sample_float.h"

template <int NSRC> static void paint(const DCPlane *S, const DCCommon &C, int sub) {
    for (int h = 0; h < S[DS_CUR].H; h++)
        for (int row = 0; row < S[DS_CUR].W; row++) {
            if (sub == 0) dcf_store<0, NSRC>(S, C, h, row);
            else if (sub == 1) dcf_store<1, NSRC>(S, C, h, row);
            else dcf_store<2, NSRC>(S, C, h, row);
        }
}

// one plane p (chroma: p > 0) of a frame with subsampling ssw / ssh, through nsrc records filled as the library fills them
static void plane(int nsrc, const unsigned char *const *srcs, long long spitch, int W, int H, int sub, int mirror, int blur, int ssw, int ssh, int p,
                  const float *trs, unsigned char *dst, long long dpitch) {
    DCClip G;
    memset(&G, 0, sizeof(G));
    G.bits = 32; G.ssw = ssw; G.ssh = ssh; G.subpixel = sub;
    G.W[p] = W; G.H[p] = H; G.border[p] = p ? 1 : 0; G.blur[p] = blur; G.spitch[p] = spitch; G.dpitch[p] = dpitch;
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
    if (nsrc == DS_SOURCES) ds_borders(S, G.border[p]);
    const DCCommon C = { mirror, 0, 1 };
    if (nsrc == 1) paint<1>(S, C, sub);
    else paint<DS_SOURCES>(S, C, sub);
}

// DepanCompensate: tr is the plane's own transform (p is 0 or 1 only to choose the border value)
extern "C" void depan_float_emu_plane(const unsigned char *src, long long spitch, int W, int H, int sub, int mirror, int chroma, int blur, const float *tr,
                                      unsigned char *dst, long long dpitch) {
    plane(1, &src, spitch, W, H, sub, mirror, blur, 0, 0, chroma ? 1 : 0, tr, dst, dpitch);
}

// DepanStabilise.  srcs: the current, next and prev source planes (NULL: that pass does not exist); trs: their luma transforms, 6 floats each
extern "C" void depan_float_stab_emu_plane(const unsigned char *const srcs[3], long long spitch, int W, int H, int sub, int mirror, int blur, int ssw, int ssh, int p,
                                           const float *trs, unsigned char *dst, long long dpitch) {
    plane(DS_SOURCES, srcs, spitch, W, H, sub, mirror, blur, ssw, ssh, p, trs, dst, dpitch);
}

#ifdef DEPAN_EMU_MAIN
// The same two functions as a stand-alone program, so that the tests can run them under AddressSanitizer and UBSan without loading anything
// into python.  Sources and destination are heap blocks of exactly the plane's size, so that a sanitizer sees any index outside them.
//   depan_float_emu compensate IN OUT : IN: W H sub mirror chroma blur as ints, six floats, the source plane (float32, no padding)
//   depan_float_emu plane IN OUT      : IN: W H sub mirror blur ssw ssh p has_next has_prev as ints, 18 floats (the luma transforms of cur, next,
//                                       prev), then the source planes present
//   OUT: the destination plane, which starts as 0xA5 bytes
#include <stdio.h>
int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const bool stab = !strcmp(argv[1], "plane");
    if (!stab && strcmp(argv[1], "compensate")) return 2;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 2;
    int hd[10] = { 0 };
    float trs[18];
    if (fread(hd, 4, stab ? 10 : 6, f) != (stab ? 10u : 6u) || fread(trs, 4, stab ? 18 : 6, f) != (stab ? 18u : 6u)) return 2;
    const size_t n = (size_t)hd[0] * hd[1] * 4;
    std::vector<unsigned char> src[3], dst(n, 0xA5);
    const unsigned char *srcs[3] = { nullptr, nullptr, nullptr };
    for (int s = 0; s < 3; s++) {
        if (s && (!stab || !hd[7 + s])) continue;
        src[s].resize(n);
        if (fread(src[s].data(), 1, n, f) != n) return 2;
        srcs[s] = src[s].data();
    }
    fclose(f);
    const long long pitch = (long long)hd[0] * 4;
    if (stab) depan_float_stab_emu_plane(srcs, pitch, hd[0], hd[1], hd[2], hd[3], hd[4], hd[5], hd[6], hd[7], trs, dst.data(), pitch);
    else depan_float_emu_plane(srcs[0], pitch, hd[0], hd[1], hd[2], hd[3], hd[4], hd[5], trs, dst.data(), pitch);
    f = fopen(argv[3], "wb");
    if (!f || fwrite(dst.data(), 1, n, f) != n) return 2;
    fclose(f);
    return 0;
}
#endif
