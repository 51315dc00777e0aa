// depan_stab_emu.cpp -- test infrastructure: DepanStabilise's per-sample selection (csrc/mvx_depan_stab_sample.h, the text the GPU kernel runs per
// thread) and its host planner (csrc/mvx_depan_stab_host.h) compiled for the host, so that tests/test_depan_stab_ref.py can hold them to the
// restatement without a GPU.  tests/depan_stab_host_main.cpp wraps the same two functions in a stand-alone program.
#include <string.h>
#include <vector>
#include "mvx_depan_stab_host.h"
#include "mvx_depan_stab_sample.h"

template <typename T> static void stab_plane(const DCPlane *S, const DCCommon &C, int sub) {
    for (int h = 0; h < S[DS_CUR].H; h++)
        for (int row = 0; row < S[DS_CUR].W; row++)
            ((T *)(S[DS_CUR].dst + (long long)h * S[DS_CUR].dpitch))[row] =
                (T)(sub == 0 ? ds_sample<T, 0>(S, C, h, row) : sub == 1 ? ds_sample<T, 1>(S, C, h, row) : ds_sample<T, 2>(S, C, h, row));
}

// one plane p of a frame with subsampling ssw / ssh.  srcs: the current, next and prev source planes (NULL: that pass does not exist), all W x H
// with pitch spitch; trs: their luma transforms, 6 floats each; border / blur: the plane's
extern "C" void depan_stab_emu_plane(const unsigned char *const srcs[3], long long spitch, int W, int H, int bps, int sub, int mirror, int pixel_max, int border, int blur,
                                     int ssw, int ssh, int p, const float *trs, unsigned char *dst, long long dpitch) {
    DCPlane S[DS_SOURCES];
    memset(S, 0, sizeof(S));
    std::vector<float> chain[DS_SOURCES];
    for (int s = 0; s < DS_SOURCES; s++) {
        if (!srcs[s]) continue;
        DCPlane &P = S[s];
        P.src = srcs[s]; P.dst = dst; P.spitch = spitch; P.dpitch = dpitch; P.W = W; P.H = H; P.blur = blur;
        ds_plane_transform(ssw, ssh, p, trs + 6 * s, &P);
        P.segs = (W + DC_SEG - 1) / DC_SEG;
        if (P.cls == 2 && (s != DS_CUR || sub < 2)) {
            chain[s].resize((size_t)H * P.segs * 2);
            P.chain = chain[s].data();
            for (int h = 0; h < H; h++) dc_chain_row(P, h);
        }
    }
    ds_borders(S, border);
    const DCCommon C = { mirror, pixel_max, 1 };
    if (bps == 1) stab_plane<unsigned char>(S, C, sub); else stab_plane<unsigned short>(S, C, sub);
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
