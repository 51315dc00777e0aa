// depan_estimate_host_main.cpp -- test infrastructure: DepanEstimate's host side (csrc/mvx_depan_estimate_host.h) as a stand-alone program, so that
// tests/test_depan_estimate_host.py can run it under AddressSanitizer and UBSan without loading anything into python.
//   depan_estimate_host_main FILE
// FILE: 4 floats (trust zoommax stab pixaspect), 13 ints (winx winy wleft wtop dxmax dymax fields tff tff_exists width height bits num_frames) as
// passed to creation, an int npairs, then per pair 2 ints (top_field or -1, frame number) and one scan (8 words) per window.
// Prints the resolved winx winy wleft wtop dxmax dymax windows, then per pair the bits of dx dy zoom trust as hex words, then -- the pairs taken as
// the frames 0 .. npairs - 1 of a clip of num_frames -- per frame the bits of stage 3's dx dy zoom.
#include <vector>
#include "mvx_depan_estimate_host.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    float fl[4];
    int hd[13], npairs;
    if (fread(fl, 4, 4, f) != 4 || fread(hd, 4, 13, f) != 13 || fread(&npairs, 4, 1, f) != 1 || npairs < 0) return 2;
    DepanEstimateParams P;
    memset(&P, 0, sizeof(P));
    P.trust_limit = fl[0]; P.zoommax = fl[1]; P.stab = fl[2]; P.pixaspect = fl[3];
    P.winx = hd[0]; P.winy = hd[1]; P.wleft = hd[2]; P.wtop = hd[3]; P.dxmax = hd[4]; P.dymax = hd[5]; P.fields = hd[6]; P.tff = hd[7]; P.tff_exists = hd[8];
    P.width = hd[9]; P.height = hd[10]; P.bits = hd[11]; P.num_frames = hd[12];
    if (const char *msg = depan_estimate_resolve(&P, false)) { printf("error %s\n", msg); return 0; }
    printf("%d %d %d %d %d %d %d\n", P.winx, P.winy, P.wleft, P.wtop, P.dxmax, P.dymax, P.nwin);
    std::vector<DepanEstimateResult> res(npairs);
    for (int i = 0; i < npairs; i++) {
        int tn[2];
        std::vector<DepanEstimateScan> scans(P.nwin);
        if (fread(tn, 4, 2, f) != 2 || fread(scans.data(), sizeof(DepanEstimateScan), P.nwin, f) != (size_t)P.nwin) return 2;
        if (!depan_estimate_pair(P, scans.data(), tn[0], tn[1], &res[i])) { printf("error no field\n"); return 0; }
        unsigned w[4];
        memcpy(w, &res[i], 16);
        printf("%x %x %x %x\n", w[0], w[1], w[2], w[3]);
    }
    fclose(f);
    for (int n = 0; n < npairs; n++) {
        const DepanEstimateResult tri[3] = { res[n > 0 ? n - 1 : 0], res[n], res[n + 1 < npairs ? n + 1 : npairs - 1] };
        float m[4];
        unsigned w[3];
        depan_estimate_finish(P, n, tri, m);
        memcpy(w, m, 12);
        printf("%x %x %x\n", w[0], w[1], w[2]);
    }
    return 0;
}
