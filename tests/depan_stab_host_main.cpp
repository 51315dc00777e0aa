// depan_stab_host_main.cpp -- test infrastructure: DepanStabilise's host planner (csrc/mvx_depan_stab_host.h) and its per-sample selection
// compiled for the host (csrc/mvx_depan_stab_sample.h) as a stand-alone program, so that tests/test_depan_stab_ref.py can run both under
// AddressSanitizer and UBSan without loading anything into python.
//   depan_stab_host_main plan IN        -> the 28 words of the plan as hex
//     IN: 12 ints and 9 floats as depan_stab_emu_plan takes them, fps_num and fps_den as int64, ndest and the number of motions as ints, the motions
//   depan_stab_host_main plane IN OUT   -> OUT: the destination plane
//     IN: W H bps sub mirror pixel_max border blur ssw ssh p has_next has_prev as ints, 18 floats (the luma transforms of cur, next, prev), then
//     the source planes present, without padding.  Sources and destination are heap blocks of exactly the plane's size, so that a sanitizer
//     sees any index outside them.
#include <stdio.h>
#include "depan_stab_emu.cpp"

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
    if (strcmp(argv[1], "plane") || argc != 4) return 2;
    int hd[13];
    float trs[18];
    if (fread(hd, 4, 13, f) != 13 || fread(trs, 4, 18, f) != 18) return 2;
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
    depan_stab_emu_plane(srcs, (long long)hd[0] * hd[2], hd[0], hd[1], hd[2], hd[3], hd[4], hd[5], hd[6], hd[7], hd[8], hd[9], hd[10], trs, dst.data(), (long long)hd[0] * hd[2]);
    f = fopen(argv[3], "wb");
    if (!f || fwrite(dst.data(), 1, n, f) != n) return 2;
    fclose(f);
    return 0;
}
