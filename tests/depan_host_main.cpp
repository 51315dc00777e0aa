// depan_host_main.cpp -- test infrastructure: DepanAnalyse's host estimator (csrc/mvx_depan_host.h) as a stand-alone program, so that
// tests/test_depan_host.py can run it under AddressSanitizer and UBSan without loading anything into python.
//   depan_host_main FIELD  ->  the bits of dx dy zoom rot error as hex words, then iter
// FIELD: 13 ints (nBlkX nBlkY nBlkSizeX nBlkSizeY nOverlapX nOverlapY nPel nLvCount isBackward width height hasMask thscd2), thscd1 as int64,
// the blob's size as int, the blob, and with hasMask a width x height mask plane.  Defaults of the filter otherwise.
#include <stdio.h>
#include <stdlib.h>
#include "mvx_depan_host.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[13], size;
    long long thscd1;
    if (fread(hd, 4, 13, f) != 13 || fread(&thscd1, 8, 1, f) != 1 || fread(&size, 4, 1, f) != 1 || size <= 0) return 2;
    std::vector<unsigned char> blob(size), mask;
    if (fread(blob.data(), 1, size, f) != (size_t)size) return 2;
    DepanAnalyseParams P;
    memset(&P, 0, sizeof(P));
    P.nBlkX = hd[0]; P.nBlkY = hd[1]; P.nBlkSizeX = hd[2]; P.nBlkSizeY = hd[3]; P.stepX = hd[2] - hd[4]; P.stepY = hd[3] - hd[5];
    P.nPel = hd[6]; P.nLvCount = hd[7]; P.isBackward = hd[8]; P.width = hd[9]; P.height = hd[10]; P.hasMask = hd[11]; P.thscd2 = hd[12];
    P.thscd1 = thscd1;
    P.zoom = 1; P.rot = 1; P.fields = 0; P.pixaspect = 1.0f; P.error = 15.0f; P.wrong = 10.0f; P.zerow = 0.05f;
    if (P.hasMask) {
        mask.resize((size_t)P.width * P.height);
        if (fread(mask.data(), 1, mask.size(), f) != mask.size()) return 2;
    }
    fclose(f);
    const int nb = P.nBlkX * P.nBlkY;
    std::vector<DepanGather> rec(nb);
    std::vector<int> maskv(nb);
    const bool usable = depan_gather_host(P, blob.data(), P.hasMask ? mask.data() : nullptr, P.width, rec.data(), maskv.data());
    DepanMotion m;
    depan_estimate(P, usable, rec.data(), maskv.data(), 0, &m);
    unsigned w[5];
    memcpy(&w[0], &m.dx, 4); memcpy(&w[1], &m.dy, 4); memcpy(&w[2], &m.zoom, 4); memcpy(&w[3], &m.rot, 4); memcpy(&w[4], &m.error, 4);
    printf("%x %x %x %x %x %x\n", w[0], w[1], w[2], w[3], w[4], (unsigned)m.iter);
    return 0;
}
