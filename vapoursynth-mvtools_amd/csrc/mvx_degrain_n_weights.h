// mvx_degrain_n_weights.h -- the arithmetic of mv.DegrainN that decides a block's weights, in one place for the device code
// (mvx_degrain_n.hip; mvx_degrain.hip takes dn_weight and, at creation, the threshold table from here too: mvx_block_shared.h) and for the
// stand-alone host program of the tests (tests/degrain_n_host_main.cpp).  It is the reference's
// template read at any radius: DegrainWeight (MVDegrains.h:184-189), normaliseWeights<radius> (MVDegrains.h:208-223), and the table of
// thresholds per temporal distance with its block-size normalisation (MVDegrains.cpp:658-661).  fp64 throughout; build with
// -ffp-contract=off.  Internal; not part of the ABI.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define DN_HD __host__ __device__ __forceinline__
#else
#define DN_HD static inline
#endif

#define DN_MAX_RADIUS 24
#define DN_MAX_REFS (2 * DN_MAX_RADIUS)

// MVDegrains.h:184-189.  The reference forms (thSAD - blockSAD) * (thSAD + blockSAD) * 256 in int64, which wraps for thresholds beyond
// about 1.9e8; the product is formed in uint64 here, which gives the same bits without signed overflow.
DN_HD int dn_weight(int64_t thSAD, int64_t blockSAD) {
    if (blockSAD >= thSAD) return 0;
    const int64_t num = (int64_t)((uint64_t)(thSAD - blockSAD) * (uint64_t)(thSAD + blockSAD) * 256u);
    return (int)((double)num / (double)(thSAD * thSAD + blockSAD * blockSAD));
}

// MVDegrains.h:208-223 in three steps, so that the weights can stay where they are (a list in memory) between them:
//   WSum = dn_wsum_begin() + every raw weight;  scale = dn_scale(WSum);  W[r] = dn_scaled(W[r], scale);  WSrc = 256 - every scaled weight
DN_HD int dn_wsum_begin(void) { return 256 + 1; }
DN_HD double dn_scale(int WSum) { return 256.0 / WSum; }
DN_HD int dn_scaled(int W, double scale) { return (int)(W * scale); }

// reference r (order mvbw, mvfw, mvbw2, mvfw2, ...) -> its temporal distance 1..radius
DN_HD int dn_distance(int r) { return r / 2 + 1; }

// ---- host side
// The user-scale threshold at distance d = 1..radius: t1 at d = 1, t2 at d = radius, a raised cosine in between (MDegrainN's thSAD2).
static inline int64_t dn_threshold(int64_t t1, int64_t t2, int radius, int d) {
    if (radius == 1 || t2 == t1) return t1;
    const double pi = 3.14159265358979323846;
    return (int64_t)floor((double)t2 + (double)(t1 - t2) * (1.0 + cos(pi * (double)(d - 1) / (double)(radius - 1))) / 2.0 + 0.5);
}
// MVDegrains.cpp:658-659: a threshold follows thscd1 through scaleThSCD
static inline int64_t dn_normalised(int64_t t, int64_t nSCD1, int64_t nSCD1_old) { return t * nSCD1 / nSCD1_old; }
// out[d - 1] for d = 1..radius; returns 0, or 1 when an entry reaches INT_MAX (MVDegrains.cpp:660-661)
static inline int dn_threshold_table(int64_t t1, int64_t t2, int radius, int64_t nSCD1, int64_t nSCD1_old, int64_t *out) {
    int over = 0;
    for (int d = 1; d <= radius; d++) {
        out[d - 1] = dn_normalised(dn_threshold(t1, t2, radius, d), nSCD1, nSCD1_old);
        if (out[d - 1] >= 2147483647LL) over = 1;
    }
    return over;
}
