// mvx_depan_stab_sample.h -- DepanStabilise's selection for one output sample now lives in mvx_depan_sample.h with DepanCompensate's
// interpolators and the host side of their records.  This header only forwards to it, under the names it had, so that host programs
// written against the two headers (the stand-alone emulations of earlier test suites) still compile and run the library's own text.
#pragma once
#include "mvx_depan_sample.h"
static inline void ds_plane_transform(int ssw, int ssh, int p, const float *tr, DCPlane *P) { dc_plane_transform(ssw, ssh, p, tr, P); }
