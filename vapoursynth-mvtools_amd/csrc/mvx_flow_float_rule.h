// mvx_flow_float_rule.h -- the per-sample arithmetic of the float FlowInter and FlowFPS (mvx_flowinter_create_float, mvx_flowfps_create_float),
// for device and host: FlowInterSimple (MaskFun.cpp:493-551), FlowInter (:374-414), FlowInterExtra (:417-490) and Blend (:349-371) on float32.
// The helpers are the float BlockFPS's (mvx_blockfps_float_rule.h): the time weights stay the integers t and 256 - t and the ">> 8" becomes a
// multiplication by the exact 1 / 256; the mask mixes divide by 255, the weights' own sum, where the reference has "(... + 255) >> 8".  No
// rounding term, no clamp to a sample range: float samples may be negative or overshoot.  Every operation is rounded on its own: build with
// -ffp-contract=off (build.py has it).  Minimum and maximum are comparisons that give the SECOND operand on a tie.
// Simple has ONE formula at every t: the reference's own formula at t = 128, ((dF + dB) * 256 + (dB - dF) * (mF - mB)) >> 9, is the general
// one with both ">> 8" stages merged into one and 256 in the place of the masks' 255 -- (dF + dB) / 2 + (dB - dF) * (mF - mB) / 512 against
// the general (dF + dB) / 2 + (dB - dF) * (mF - mB) / 510, within peak / 512 of each other -- so it is the general one up to the
// reference's rounding, and float32 has no shift to save.
// dF: the fetch from the left super frame along the forward vector scaled by t; dB: the fetch from the right one along the backward vector
// scaled by 256 - t; dF0 / dB0: the left / right sample at the output position; dFF / dBB: the Extra fetches (forward vector at nleft from
// the left frame, backward vector at nright from the right one); mF / mB: the upsized occlusion masks, 0..255.
// tests/flow_float_rule_host_main.cpp runs this header on the host against the numpy restatement (tests/flow_float_ref.py).  Internal; not
// part of the ABI.
#pragma once
#include "mvx_blockfps_float_rule.h"

// FlowInterSimple: the left term takes dB where the forward mask is set, the right term dF where the backward mask is set
MVX_BFF_HD float mvx_flf_simple(int t, float dF, float dB, int mF, int mB) {
    return mvx_bff_time(mvx_bff_mix(mB, dF, dB), mvx_bff_mix(mF, dB, dF), t);
}
// FlowInter: under a mask the other direction's fetch, and under both masks the own frame's sample at the output position
MVX_BFF_HD float mvx_flf_regular(int t, float dF, float dB, float dF0, float dB0, int mF, int mB) {
    const float a = mvx_bff_mix(mF, mvx_bff_mix(mB, dF0, dB), dF), b = mvx_bff_mix(mB, mvx_bff_mix(mF, dB0, dF), dB);
    return mvx_bff_time(b, a, t);
}
// FlowInterExtra: under a mask the extra fetch clamped between dB and dF
MVX_BFF_HD float mvx_flf_extra(int t, float dF, float dB, float dFF, float dBB, int mF, int mB) {
    const float lo = mvx_bff_min(dB, dF), hi = mvx_bff_max(dB, dF);
    const float medBB = mvx_bff_max(lo, mvx_bff_min(dBB, hi)), medFF = mvx_bff_max(lo, mvx_bff_min(dFF, hi));
    return mvx_bff_time(mvx_bff_mix(mB, medFF, dB), mvx_bff_mix(mF, medBB, dF), t);
}
// Blend of the clip frames, for a job whose vectors are not usable (blend = 1)
MVX_BFF_HD float mvx_flf_blend(int t, float l, float r) { return mvx_bff_time(r, l, t); }
