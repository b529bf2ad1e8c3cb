// sb_batch_pose_math.h -- the arithmetic of a pose row (sb_batch_pose_device of include/softbody.h): what a matched
// particle contributes to the eleven sums of its group, the five moments derived from them, and words 4 .. 16 of the row.  The one
// definition behind sb_batch_pose.hip and tests/batch_pose_check.cpp, which runs it on the host under the sanitizers; both build
// with -ffp-contract=off: one IEEE rounding per operator.  Only + - * / in double: no sqrt, atan2 or hypot, whose last bit this
// project does not pin on the device.  The sums themselves are sb_summary_math.h's (the pinned tree, sbu_sparse_step, sbu_canon).
#pragma once
#include "sb_summary_math.h"

#define SBP_NSUM 11u
// the columns of the sums, in the order of the definition
enum { SBP_X, SBP_Y, SBP_RX, SBP_RY, SBP_VX, SBP_VY, SBP_D, SBP_C, SBP_Q, SBP_Q0, SBP_L };
#define SBP_QNAN64 0x7FF8000000000000ull // the moment of a group without a matched member

SBU_HD double sbp_double(uint64_t w) { double x; memcpy(&x, &w, sizeof x); return x; }

// "has a reference": both of its floats are finite
SBU_HD bool sbp_ref_finite(sbu_float2 r) { return sbb_finite(r.x) && sbb_finite(r.y); }

// the leaves of a matched particle at p with velocity v whose reference is r.  Every float is cast to double first, so every
// product is exact (48 bits of 53) and each leaf is rounded once, in its sum or difference.
SBU_HD void sbp_leaves(sbu_float2 p, sbu_float2 v, sbu_float2 r, double (&out)[SBP_NSUM])
{
    const double x = (double)p.x, y = (double)p.y, X = (double)r.x, Y = (double)r.y, vx = (double)v.x, vy = (double)v.y;
    out[SBP_X] = x, out[SBP_Y] = y, out[SBP_RX] = X, out[SBP_RY] = Y, out[SBP_VX] = vx, out[SBP_VY] = vy;
    out[SBP_D] = x * X + y * Y;
    out[SBP_C] = X * y - Y * x;
    out[SBP_Q] = x * x + y * y;
    out[SBP_Q0] = X * X + Y * Y;
    out[SBP_L] = x * vy - y * vx;
}

// the moments about the centroids, from the sums S over n >= 1 matched members: a, b (the rotation from reference to current is
// atan2(b, a)), the moment of inertia I, the reference's I0, the spin Lc
struct SbpFit { double a, b, I, I0, Lc; };
SBU_HD SbpFit sbp_fit(const double *S, double n)
{
    SbpFit f;
    f.a = S[SBP_D] - (S[SBP_X] * S[SBP_RX] + S[SBP_Y] * S[SBP_RY]) / n;
    f.b = S[SBP_C] - (S[SBP_RX] * S[SBP_Y] - S[SBP_RY] * S[SBP_X]) / n;
    f.I = S[SBP_Q] - (S[SBP_X] * S[SBP_X] + S[SBP_Y] * S[SBP_Y]) / n;
    f.I0 = S[SBP_Q0] - (S[SBP_RX] * S[SBP_RX] + S[SBP_RY] * S[SBP_RY]) / n;
    f.Lc = S[SBP_L] - (S[SBP_X] * S[SBP_VY] - S[SBP_Y] * S[SBP_VX]) / n;
    return f;
}

// words 4 .. 16 of the row of a group with n >= 1 matched members, each rounded once from its double
SBU_HD void sbp_row_fit(float *row, const double *S, double n, const SbpFit &f)
{
    SBU_UNROLL
    for (int k = 0; k < 6; k++) row[4 + k] = (float)(S[k] / n); // the centroids: current, reference, velocity
    row[10] = (float)f.a, row[11] = (float)f.b, row[12] = (float)f.I, row[13] = (float)f.I0, row[14] = (float)f.Lc;
    row[15] = f.I > 0.0 ? (float)(f.Lc / f.I) : sbu_float(SBB_QNAN);  // the angular velocity
    row[16] = f.I0 > 0.0 ? (float)(f.I / f.I0) : sbu_float(SBB_QNAN); // the squared stretch
}
// the moments beside it
SBU_HD void sbp_moments(double *m, double n, const SbpFit &f) { m[0] = f.a, m[1] = f.b, m[2] = f.I, m[3] = f.I0, m[4] = f.Lc, m[5] = n, m[6] = 0.0, m[7] = 0.0; }

// word w of a row with no matched member behind word 3: 4 .. 16 NaN, 17 .. 23 zero; its moments: NaN x 5, then zeros
SBU_HD float sbp_unmatched_word(uint32_t w) { return w <= 16u ? sbu_float(SBB_QNAN) : 0.0f; }
SBU_HD double sbp_unmatched_moment(uint32_t w) { return w <= 4u ? sbp_double(SBP_QNAN64) : 0.0; }
