// sb_batch_forces_math.h -- the float arithmetic of sb_batch_forces_device that sb_physics.h does not hand out as a value
// (DESIGN.md 5.32): the force_mag of a beam (sb_physics.h's sb_beam_eval keeps it to itself) and the terms one partner adds to a
// particle's contact sums (sb_collide_pair_at subtracts them from a particle record instead).  Same expressions, same order, one
// rounding per operator: build with -ffp-contract=off; `/` and sqrtf are the IEEE ones on the host and, under
// -fhip-fp32-correctly-rounded-divide-sqrt, on the device -- the bits of the short gated forms the step takes inside their gates
// (profiles/r02_exact_math_check.txt).  Compiles on the host too: tests/batch_forces_check.cpp runs it against the numpy
// restatement (tests/batch_forces_ref.py) under sanitizers.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SBF_HD __host__ __device__ __forceinline__
#else
#define SBF_HD static inline
#endif

SBF_HD float sbf_min(float a, float b) { return (b < a) ? b : a; } // sb_min / sb_max / sb_clamp of sb_physics.h
SBF_HD float sbf_max(float a, float b) { return (a < b) ? b : a; }
SBF_HD float sbf_clamp(float x, float lo, float hi) { return sbf_min(sbf_max(x, lo), hi); }

SBF_HD bool sbf_finite(float x)
{
    union { float f; uint32_t u; } v;
    v.f = x;
    return (v.u & 0x7f800000u) != 0x7f800000u;
}

// force_mag of compute.wgsl:110 (sb_physics.h:237) from the positions of the two endpoints and the beam's {target_length,
// last_length, spring, damp}: the length with the guard of :104-107 for a beam of length zero.  The reference's sign:
// positive where the beam is shorter than its target and pushes its endpoints apart, negative where it is stretched and pulls.
SBF_HD float sbf_force_mag(float ax, float ay, float bx, float by, float target_length, float last_length, float spring, float damp)
{
    const float dx = bx - ax, dy = by - ay;
    const float len0 = sqrtf(dx * dx + dy * dy);
    const float len = len0 == 0.0f ? sqrtf(0.0f * 0.0f + -1.0e-10f * -1.0e-10f) : len0; // length(vec2(0, -1e-10))
    return (target_length - len) * spring + (last_length - len) * damp;
}

// the contact sums of one particle; all +0 before its first partner
struct SbfContact {
    float push_x, push_y, impulse_x, impulse_y, depth;
    uint32_t partners;
};
SBF_HD SbfContact sbf_contact_zero()
{
    SbfContact c;
    c.push_x = c.push_y = c.impulse_x = c.impulse_y = c.depth = 0.0f;
    c.partners = 0u;
    return c;
}

// "is the particle at (dx, dy) from me, dist = sqrt(dx * dx + dy * dy), a partner?": compute.wgsl:150-155
SBF_HD bool sbf_is_partner(float dist, float two_r) { return dist == 0.0f || dist < two_r; }

// One partner (sbf_is_partner holds), (dx, dy) = its position - mine, (ux, uy) = my velocity - its velocity (:158): what
// sb_collide_pair_at would subtract from particle.a (push) and particle.v (impulse), subtracted from the sums in `c`.  A partner on
// my own spot counts with depth 2r and adds nothing else (the step only moves p.y there).  inv_dt2 == 0: divide by dt2.
SBF_HD void sbf_contact_add(SbfContact &c, float dx, float dy, float dist, float ux, float uy, float two_r, float friction,
                            float elasticity_coeff, float inv_dt2, float dt2)
{
    c.partners++;
    const float overlap = two_r - dist; // :164
    if (overlap > c.depth) c.depth = overlap;
    if (dist == 0.0f) return; // :151-154
    const float inv_dist = 1.0f / dist;
    const float nx = dx * inv_dist, ny = dy * inv_dist; // :156
    const float tx = -ny, ty = nx;                      // :157
    const float impulse_normal = elasticity_coeff * (ux * nx + uy * ny); // :159
    const float max_friction = impulse_normal * friction;                // :160
    const float impulse_tangent = sbf_clamp(ux * tx + uy * ty, -max_friction, max_friction); // :161
    c.impulse_x -= impulse_normal * nx + impulse_tangent * tx; // :162
    c.impulse_y -= impulse_normal * ny + impulse_tangent * ty;
    const float csx = nx * overlap * 0.5f, csy = ny * overlap * 0.5f; // (n * overlap) / 2
    if (inv_dt2 != 0.0f) { // :168
        c.push_x -= csx * inv_dt2;
        c.push_y -= csy * inv_dt2;
    } else {
        c.push_x -= csx / dt2;
        c.push_y -= csy / dt2;
    }
}
