// sb_batch_add_math.h -- "may this row become a beam, and how long is it?", the verdict of one sb_batch_new_beam row before the
// scene's topology is looked at (sb_batch_add_beams_device, sb_batch_add.hip; include/softbody.h states it): empty,
// range, self, the reserved word, the length's resolution and "a finite number > 0".  Host and device: integers and comparisons
// plus, on the host, the current distance as the beam phase takes it -- float32, one rounding per operator in the order written
// (the library builds with -ffp-contract=off; tests/batch_add_check.cpp builds it the same way), the square root IEEE.  Every
// comparison with a NaN is false, so a NaN length is no length.  Header-only and HIP-free on the host.  The row's width, the
// codes every adding call shares and word_as_float are sb_batch_alloc.h's.
#pragma once
#include "sb_batch_alloc.h"

// (a row: {a, b, length, spring, damp, yield_strain, strain_break_limit, reserved}, sb_batch_new_beam)
namespace sbw {

using sba::word_as_float;
// a row's verdict: sba::CANDIDATE (it goes on to the joined test and to the room) or SB_BATCH_ADD_EMPTY / _INVALID
enum { SBW_JOINED = sba::OWN };
enum { SBW_DRY_RUN = 1u, SBW_LENGTH_CURRENT = 2u, SBW_SKIP_JOINED = 4u };

// the current distance of two particle records: sb_length(pb.x - pa.x, pb.y - pa.y), the beam phase's own expression (the
// kernel calls sb_length itself; this is the host's restatement of it for the check program)
inline float distance(float ax, float ay, float bx, float by)
{
    const float dx = bx - ax, dy = by - ay;
    return __builtin_sqrtf(dx * dx + dy * dy);
}

// "a finite number > 0" (NaN fails the first comparison, +inf the second)
SBA_HD bool length_ok(float x) { return x > 0.0f && x <= 3.4028234663852886e38f; }

// range and self: the endpoints are two different data indices inside the capacity (a negative b is above it as unsigned)
SBA_HD bool ends_in_range(int32_t a, int32_t b, uint32_t max_particles)
{
    return a >= 0 && (uint32_t)a < max_particles && (uint32_t)b < max_particles && a != b;
}

// The verdict of row `w` (SBA_ROW_WORDS words).  loaded: the scene was uploaded; holds_a / holds_b: the endpoint is the data index
// of a particle slot < P (only looked at when the ends are in range); current: their current distance (only looked at when both
// hold a particle).  *length: the resolved rest length of a candidate.
SBA_HD int row_verdict(const uint32_t *w, uint32_t flags, uint32_t max_particles, bool loaded, bool holds_a, bool holds_b, float current,
                       float *length)
{
    const int32_t a = (int32_t)w[0], b = (int32_t)w[1];
    *length = 0.0f;
    if (a < 0) return sba::EMPTY;
    if (!loaded || !ends_in_range(a, b, max_particles) || !holds_a || !holds_b || w[7] != 0u) return sba::INVALID;
    const float len = (flags & SBW_LENGTH_CURRENT) ? current : word_as_float(w[2]);
    if (!length_ok(len)) return sba::INVALID;
    *length = len;
    return sba::CANDIDATE;
}

} // namespace sbw
