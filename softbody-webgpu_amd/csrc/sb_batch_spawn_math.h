// sb_batch_spawn_math.h -- "may this row become a particle, and does it touch that one?", the verdict of one
// sb_batch_new_particle row before the scene's room is looked at (sb_batch_add_particles_device, sb_batch_spawn.hip;
// include/softbody.h states it): empty, the reserved word, "x and y are finite", and the blocked rule over the
// rows of one call.  Host and device: integers and comparisons; the contact test the blocked rule is asked with is
// sb_contact_cells.h's (sb_touch_test, sb_touch / sb_touch_xy), which tests/batch_spawn_check.cpp calls too.  Header-only and
// HIP-free on the host.  The row's width, the codes every adding call shares and word_as_float are sb_batch_alloc.h's.
#pragma once
#include "sb_batch_alloc.h"

// (a row: {tag, x, y, vx, vy, ax, ay, reserved}, sb_batch_new_particle)
namespace sbs {

using sba::word_as_float;
// a row's verdict: sba::CANDIDATE (it goes on to the blocked test and to the room) or SB_BATCH_SPAWN_EMPTY / _INVALID
enum { SBS_CANDIDATE = sba::CANDIDATE, SBS_BLOCKED = sba::OWN }; // (SBS_CANDIDATE: the check program's name for it)
enum { SBS_DRY_RUN = 1u, SBS_SKIP_TOUCHING = 2u };

// "a finite number" by its bits (neither infinity nor NaN: the exponent is not all ones)
SBA_HD bool finite_bits(uint32_t w) { return (w & 0x7f800000u) != 0x7f800000u; }

// steps 1 and 2 of the definition on row `w` (SBA_ROW_WORDS words).  loaded: the scene was uploaded.
SBA_HD int row_verdict(const uint32_t *w, bool loaded)
{
    if ((int32_t)w[0] < 0) return sba::EMPTY;
    if (!loaded || w[7] != 0u || !finite_bits(w[1]) || !finite_bits(w[2])) return sba::INVALID;
    return sba::CANDIDATE;
}

// Step 3 for row j from what is known of the rows before it: verd[i] (steps 1 and 2), E[i] ("touches a particle slot < P"),
// hit[i] ("row j touches row i").  Row j itself: a candidate.
template <class Verd, class Bit, class Hit>
SBA_HD bool blocked(uint32_t j, bool e_j, Verd verd, Bit e, Hit hit)
{
    if (e_j) return true;
    for (uint32_t i = 0; i < j; i++)
        if (verd(i) == sba::CANDIDATE && !e(i) && hit(i)) return true;
    return false;
}

} // namespace sbs
