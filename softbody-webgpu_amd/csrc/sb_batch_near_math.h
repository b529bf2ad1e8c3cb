// sb_batch_near_math.h -- "how far is this point from this particle, this beam, these walls, which of them is nearest and where on it?",
// the arithmetic behind sb_batch_nearest_device (sb_batch_nearest.hip); include/softbody.h states it row by row.
// Host and device: float32, one rounding per operator in the order written (the library builds with -ffp-contract=off;
// tests/batch_near_check.cpp builds it the same way), the division and the square root IEEE.  Every comparison with a NaN is false,
// so a NaN distance is never kept; an infinity follows the operators like any other number.  The winner is a minimum over 64-bit
// integer keys: no schedule can change a bit of it.  Header-only and HIP-free on the host.
#pragma once
#include "sb_query_key.h" // the kind, mask and wall words, the key and its decoding: shared with sb_batch_ray_math.h

#define SBN_HD SBQ_HD
#define SBN_ROW_WORDS SBQ_ROW_WORDS // {mask, px, py, rmax, skip_label, 0, 0, 0}: sb_batch_near_point
#define SBN_HIT_WORDS SBQ_HIT_WORDS
#define SBN_NO_KEY SBQ_NO_KEY

namespace sbn {
using namespace sbq; // (re-exported: MISS .. INVALID, MASK_*, WALL_*, word_as_float, float_as_word, finite_bits, skipped, pack, nearer,
                     // key_kind, key_index, out_kind, out_index)
enum { AT_A = 0, AT_B = 1, INSIDE = 2 }; // where on a segment its closest point lies

struct Probe {
    uint32_t mask;
    float px, py, rmax;
    int32_t skip;
    float rmax2; // rmax * rmax, once per row
};

// a row's verdict: MISS (it is asked), EMPTY or INVALID.  labels: the call has labels.
SBN_HD int row_verdict(const uint32_t *w, bool labels)
{
    if (w[0] == 0u) return EMPTY;
    if (w[0] & ~(uint32_t)MASK_KNOWN) return INVALID;
    if (!finite_bits(w[1]) || !finite_bits(w[2])) return INVALID;
    if (!(word_as_float(w[3]) >= 0.0f)) return INVALID; // (a NaN fails; +inf is legal)
    if ((w[5] | w[6] | w[7]) != 0u) return INVALID;
    if ((int32_t)w[4] != -1 && !labels) return INVALID;
    return MISS;
}

SBN_HD Probe probe_of(const uint32_t *w)
{
    Probe p{w[0], word_as_float(w[1]), word_as_float(w[2]), word_as_float(w[3]), (int32_t)w[4], 0.0f};
    p.rmax2 = p.rmax * p.rmax;
    return p;
}

// ---- the three distance tests: the squared distance from the probe to the closest point Q of a primitive
SBN_HD float d2_to(const Probe &p, float qx, float qy)
{
    const float vx = qx - p.px, vy = qy - p.py;
    return vx * vx + vy * vy;
}
// the segment from A to B: its closest point, the division behind the two sign tests (a degenerate segment has ee = 0 and so
// we = 0: endpoint A, nothing divided).  Returns AT_A, AT_B or INSIDE.
SBN_HD int segment_q(const Probe &p, float ax, float ay, float bx, float by, float *qx, float *qy)
{
    const float ex = bx - ax, ey = by - ay, wx = p.px - ax, wy = p.py - ay;
    const float ee = ex * ex + ey * ey, we = wx * ex + wy * ey;
    if (!(we > 0.0f)) {
        *qx = ax, *qy = ay;
        return AT_A;
    }
    if (!(we < ee)) {
        *qx = bx, *qy = by;
        return AT_B;
    }
    const float u = we / ee;
    *qx = ax + u * ex, *qy = ay + u * ey;
    return INSIDE;
}
SBN_HD float segment_d2(const Probe &p, float ax, float ay, float bx, float by)
{
    float qx, qy;
    segment_q(p, ax, ay, bx, by, &qx, &qy);
    return d2_to(p, qx, qy); // (at a clamped end: the particle's expression on that endpoint, bit for bit)
}
// one wall: only the coordinate across it counts
SBN_HD void wall_q(const Probe &p, float bounds, uint32_t wall, float *qx, float *qy)
{
    *qx = wall == WALL_LEFT ? 0.0f : wall == WALL_RIGHT ? bounds : p.px;
    *qy = wall == WALL_LOW ? 0.0f : wall == WALL_HIGH ? bounds : p.py;
}
SBN_HD float wall_d2(const Probe &p, float bounds, uint32_t wall)
{
    const bool in_x = wall == WALL_LEFT || wall == WALL_RIGHT;
    const float v = ((wall == WALL_LEFT || wall == WALL_LOW) ? 0.0f : bounds) - (in_x ? p.px : p.py);
    return v * v;
}

// ---- keys: kept iff d2 <= rmax2 (a NaN drops out; +inf is kept only under rmax = +inf).  d2 is a sum of squares, never -0: its
// bits order as the floats do.
// Two packings of one order: the batch's (16 bits of index) and the engine's (WIDE: 30 bits, sb_nearest.hip); one copy of the arithmetic.
SBN_HD uint64_t pack_wide(float d2, uint32_t kind, uint32_t index) { return ((uint64_t)float_as_word(d2) << 32) | ((uint64_t)kind << 30) | (uint64_t)index; }
template <bool WIDE>
SBN_HD uint64_t candidate_as(const Probe &p, float d2, uint32_t kind, uint32_t index)
{
    if (!(d2 <= p.rmax2)) return SBN_NO_KEY;
    return WIDE ? pack_wide(d2, kind, index) : pack(d2, kind, index);
}
template <bool WIDE>
SBN_HD uint64_t walls_as(const Probe &p, float bounds)
{
    uint64_t key = SBN_NO_KEY;
    for (uint32_t wall = WALL_LEFT; wall <= WALL_HIGH; wall <<= 1) key = nearer(key, candidate_as<WIDE>(p, wall_d2(p, bounds, wall), WALL, wall));
    return key;
}
SBN_HD uint64_t candidate(const Probe &p, float d2, uint32_t kind, uint32_t index) { return candidate_as<false>(p, d2, kind, index); }
SBN_HD uint64_t particle(const Probe &p, float cx, float cy, uint32_t index) { return candidate(p, d2_to(p, cx, cy), PARTICLE, index); }
SBN_HD uint64_t segment(const Probe &p, float ax, float ay, float bx, float by, uint32_t index) { return candidate(p, segment_d2(p, ax, ay, bx, by), BEAM, index); }
SBN_HD uint64_t walls(const Probe &p, float bounds) { return walls_as<false>(p, bounds); }
// the engine's packing of the same three distances (SBN_NO_KEY is above every wide key too: a wide key's kind is never 3 with an index of all ones)
SBN_HD uint64_t particle_wide(const Probe &p, float cx, float cy, uint32_t index) { return candidate_as<true>(p, d2_to(p, cx, cy), PARTICLE, index); }
SBN_HD uint64_t segment_wide(const Probe &p, float ax, float ay, float bx, float by, uint32_t index) { return candidate_as<true>(p, segment_d2(p, ax, ay, bx, by), BEAM, index); }
SBN_HD uint64_t walls_wide(const Probe &p, float bounds) { return walls_as<true>(p, bounds); }

// ---- a row's answer from its verdict and its smallest key (its kind and index: sb_query_key.h)
SBN_HD uint32_t key_d2(uint64_t key) { return (uint32_t)(key >> 32); }
// the d word: sqrt(d2) of the winner, the row's rmax bits verbatim on a miss, 0 for an empty or invalid row
SBN_HD uint32_t out_d(int verdict, uint64_t key, uint32_t rmax_bits)
{
    if (verdict != MISS) return 0u;
    return key == SBN_NO_KEY ? rmax_bits : float_as_word(__builtin_sqrtf(word_as_float(key_d2(key))));
}

// ---- the same answers from a wide key (index: 30 bits; key_d2 and out_d read the high word, which both packings share)
#define SBN_WIDE_INDEX_BITS 30u
SBN_HD uint32_t wide_kind(uint64_t key) { return (uint32_t)(key >> SBN_WIDE_INDEX_BITS) & 3u; }
SBN_HD uint32_t wide_index(uint64_t key) { return (uint32_t)key & ((1u << SBN_WIDE_INDEX_BITS) - 1u); }
SBN_HD int32_t out_kind_wide(int verdict, uint64_t key) { return verdict != MISS ? verdict : (key == SBN_NO_KEY ? (int32_t)MISS : (int32_t)wide_kind(key)); }
SBN_HD int32_t out_index_wide(int verdict, uint64_t key) { return verdict != MISS || key == SBN_NO_KEY ? -1 : (int32_t)wide_index(key); }

} // namespace sbn
