// sb_batch_ray_math.h -- "where does this ray meet this disc, this segment, these walls, and which meeting wins?", the arithmetic
// behind sb_batch_raycast_device (sb_batch_raycast.hip); include/softbody.h states it row by row.  Host and
// device: float32, one rounding per operator in the order written (the library builds with -ffp-contract=off;
// tests/batch_ray_check.cpp builds it the same way), the division and the square root IEEE.  Every comparison with a NaN is false,
// so a NaN meets nothing; an infinity follows the operators like any other number.  The winner is a minimum over 64-bit integer
// keys: no schedule can change a bit of it.  Header-only and HIP-free on the host.
#pragma once
#include "sb_query_key.h" // the kind, mask and wall words, the key and its decoding: shared with sb_batch_near_math.h

#define SBR_HD SBQ_HD
#define SBR_ROW_WORDS SBQ_ROW_WORDS // {mask, ox, oy, dx, dy, tmax, skip_label, 0}: sb_batch_ray
#define SBR_HIT_WORDS SBQ_HIT_WORDS
#define SBR_NO_KEY SBQ_NO_KEY

namespace sbr {
using namespace sbq; // (re-exported: MISS .. INVALID, MASK_*, WALL_*, word_as_float, float_as_word, finite_bits, skipped, pack, nearer,
                     // key_kind, key_index, out_kind, out_index)

struct Ray {
    uint32_t mask;
    float ox, oy, dx, dy, tmax;
    int32_t skip;
    float a; // dx * dx + dy * dy, once per row
};

// a row's verdict: MISS (it is cast), EMPTY or INVALID.  labels: the call has labels.
SBR_HD int row_verdict(const uint32_t *w, bool labels)
{
    if (w[0] == 0u) return EMPTY;
    if (w[0] & ~(uint32_t)MASK_KNOWN) return INVALID;
    if (!finite_bits(w[1]) || !finite_bits(w[2]) || !finite_bits(w[3]) || !finite_bits(w[4])) return INVALID;
    if (!(word_as_float(w[5]) >= 0.0f)) return INVALID; // (a NaN fails; +inf is legal)
    if (w[7] != 0u) return INVALID;
    if ((int32_t)w[6] != -1 && !labels) return INVALID;
    return MISS;
}

SBR_HD Ray ray_of(const uint32_t *w)
{
    Ray r{w[0], word_as_float(w[1]), word_as_float(w[2]), word_as_float(w[3]), word_as_float(w[4]), word_as_float(w[5]), (int32_t)w[6], 0.0f};
    r.a = r.dx * r.dx + r.dy * r.dy;
    return r;
}

// every candidate: -0 becomes +0; kept iff 0 <= t <= tmax (*t: the kept t).  A key orders by (t, kind, index): t is non-negative, so
// its bits order as the floats do.  Two packings of one order: the batch's (16 bits of index) and the engine's (30 bits, sb_raycast.hip).
SBR_HD bool kept_t(const Ray &r, float t, float *out)
{
    t = t + 0.0f;
    if (!(t >= 0.0f && t <= r.tmax)) return false;
    *out = t;
    return true;
}
SBR_HD uint64_t pack_wide(float t, uint32_t kind, uint32_t index) { return ((uint64_t)float_as_word(t) << 32) | ((uint64_t)kind << 30) | (uint64_t)index; }
SBR_HD uint64_t candidate(const Ray &r, float t, uint32_t kind, uint32_t index) { return kept_t(r, t, &t) ? pack(t, kind, index) : SBR_NO_KEY; }

// "the t of this meeting, or none": the disc of centre (cx, cy) and squared radius r2
SBR_HD bool disc_t(const Ray &r, float cx, float cy, float r2, float *t)
{
    const float wx = cx - r.ox, wy = cy - r.oy;
    const float b = wx * r.dx + wy * r.dy, c = (wx * wx + wy * wy) - r2;
    if (c <= 0.0f) return kept_t(r, 0.0f, t); // the origin is inside
    if (!(b > 0.0f)) return false;
    const float q = b * b - r.a * c;
    if (!(q >= 0.0f)) return false;
    return kept_t(r, (b - __builtin_sqrtf(q)) / r.a, t);
}
SBR_HD uint64_t disc(const Ray &r, float cx, float cy, float r2, uint32_t index)
{
    float t;
    return disc_t(r, cx, cy, r2, &t) ? pack(t, PARTICLE, index) : SBR_NO_KEY;
}

// the segment from (ax, ay) to (bx, by): no division before a candidate is found
SBR_HD bool segment_t(const Ray &r, float ax, float ay, float bx, float by, float *t)
{
    const float ex = bx - ax, ey = by - ay, wx = ax - r.ox, wy = ay - r.oy;
    float den = r.dx * ey - r.dy * ex, tn = wx * ey - wy * ex, un = wx * r.dy - wy * r.dx;
    if (den == 0.0f) return false; // parallel or degenerate
    if (den < 0.0f) den = -den, tn = -tn, un = -un;
    if (!(0.0f <= un && un <= den && 0.0f <= tn)) return false; // (a NaN den fails here)
    return kept_t(r, tn / den, t);
}
SBR_HD uint64_t segment(const Ray &r, float ax, float ay, float bx, float by, uint32_t index)
{
    float t;
    return segment_t(r, ax, ay, bx, by, &t) ? pack(t, BEAM, index) : SBR_NO_KEY;
}

// the four lines x = 0, x = bounds, y = 0, y = bounds: at most two candidates; the other coordinate is not tested.  One copy of the
// arithmetic for both packings (WIDE: the engine's key).
template <bool WIDE>
SBR_HD uint64_t candidate_as(const Ray &r, float t, uint32_t kind, uint32_t index)
{
    if (!kept_t(r, t, &t)) return SBR_NO_KEY;
    return WIDE ? pack_wide(t, kind, index) : pack(t, kind, index);
}
template <bool WIDE>
SBR_HD uint64_t walls_as(const Ray &r, float bounds)
{
    uint64_t key = SBR_NO_KEY;
    if (r.dx < 0.0f) key = nearer(key, candidate_as<WIDE>(r, (0.0f - r.ox) / r.dx, WALL, WALL_LEFT));
    if (r.dx > 0.0f) key = nearer(key, candidate_as<WIDE>(r, (bounds - r.ox) / r.dx, WALL, WALL_RIGHT));
    if (r.dy < 0.0f) key = nearer(key, candidate_as<WIDE>(r, (0.0f - r.oy) / r.dy, WALL, WALL_LOW));
    if (r.dy > 0.0f) key = nearer(key, candidate_as<WIDE>(r, (bounds - r.oy) / r.dy, WALL, WALL_HIGH));
    return key;
}
SBR_HD uint64_t walls(const Ray &r, float bounds) { return walls_as<false>(r, bounds); }
// the engine's packing of the same three meetings (SBR_NO_KEY is above every wide key too: a wide key's kind is never 3 with an index of all ones)
SBR_HD uint64_t disc_wide(const Ray &r, float cx, float cy, float r2, uint32_t index)
{
    float t;
    return disc_t(r, cx, cy, r2, &t) ? pack_wide(t, PARTICLE, index) : SBR_NO_KEY;
}
SBR_HD uint64_t segment_wide(const Ray &r, float ax, float ay, float bx, float by, uint32_t index)
{
    float t;
    return segment_t(r, ax, ay, bx, by, &t) ? pack_wide(t, BEAM, index) : SBR_NO_KEY;
}
SBR_HD uint64_t walls_wide(const Ray &r, float bounds) { return walls_as<true>(r, bounds); }

// ---- a row's answer from its verdict and its smallest key (its kind and index: sb_query_key.h)
// the t word: the hit's t, the row's tmax bits verbatim on a miss, 0 for an empty or invalid row
SBR_HD uint32_t out_t(int verdict, uint64_t key, uint32_t tmax_bits)
{
    if (verdict != MISS) return 0u;
    return key == SBR_NO_KEY ? tmax_bits : (uint32_t)(key >> 32);
}

// ---- the same answers from a wide key (index: 30 bits)
#define SBR_WIDE_INDEX_BITS 30u
SBR_HD uint32_t wide_kind(uint64_t key) { return (uint32_t)(key >> SBR_WIDE_INDEX_BITS) & 3u; }
SBR_HD uint32_t wide_index(uint64_t key) { return (uint32_t)key & ((1u << SBR_WIDE_INDEX_BITS) - 1u); }
SBR_HD int32_t out_kind_wide(int verdict, uint64_t key) { return verdict != MISS ? verdict : (key == SBR_NO_KEY ? (int32_t)MISS : (int32_t)wide_kind(key)); }
SBR_HD int32_t out_index_wide(int verdict, uint64_t key) { return verdict != MISS || key == SBR_NO_KEY ? -1 : (int32_t)wide_index(key); }

} // namespace sbr
