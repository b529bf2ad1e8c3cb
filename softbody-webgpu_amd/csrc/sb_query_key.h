// sb_query_key.h -- what the queries of a scene share below their arithmetic ("which primitive does this ray meet first?",
// sb_batch_ray_math.h; "which is nearest to this point?", sb_batch_near_math.h): a row of eight words, the kind and mask words, the
// wall words, and the 64-bit integer key (bits of a non-negative float << 32) | (kind << 16) | index whose minimum wins -- on equal
// floats a particle beats a beam beats a wall, then the smaller index -- and is decoded into a row's kind and index (DESIGN.md
// 5.30).  The two headers re-export these names into sbr:: and sbn::; what one query alone needs stays in its header.  Host and
// device, header-only and HIP-free on the host.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBQ_HD __host__ __device__ inline
#else
#define SBQ_HD inline
#endif

#define SBQ_ROW_WORDS 8u // a query row; word 0 is its mask
#define SBQ_HIT_WORDS 3u // {kind, index, label}
#define SBQ_NO_KEY 0xFFFFFFFFFFFFFFFFull // above every key: no candidate yet (a key's kind field is never all ones)

namespace sbq {

// the kind word of a hit row; the three hits are also the kind field of a key
enum { MISS = 0, PARTICLE = 1, BEAM = 2, WALL = 3, EMPTY = -1, INVALID = -2 };
enum { MASK_PARTICLES = 1u, MASK_BEAMS = 2u, MASK_WALLS = 4u, MASK_KNOWN = 7u };
enum { WALL_LEFT = 1u, WALL_RIGHT = 2u, WALL_LOW = 4u, WALL_HIGH = 8u }; // SB_BATCH_WALL_*: the index of a wall

SBQ_HD float word_as_float(uint32_t w)
{
    float f;
    memcpy(&f, &w, sizeof f);
    return f;
}
SBQ_HD uint32_t float_as_word(float f)
{
    uint32_t w;
    memcpy(&w, &f, sizeof w);
    return w;
}
// "a finite number" by its bits (neither infinity nor NaN: the exponent is not all ones)
SBQ_HD bool finite_bits(uint32_t w) { return (w & 0x7f800000u) != 0x7f800000u; }

// "is a primitive of this label ignored by this row?" (-1 ignores nothing; without labels every label passed here is -1)
template <class Row>
SBQ_HD bool skipped(const Row &r, int32_t label) { return r.skip != -1 && label == r.skip; }

// ---- keys: f is never negative and never -0, so its bits order as the floats do
SBQ_HD uint64_t pack(float f, uint32_t kind, uint32_t index) { return ((uint64_t)float_as_word(f) << 32) | ((uint64_t)kind << 16) | (uint64_t)index; }
SBQ_HD uint64_t nearer(uint64_t x, uint64_t y) { return x < y ? x : y; }
SBQ_HD uint32_t key_kind(uint64_t key) { return (uint32_t)(key >> 16) & 0xffffu; }
SBQ_HD uint32_t key_index(uint64_t key) { return (uint32_t)key & 0xffffu; }
// a row's kind and index from its verdict and its smallest key
SBQ_HD int32_t out_kind(int verdict, uint64_t key) { return verdict != MISS ? verdict : (key == SBQ_NO_KEY ? (int32_t)MISS : (int32_t)key_kind(key)); }
SBQ_HD int32_t out_index(int verdict, uint64_t key) { return verdict != MISS || key == SBQ_NO_KEY ? -1 : (int32_t)key_index(key); }

} // namespace sbq
