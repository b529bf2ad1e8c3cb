// sb_graph_math.h -- the key of a half-edge of a batch scene's beam graph (sb_batch_graph_device, sb_batch_graph.hip;
// include/softbody.h states the graph).  A listed beam at data index d that joins the particles a and b (data
// indices) has two half-edges: side 0 at a (its neighbour is b) and side 1 at b (its neighbour is a).  The key packs
// (particle data index, beam data index, side) into 10 + 12 + 1 bits, most significant first, so that the order of the keys as
// unsigned numbers IS the order of nbr's rows: by particle, inside a particle by beam data index, a beam from a particle to itself
// side 0 first.  No two half-edges of a scene share a key (a beam data index is listed once), so a sort of the keys has one result.
// Host and device: integers only.  Header-only and HIP-free on the host (tests/graph_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBG_HD __host__ __device__ inline
#else
#define SBG_HD inline
#endif

#define SBG_PARTICLE_BITS 10u // SB_BATCH_MAX_PARTICLES = 1024
#define SBG_BEAM_BITS 12u     // SB_BATCH_MAX_BEAMS = 4096
#define SBG_KEY_BITS (SBG_PARTICLE_BITS + SBG_BEAM_BITS + 1u)
#define SBG_NO_KEY 0xFFFFFFFFu // above every key: the padding of the sort, a beam slot that is not listed

namespace sbg {

SBG_HD uint32_t key(uint32_t particle, uint32_t beam, uint32_t side) { return (particle << (SBG_BEAM_BITS + 1u)) | (beam << 1) | side; }
SBG_HD uint32_t key_particle(uint32_t k) { return k >> (SBG_BEAM_BITS + 1u); }
SBG_HD uint32_t key_beam(uint32_t k) { return (k >> 1) & ((1u << SBG_BEAM_BITS) - 1u); }
SBG_HD uint32_t key_side(uint32_t k) { return k & 1u; }
// the smallest key a half-edge at `particle` can have (particle == the capacity: above every key of the scene, below SBG_NO_KEY)
SBG_HD uint32_t first_key_of(uint32_t particle) { return particle << (SBG_BEAM_BITS + 1u); }

// keys the sort of a scene of `half_edges` half-edges runs over: the smallest power of two >= half_edges (0 for none)
SBG_HD uint32_t sort_width(uint32_t half_edges)
{
    uint32_t n = half_edges ? 1u : 0u;
    while (n < half_edges) n <<= 1;
    return n;
}

// the number of keys below `bound` among the ascending keys[0 .. n-1]: row_ptr[p] is lower_bound(first_key_of(p))
SBG_HD uint32_t lower_bound(const uint32_t *keys, uint32_t n, uint32_t bound)
{
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] < bound) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// One compare-exchange of the bitonic network over `n` keys (a power of two), t = 0 .. n/2 - 1: for k = 2, 4 .. n and
// j = k/2, k/4 .. 1 the pass (k, j) orders the pair (i, i | j) ascending where i & k == 0, else descending.  Returns i.
SBG_HD uint32_t bitonic_low(uint32_t t, uint32_t j) { return ((t & ~(j - 1u)) << 1) | (t & (j - 1u)); }

// the whole network on the host, one pass after the other as the kernel runs them (tests/graph_check.cpp)
inline void bitonic_sort(uint32_t *keys, uint32_t n)
{
    for (uint32_t k = 2u; k <= n; k <<= 1)
        for (uint32_t j = k >> 1; j > 0u; j >>= 1)
            for (uint32_t t = 0; t < n / 2u; t++) {
                const uint32_t i = bitonic_low(t, j), l = i | j, x = keys[i], y = keys[l];
                if ((x > y) == ((i & k) == 0u)) keys[i] = y, keys[l] = x;
            }
}

} // namespace sbg
