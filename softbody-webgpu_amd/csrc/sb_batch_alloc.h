// sb_batch_alloc.h -- what the batch's adding calls share (sb_batch_add_beams_device, sb_batch_add_particles_device; DESIGN.md
// 5.24a): the vocabulary of their 8-word rows, and the allocator that hands a new beam or particle its DATA index -- a bitmap of
// the free indices of one scene, a popcount prefix over its words, "the r-th free index", and wave 0's finish: ranks from one
// ballot, the room test, the downgrade to FULL, the result row and the count words.  What a call then stores into its scene stays
// in that call's file.  All of it is integers.  The bitmap word and the r-th free index are host and device
// (tests/batch_alloc_check.cpp runs them under sanitizers); the workgroup and wave routines are device only.  Header-only and
// HIP-free on the host.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBA_HD __host__ __device__ inline
#else
#define SBA_HD inline
#endif

#define SBA_ROW_WORDS 8u   // sb_batch_new_beam, sb_batch_new_particle
#define SBA_COUNT_WORDS 4u // {added, invalid, the call's own code, full}

namespace sba {

// a row's verdict: CANDIDATE goes on to the call's own test (code -3: joined / blocked) and to the room
enum { CANDIDATE = 0, EMPTY = -1, INVALID = -2, OWN = -3, FULL = -4 };

SBA_HD float word_as_float(uint32_t w)
{
    float f;
    memcpy(&f, &w, sizeof f);
    return f;
}

SBA_HD uint32_t bitmap_words(uint32_t capacity) { return (capacity + 31u) >> 5; }

// Word w (< bitmap_words(capacity)) of the free bitmap: bit e set, data index 32 w + e is free -- below the capacity and its
// occupancy byte zero in `occ` and, where occ_b is not null, in `occ_b` too.  The bytes are read four to a load (little endian):
// a row of them is padded to a multiple of four, and the padding at and past the capacity is not looked at, whatever it holds.
// A scene never uploaded has no free index.
SBA_HD uint32_t free_word(const uint32_t *occ, const uint32_t *occ_b, uint32_t capacity, bool loaded, uint32_t w)
{
    uint32_t bits = 0u;
    for (uint32_t q = 0; q < 8u; q++) {
        const uint32_t d0 = 32u * w + 4u * q;
        if (d0 >= capacity) break;
        const uint32_t held = occ[d0 >> 2] | (occ_b ? occ_b[d0 >> 2] : 0u);
        for (uint32_t e = 0; e < 4u; e++)
            if (d0 + e < capacity && ((held >> (8u * e)) & 0xffu) == 0u) bits |= 1u << (4u * q + e);
    }
    return loaded ? bits : 0u;
}

// The r-th free index (r = 0: the smallest) of a bitmap of n_words words; prefix[w]: the free indices in words 0 .. w - 1,
// prefix[n_words]: all of them.  r < prefix[n_words] is the caller's to see to (the room test).
SBA_HD uint32_t nth_free(const uint32_t *free_bits, const uint32_t *prefix, uint32_t n_words, uint32_t r)
{
    uint32_t lo = 0u, hi = n_words; // the word with prefix[lo] <= r < prefix[lo + 1]
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= r) lo = mid;
        else hi = mid;
    }
    uint32_t bits = free_bits[lo];
    for (uint32_t t = r - prefix[lo]; t != 0u; t--) bits &= bits - 1u;
    return 32u * lo + (uint32_t)__builtin_ctz(bits);
}

#if defined(__HIPCC__)
#define SBA_MAX_WORDS 128u // a lane of wave 0 scans two words

// All lanes of a workgroup of `block` threads (a multiple of 64, tid its thread index): s_free[n_words] and s_pref[n_words + 1]
// of a scene in LDS, n_words = bitmap_words(capacity) <= SBA_MAX_WORDS.  One barrier inside, between the words and wave 0's scan
// of their popcounts (two words to a lane, six shuffles); the caller's next barrier publishes the prefix.
__device__ inline void fill_free(uint32_t *s_free, uint32_t *s_pref, uint32_t n_words, const uint32_t *occ, const uint32_t *occ_b,
                                 uint32_t capacity, bool loaded, uint32_t tid, uint32_t block)
{
    for (uint32_t w = tid; w < n_words; w += block) s_free[w] = free_word(occ, occ_b, capacity, loaded, w);
    __syncthreads();
    if (tid >= 64u) return;
    const uint32_t w0 = 2u * tid;
    const uint32_t c0 = w0 < n_words ? (uint32_t)__builtin_popcount(s_free[w0]) : 0u;
    const uint32_t c1 = w0 + 1u < n_words ? (uint32_t)__builtin_popcount(s_free[w0 + 1u]) : 0u;
    uint32_t run = c0 + c1; // inclusive over the lanes
    for (uint32_t step = 1u; step < 64u; step <<= 1) {
        const uint32_t below = (uint32_t)__shfl_up((int)run, step);
        if (tid >= step) run += below;
    }
    if (tid == 0u) s_pref[0] = 0u;
    if (w0 + 1u <= n_words) s_pref[w0 + 1u] = run - c1;
    if (w0 + 2u <= n_words) s_pref[w0 + 2u] = run;
}

// Wave 0's finish, a lane per row (all 64 lanes call it; a lane without a row brings EMPTY): `verdict` is the lane's after the
// call's own tests.  A CANDIDATE's rank r is the number of candidates in the lanes below it; it is added at slot live + r with
// the r-th free data index where live + r < capacity and r < the free count, else its verdict becomes FULL.
struct Finish {
    int32_t verdict;               // final
    bool add;                      // verdict == CANDIDATE
    uint32_t rank, index, n_added; // rank and data index of a lane that adds; lanes of the wave that add
    unsigned long long m_invalid, m_own, m_full;
};
__device__ inline Finish finish(int32_t verdict, uint32_t lane, uint32_t live, uint32_t capacity, const uint32_t *s_free, const uint32_t *s_pref,
                                uint32_t n_words)
{
    Finish f;
    const unsigned long long m_cand = __ballot(verdict == CANDIDATE);
    f.rank = (uint32_t)__popcll(m_cand & ((1ull << lane) - 1ull));
    f.index = 0u;
    if (verdict == CANDIDATE) {
        if (live + f.rank < capacity && f.rank < s_pref[n_words]) f.index = nth_free(s_free, s_pref, n_words, f.rank);
        else verdict = FULL;
    }
    f.verdict = verdict;
    f.add = verdict == CANDIDATE;
    f.n_added = (uint32_t)__popcll(__ballot(f.add));
    f.m_invalid = __ballot(verdict == INVALID), f.m_own = __ballot(verdict == OWN), f.m_full = __ballot(verdict == FULL);
    return f;
}

// the lane's word of the scene's `result` row (row: the lane has one of the k rows) and the scene's count words, the third of
// them the ballot of code -3; either pointer may be null
__device__ inline void report(const Finish &f, bool row, uint32_t lane, uint32_t scene, uint32_t k, int32_t *result, int32_t *counts)
{
    if (result && row) result[(size_t)scene * k + lane] = f.add ? (int32_t)f.index : f.verdict;
    if (counts && lane == 0u) {
        int32_t *c = counts + (size_t)scene * SBA_COUNT_WORDS;
        c[0] = (int32_t)f.n_added;
        c[1] = __popcll(f.m_invalid);
        c[2] = __popcll(f.m_own);
        c[3] = __popcll(f.m_full);
    }
}
#endif

} // namespace sba
