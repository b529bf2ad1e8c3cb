// sb_summary_math.h -- the arithmetic of a summary row, the one definition behind sb_batch_summary.hip, sb_summary.hip,
// sb_batch_body_summary.hip and sb_body_summary.hip: what a particle and a beam contribute, the pinned tree, a level of the sparse
// tree over sorted members, words 6 .. 18 of a row.  Nothing here knows where a scene lies.  Host and device
// (tests/summary_math_check.cpp runs it under the host sanitizers); what needs a wave is device-only.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SBU_HD __host__ __device__ __forceinline__
typedef float2 sbu_float2;
#define SBU_UNROLL _Pragma("unroll")
#else
#define SBU_HD inline
#define SBU_UNROLL
struct sbu_float2 { float x, y; }; // (a name of its own: a host file may also see HIP's vector types)
#endif

// ---------------------------------------------------------------- the codec of a row's words
#define SBB_QNAN 0x7FC00000u // the word of a statistic over an empty set
SBU_HD uint32_t sbu_bits(float x) { uint32_t w; memcpy(&w, &x, sizeof w); return w; }
SBU_HD float sbu_float(uint32_t w) { float x; memcpy(&x, &w, sizeof x); return x; }
SBU_HD bool sbb_finite(float x) { return (sbu_bits(x) & 0x7f800000u) != 0x7f800000u; }
// finite floats as unsigned keys of the same order, -0.0 BELOW +0.0: a minimum over both zeros is -0.0, a maximum +0.0.  An extreme
// is a key from its first comparison on -- in a thread, in LDS, in HBM -- so which zero it returns never depends on which leaves
// share a thread.  A running maximum starts at SBB_KEY_LEAST, a running minimum at SBB_KEY_MOST: beyond the key of every float.
#define SBB_KEY_LEAST 0u
#define SBB_KEY_MOST 0xFFFFFFFFu
SBU_HD uint32_t sbb_fkey(float x) { const uint32_t b = sbu_bits(x); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
SBU_HD float sbb_unkey(uint32_t k) { return sbu_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
SBU_HD uint32_t sbu_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
SBU_HD uint32_t sbu_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
// the leaves of the pinned summation tree over a capacity: the smallest power of two >= n
static inline uint32_t sbb_pow2_at_least(uint32_t n) { uint32_t w = 1u; while (w < n) w <<= 1; return w; }
SBU_HD double sbu_canon(double sum) { return sum + 0.0; } // -0.0 -> +0.0, every other value as it is

// ---------------------------------------------------------------- leaves
SBU_HD bool sbu_particle_finite(sbu_float2 p, sbu_float2 v, sbu_float2 a)
{
    return sbb_finite(p.x) && sbb_finite(p.y) && sbb_finite(v.x) && sbb_finite(v.y) && sbb_finite(a.x) && sbb_finite(a.y);
}
// sbb_fkey of the position; v2 = vx^2 + vy^2 (exact products; never below +0.0, so its bits -- and its float's -- order as it does)
struct SbuParticleKeys { uint32_t x, y; double v2; };
SBU_HD SbuParticleKeys sbu_particle_keys(sbu_float2 p, sbu_float2 v)
{
    return SbuParticleKeys{sbb_fkey(p.x), sbb_fkey(p.y), (double)v.x * (double)v.x + (double)v.y * (double)v.y};
}
// the leaves of a finite particle: {px, py, vx, vy, 0.5 (vx^2 + vy^2)}, with N = 6 also x vy - y vx; and its keys
template <int N>
SBU_HD void sbu_particle_values(sbu_float2 p, sbu_float2 v, double (&out)[N], SbuParticleKeys &k)
{
    static_assert(N == 5 || N == 6, "five sums of a scene row, six of a body row");
    k = sbu_particle_keys(p, v);
    out[0] = (double)p.x, out[1] = (double)p.y, out[2] = (double)v.x, out[3] = (double)v.y, out[4] = 0.5 * k.v2;
    if constexpr (N == 6) out[5] = (double)p.x * (double)v.y - (double)p.y * (double)v.x;
}
// false: not finite, `out` and `k` are left as they were
template <int N>
SBU_HD bool sbu_particle_leaf(sbu_float2 p, sbu_float2 v, sbu_float2 a, double (&out)[N], SbuParticleKeys &k)
{
    if (!sbu_particle_finite(p, v, a)) return false;
    sbu_particle_values(p, v, out, k);
    return true;
}
// the leaf of a finite beam: its strain; its keys {strain, stress}
SBU_HD bool sbu_beam_leaf(float strain, float stress, double &out, uint32_t (&k)[2])
{
    if (!(sbb_finite(strain) && sbb_finite(stress))) return false;
    out = (double)strain, k[0] = sbb_fkey(strain), k[1] = sbb_fkey(stress);
    return true;
}

// what a thread of a scene row gathers beside its sums
struct SbuLocal {
    uint32_t p_fin = 0u, p_bad = 0u, b_fin = 0u, b_bad = 0u;
    uint32_t minx = SBB_KEY_MOST, miny = SBB_KEY_MOST, maxx = SBB_KEY_LEAST, maxy = SBB_KEY_LEAST;
    uint32_t max_strain = SBB_KEY_LEAST, max_stress = SBB_KEY_LEAST, min_stress = SBB_KEY_MOST;
    double max_v2 = 0.0;
};
// a particle / a live beam of the scene: its leaves (+0.0 where it is not finite) and its share of `l`
SBU_HD void sbu_local_particle(SbuLocal &l, sbu_float2 p, sbu_float2 v, sbu_float2 a, double (&out)[5])
{
    SbuParticleKeys k;
    if (!sbu_particle_leaf(p, v, a, out, k)) return (void)l.p_bad++;
    l.minx = sbu_min(l.minx, k.x), l.maxx = sbu_max(l.maxx, k.x), l.miny = sbu_min(l.miny, k.y), l.maxy = sbu_max(l.maxy, k.y);
    l.max_v2 = k.v2 > l.max_v2 ? k.v2 : l.max_v2;
    l.p_fin++;
}
SBU_HD void sbu_local_beam(SbuLocal &l, float strain, float stress, double (&out)[1])
{
    uint32_t k[2];
    if (!sbu_beam_leaf(strain, stress, out[0], k)) return (void)l.b_bad++;
    l.max_strain = sbu_max(l.max_strain, k[0]), l.max_stress = sbu_max(l.max_stress, k[1]), l.min_stress = sbu_min(l.min_stress, k[1]);
    l.b_fin++;
}

// ---------------------------------------------------------------- the pinned tree
// the stride-halving tree over K values e_j = leaf(base + j step), j < K: tree(e_0 .. e_K-1) = tree(even e) + tree(odd e)
template <int K, int N, class Leaf>
SBU_HD void sbu_tree(const Leaf &leaf, uint32_t base, uint32_t step, double (&out)[N])
{
    if constexpr (K == 1) {
        leaf(base, out);
    } else {
        double even[N], odd[N];
        sbu_tree<K / 2, N>(leaf, base, 2u * step, even);
        sbu_tree<K / 2, N>(leaf, base + step, 2u * step, odd);
        SBU_UNROLL
        for (int c = 0; c < N; c++) out[c] = even[c] + odd[c];
    }
}

// One level l of the sparse tree over sorted, unique keys: position q >= 1 adds onto the head of its left sibling
// block -- the first position >= lo (the caller's bound) of a key >= ((key >> l) - 1) << l, returned -- or adds nothing: SBU_NO_ADD.
#define SBU_NO_ADD 0xFFFFFFFFu
template <class Key>
SBU_HD uint32_t sbu_sparse_step(const Key *keys, uint32_t q, uint32_t l, uint32_t lo)
{
    const Key key = keys[q], prev = keys[q - 1u];
    if ((prev >> l) == (key >> l) || !((key >> l) & 1u) || (prev >> (l + 1u)) != (key >> (l + 1u))) return SBU_NO_ADD;
    const Key want = ((key >> l) - 1u) << l;
    uint32_t hi = q - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1; // (positions lie below 2^31, the capacity limit: the sum fits)
        if (keys[mid] < want) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

#if defined(__HIPCC__)
// levels h = 128 .. 1 of a tree whose upper levels left w <= 256 partials in s_col[0 .. w-1] (LDS; wave 0 calls it): two levels
// through LDS, then the xor butterfly -- lane i < h receives s[i] + s[i ^ h]; levels h >= w do not exist.  The sum is lane 0's.
__device__ __forceinline__ double sbu_tree_tail(const double *s_col, uint32_t lane, uint32_t w)
{
    double v = s_col[lane];
    if (w >= 256u) v = (v + s_col[lane + 128u]) + (s_col[lane + 64u] + s_col[lane + 192u]);
    else if (w == 128u) v = v + s_col[lane + 64u];
#pragma unroll
    for (uint32_t h = 32u; h != 0u; h >>= 1)
        if (h < w) v = v + __shfl_xor(v, (int)h);
    return v;
}
#endif

// ---------------------------------------------------------------- the row: words 6 .. 18 over np finite particles and nb finite beams
// (the other words differ between a scene row and a body row).  6 .. 9, 14: the means of x, y, vx, vy and the energy, from tot[0 .. 4]
template <class Count>
SBU_HD void sbu_row_sums(float *row, Count np, const double *tot)
{
    SBU_UNROLL
    for (int k = 0; k < 4; k++) row[6 + k] = np ? (float)(tot[k] / (double)np) : sbu_float(SBB_QNAN);
    row[14] = (float)tot[4]; // (round to nearest: +inf beyond the range of float)
}
// 10 .. 13, 15 .. 18: the extremes from their keys, NaN over an empty set (max_v2: rounding to float is monotonic)
struct SbuRowKeys { uint32_t minx, miny, maxx, maxy; float max_v2; uint32_t max_strain, max_stress, min_stress; };
template <class Count>
SBU_HD void sbu_row_extremes(float *row, Count np, Count nb, SbuRowKeys k)
{
    const float nan = sbu_float(SBB_QNAN);
    row[10] = np ? sbb_unkey(k.minx) : nan, row[11] = np ? sbb_unkey(k.miny) : nan;
    row[12] = np ? sbb_unkey(k.maxx) : nan, row[13] = np ? sbb_unkey(k.maxy) : nan;
    row[15] = np ? k.max_v2 : nan;
    row[16] = nb ? sbb_unkey(k.max_strain) : nan, row[17] = nb ? sbb_unkey(k.max_stress) : nan, row[18] = nb ? sbb_unkey(k.min_stress) : nan;
}

// word w of the body row behind the last group: counts, energy and angular momentum 0, the label -1, every other statistic NaN
SBU_HD float sbu_empty_body_word(uint32_t w) { return (w <= 1u || (w >= 3u && w <= 5u) || w == 14u || w >= 19u) ? 0.0f : (w == 2u ? -1.0f : sbu_float(SBB_QNAN)); }
