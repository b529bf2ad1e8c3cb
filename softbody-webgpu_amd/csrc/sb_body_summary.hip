// sb_body_summary.hip -- statistics per GROUP of particles (with sb_bodies_device's labels: per body) of the whole scene of an
// sb_engine, reproducible bit for bit, on the device (sb_body_summary / sb_body_summary_device of include/softbody.h; gfx950,
// wave64).
//
// The definition is sb_batch_body_summary_device's, word for word (both files call sb_summary_math.h), and so is its pin: the sum of a group is
// what sb_summary's tree gives for a scene holding only the group's finite particles -- double precision, leaf i = the value at
// DATA index i if the particle is finite and in the group, else +0.0, i = 0 .. W-1, reduced by  for h = W/2 .. 1: s[i] += s[i + h].
// k_batch_body_summary sorts a scene in the LDS of one workgroup; here the members lie in HBM, a scene holds a million bodies or
// one, and the call may only enqueue: nothing loops on a host read-back and no workgroup waits for another.  One launch a stage:
//   k_bsum_stage     a thread per t < Wn (Wn the smallest power of two >= the highest data index in use + 1): the data index
//                    d = bitrev(t), its group g (through the shared data index -> internal particle table, sb_report.hip; `none` where no
//                    particle lives or the label names no group), the key  g << 32 | bitrev32(d).  bitrev32(d) is r = bitrev(d)
//                    over log2 W bits, left-aligned: the order of  label * W + r, and t ascending IS r ascending
//   sort             a stable LSD radix sort of the keys by their label bits alone (the input is in r order, so that is the
//                    order by the whole key; the keys are unique): per pass k_bsum_hist (digit counts per block of SBY_SORT keys),
//                    an exclusive scan of the counts (sbq_scan, sb_report.hip), k_bsum_scatter (the rank of a key inside its block by wave ballots and a
//                    count per wave and round in LDS: the order comes from the keys' places alone, never from which atomic won)
//   k_bsum_leaves    a thread per sorted position: the six leaves of its particle (+0.0 for one that is not finite: such a leaf
//                    changes no partial sum but a zero's sign, and a zero sum is written as +0.0), its order-free particle words,
//                    the head flag of its label's run
//   k_bsum_level     the batch's sparse tree, one launch per level l: a position is a HEAD iff its predecessor differs in
//                    key >> l; a head with bit l set whose predecessor shares key >> (l + 1) adds its six partial sums -- and
//                    merges its particle words -- onto the head of its left sibling block (a lower-bound search over at most
//                    2^l positions).  Target and source are distinct, nothing is touched twice at a level, the launch boundary
//                    is the barrier.  Only levels at which a key can have its bit set are launched: log2 Wn of them
//   k_bsum_beams     a thread per caller beam slot: live, in a group (both endpoints), pending, finite, strain and stress keys;
//                    reduced per run of equal groups in a wave, then per workgroup for the group of its first slot, then one
//                    atomic per word on the row of the group's first sorted position
//   k_bsum_groups    behind an exclusive scan of the head flags: per group (label ascending) its first sorted position, its
//                    particles (the length of its run: an upper-bound search), its rank key; the group count, on the device
//   sort             the groups by ~particles with the same routine (stable: equal sizes stay label ascending), the number of
//                    keys read on the device
//   k_bsum_rank_of / k_bsum_rows / k_bsum_rank   the sorted place is the rank; rows, exact counts, the empty rows behind the last
//                    group; the rank of every data index
// Everything that reaches an output is either a double sum whose operands and order the keys fix, or an integer (count, minimum,
// maximum of ordered keys): no schedule can change a bit.  The file only READS the engine.
#include <algorithm>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "sb_report.h"
#include "sb_batch.h" // (sb_summary_math.h: the row's arithmetic, shared with the batch)

#define SBY_BLOCK 256u
#define SBY_WAVES (SBY_BLOCK / 64u)
#define SBY_PER 4u                        // keys (sort) / beam slots a thread owns
#define SBY_SORT (SBY_BLOCK * SBY_PER)    // keys of a sort block: 1024
#define SBY_RADIX_BITS 8u
#define SBY_RADIX 256u                    // = SBY_BLOCK: a thread per digit where the counts are scanned
#define SBY_GROUPS (SBY_PER * SBY_WAVES)  // (round, wave) pairs of a sort block, in key order
#define SBY_NSUM 6u                       // x, y, vx, vy, 0.5 (vx^2 + vy^2), x vy - y vx
#define SBY_NONE 0xFFFFFFFFu

static_assert(SBY_RADIX == SBY_BLOCK, "k_bsum_hist / k_bsum_scatter: one thread per digit");
static_assert(SBY_RADIX == SBQ_RADIX && SBY_SORT == SBQ_SORT, "what sb_report.h tells sbq_sort's callers about its buffers");

enum { SBY_P_BAD, SBY_P_MINX, SBY_P_MINY, SBY_P_MAXX, SBY_P_MAXY, SBY_P_MAXV2, SBY_NPST }; // particle words per sorted position
enum { SBY_B_LIVE, SBY_B_PENDING, SBY_B_BAD, SBY_B_MAXSTRAIN, SBY_B_MAXSTRESS, SBY_B_MINSTRESS, SBY_NBST }; // beam words per head
enum { SBY_C_HEADS, SBY_C_GROUPS, SBY_NCTL }; // device control words: runs of equal label (the `none` run included); groups

SB_DEV uint32_t sby_label(unsigned long long key) { return (uint32_t)(key >> 32); }
SB_DEV uint32_t sby_data_index(unsigned long long key) { return __brev((uint32_t)key); }

// the number of keys of a sort: the host's bound, or the device's word where that is smaller
SB_DEV uint32_t sby_count(uint32_t n_max, const uint32_t *__restrict__ n_dev) { return n_dev ? min(*n_dev, n_max) : n_max; }

// a thread per t < Wn
__global__ __launch_bounds__(SBY_BLOCK) void k_bsum_stage(const uint32_t *__restrict__ pinv, uint32_t np, const int32_t *__restrict__ labels,
                                                          uint32_t none, uint32_t Wn, uint32_t logWn, unsigned long long *keys)
{
    const uint32_t t = blockIdx.x * SBY_BLOCK + threadIdx.x;
    if (t >= Wn) return;
    const uint32_t r32 = logWn ? t << (32u - logWn) : 0u, d = __brev(r32);
    uint32_t g = none;
    if (d < np && pinv[d] != SBY_NONE) {
        const uint32_t lab = (uint32_t)labels[d]; // (a negative label is a large unsigned one)
        g = lab < none ? lab : none;
    }
    keys[t] = ((unsigned long long)g << 32) | r32;
}

// ---- the sort: digit (key >> shift) & mask, shift >= 32 (the label half)
// the valid lanes of the wave that hold this lane's digit, by one ballot per digit bit; every lane of the wave calls it
SB_DEV unsigned long long sby_same_digit(bool valid, uint32_t dig)
{
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < SBY_RADIX_BITS; b++) {
        const bool bit = (dig >> b) & 1u;
        const unsigned long long has = __ballot(bit);
        same &= bit ? has : ~has;
    }
    return same;
}

__global__ __launch_bounds__(SBY_BLOCK) void k_bsum_hist(const unsigned long long *__restrict__ keys, uint32_t n_max,
                                                         const uint32_t *__restrict__ n_dev, uint32_t shift, uint32_t mask,
                                                         uint32_t *hist, uint32_t nb)
{
    __shared__ uint32_t s_h[SBY_RADIX];
    const uint32_t tid = threadIdx.x, n = sby_count(n_max, n_dev);
    s_h[tid] = 0u;
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < SBY_PER; q++) {
        const uint64_t k = (uint64_t)blockIdx.x * SBY_SORT + q * SBY_BLOCK + tid;
        const bool valid = k < n;
        const uint32_t dig = valid ? (uint32_t)(keys[k] >> shift) & mask : 0u;
        const unsigned long long same = sby_same_digit(valid, dig);
        // one add per wave, round and digit, by the first lane that holds it: a scene that is one body has ONE digit in every pass,
        // and a lane an add would be 1024 adds on one LDS word (a count: the order of the adds is nothing)
        if (valid && (same & ((1ull << (tid & 63u)) - 1ull)) == 0ull) atomicAdd(&s_h[dig], (uint32_t)__popcll(same));
    }
    __syncthreads();
    hist[(size_t)tid * nb + blockIdx.x] = s_h[tid];
}

// base: the scanned counts, digit-major.  The place of a key: base of its digit and block + the keys of that digit in the (round,
// wave) pairs before its own + the lanes of its wave below it that hold the digit -- all from where the keys stand.
__global__ __launch_bounds__(SBY_BLOCK) void k_bsum_scatter(const unsigned long long *__restrict__ in, unsigned long long *__restrict__ out,
                                                            uint32_t n_max, const uint32_t *__restrict__ n_dev, uint32_t shift, uint32_t mask,
                                                            const uint32_t *__restrict__ base, uint32_t nb)
{
    __shared__ uint32_t s_cnt[SBY_GROUPS][SBY_RADIX];
    __shared__ uint32_t s_base[SBY_RADIX];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, n = sby_count(n_max, n_dev);
#pragma unroll
    for (uint32_t g = 0; g < SBY_GROUPS; g++) s_cnt[g][tid] = 0u;
    __syncthreads();
    unsigned long long key[SBY_PER];
    uint32_t below[SBY_PER];
#pragma unroll
    for (uint32_t q = 0; q < SBY_PER; q++) {
        const uint64_t k = (uint64_t)blockIdx.x * SBY_SORT + q * SBY_BLOCK + tid;
        const bool valid = k < n;
        key[q] = valid ? in[k] : 0ull;
        const uint32_t dig = (uint32_t)(key[q] >> shift) & mask;
        const unsigned long long same = sby_same_digit(valid, dig);
        const unsigned long long lower = same & ((1ull << lane) - 1ull);
        below[q] = (uint32_t)__popcll(lower);
        if (valid && lower == 0ull) s_cnt[q * SBY_WAVES + wave][dig] = (uint32_t)__popcll(same); // (one lane per digit, wave and round)
    }
    __syncthreads();
    uint32_t run = 0u;
#pragma unroll
    for (uint32_t g = 0; g < SBY_GROUPS; g++) {
        const uint32_t c = s_cnt[g][tid];
        s_cnt[g][tid] = run;
        run += c;
    }
    s_base[tid] = base[(size_t)tid * nb + blockIdx.x];
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < SBY_PER; q++) {
        const uint64_t k = (uint64_t)blockIdx.x * SBY_SORT + q * SBY_BLOCK + tid;
        if (k >= n) continue;
        const uint32_t dig = (uint32_t)(key[q] >> shift) & mask;
        const uint32_t at = s_base[dig] + s_cnt[q * SBY_WAVES + wave][dig] + below[q];
        if (at < n) out[at] = key[q]; // (always: the counts add up to n)
    }
}

// ---- a thread per sorted position: col [SBY_NSUM][Wn], pst [SBY_NPST][Wn], bst [SBY_NBST][Wn] (rows of heads only), flag [Wn]
__global__ __launch_bounds__(SBY_BLOCK) void k_bsum_leaves(const unsigned long long *__restrict__ keys, uint32_t Wn, uint32_t none,
                                                           const uint32_t *__restrict__ pinv, const float2 *__restrict__ pos,
                                                           const float2 *__restrict__ vel, const float2 *__restrict__ acc,
                                                           double *col, uint32_t *pst, uint32_t *bst, uint32_t *flag)
{
    const uint32_t q = blockIdx.x * SBY_BLOCK + threadIdx.x;
    if (q >= Wn) return;
    const unsigned long long key = keys[q];
    const uint32_t g = sby_label(key);
    const bool head = q == 0u || sby_label(keys[q - 1u]) != g;
    flag[q] = head ? 1u : 0u;
    if (g == none) return;
    const uint32_t i = pinv[sby_data_index(key)]; // (a member: a particle lives there)
    double leaf[SBY_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t st[SBY_NPST] = {1u, SBB_KEY_MOST, SBB_KEY_MOST, SBB_KEY_LEAST, SBB_KEY_LEAST, 0u};
    SbuParticleKeys pk;
    if (sbu_particle_leaf(pos[i], vel[i], acc[i], leaf, pk)) {
        st[SBY_P_BAD] = 0u;
        st[SBY_P_MINX] = st[SBY_P_MAXX] = pk.x;
        st[SBY_P_MINY] = st[SBY_P_MAXY] = pk.y;
        // (rounding to float is monotonic: the largest float is the float of the largest double; >= 0, so its bits order as it does)
        st[SBY_P_MAXV2] = __float_as_uint((float)pk.v2);
    }
#pragma unroll
    for (uint32_t k = 0; k < SBY_NSUM; k++) col[(size_t)k * Wn + q] = leaf[k];
#pragma unroll
    for (uint32_t k = 0; k < SBY_NPST; k++) pst[(size_t)k * Wn + q] = st[k];
    if (head) {
#pragma unroll
        for (uint32_t k = 0; k < SBY_NBST; k++) bst[(size_t)k * Wn + q] = k == SBY_B_MINSTRESS ? SBB_KEY_MOST : 0u;
    }
}

// level `bit` of the key (32 - log2 Wn .. 31); span = the most positions a sibling block holds at this level
__global__ __launch_bounds__(SBY_BLOCK) void k_bsum_level(const unsigned long long *__restrict__ keys, uint32_t Wn, uint32_t none, uint32_t bit,
                                                          uint32_t span, double *col, uint32_t *pst)
{
    const uint32_t q = blockIdx.x * SBY_BLOCK + threadIdx.x;
    if (q == 0u || q >= Wn) return; // (position 0 never adds)
    if (sby_label(keys[q]) == none) return;
    const uint32_t lo = sbu_sparse_step(keys, q, bit, q > span ? q - span : 0u); // (the sibling block holds at most span keys)
    if (lo == SBU_NO_ADD) return;
#pragma unroll
    for (uint32_t k = 0; k < SBY_NSUM; k++) col[(size_t)k * Wn + lo] = col[(size_t)k * Wn + lo] + col[(size_t)k * Wn + q];
    pst[(size_t)SBY_P_BAD * Wn + lo] += pst[(size_t)SBY_P_BAD * Wn + q];
#pragma unroll
    for (uint32_t k = SBY_P_MINX; k <= SBY_P_MINY; k++) pst[(size_t)k * Wn + lo] = min(pst[(size_t)k * Wn + lo], pst[(size_t)k * Wn + q]);
#pragma unroll
    for (uint32_t k = SBY_P_MAXX; k <= SBY_P_MAXV2; k++) pst[(size_t)k * Wn + lo] = max(pst[(size_t)k * Wn + lo], pst[(size_t)k * Wn + q]);
}

// the first sorted position of label g (Wn: none)
SB_DEV uint32_t sby_head_of(const unsigned long long *__restrict__ keys, uint32_t Wn, uint32_t g)
{
    const unsigned long long want = (unsigned long long)g << 32;
    uint32_t lo = 0u, hi = Wn;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < want) lo = mid + 1u;
        else hi = mid;
    }
    return lo < Wn && sby_label(keys[lo]) == g ? lo : Wn;
}

SB_DEV void sby_beam_merge(uint32_t (&v)[SBY_NBST], const uint32_t (&o)[SBY_NBST])
{
    v[SBY_B_LIVE] += o[SBY_B_LIVE], v[SBY_B_PENDING] += o[SBY_B_PENDING], v[SBY_B_BAD] += o[SBY_B_BAD];
    v[SBY_B_MAXSTRAIN] = max(v[SBY_B_MAXSTRAIN], o[SBY_B_MAXSTRAIN]);
    v[SBY_B_MAXSTRESS] = max(v[SBY_B_MAXSTRESS], o[SBY_B_MAXSTRESS]);
    v[SBY_B_MINSTRESS] = min(v[SBY_B_MINSTRESS], o[SBY_B_MINSTRESS]);
}

template <class T>
SB_DEV void sby_beam_push(T *row, size_t stride, const uint32_t (&v)[SBY_NBST])
{
    if (v[SBY_B_LIVE]) atomicAdd(&row[SBY_B_LIVE * stride], v[SBY_B_LIVE]);
    if (v[SBY_B_PENDING]) atomicAdd(&row[SBY_B_PENDING * stride], v[SBY_B_PENDING]);
    if (v[SBY_B_BAD]) atomicAdd(&row[SBY_B_BAD * stride], v[SBY_B_BAD]);
    if (v[SBY_B_MAXSTRAIN]) atomicMax(&row[SBY_B_MAXSTRAIN * stride], v[SBY_B_MAXSTRAIN]);
    if (v[SBY_B_MAXSTRESS]) atomicMax(&row[SBY_B_MAXSTRESS * stride], v[SBY_B_MAXSTRESS]);
    if (v[SBY_B_MINSTRESS] != SBB_KEY_MOST) atomicMin(&row[SBY_B_MINSTRESS * stride], v[SBY_B_MINSTRESS]);
}

// tab: [4][n] = data index of A, data index of B, engine slot, the copy read back for it, per caller beam slot.  A workgroup owns
// SBY_PER * SBY_BLOCK slots.  A beam of group g goes, with the lanes of its run of equal groups in the wave, into LDS where g is
// the group of the workgroup's first slot, else onto g's row at once; the LDS words onto that group's row at the end.
__global__ __launch_bounds__(SBY_BLOCK) void k_bsum_beams(const uint32_t *__restrict__ tab, uint32_t n, const uint32_t *__restrict__ dead,
                                                          const uint32_t *__restrict__ broken, const float *__restrict__ strain,
                                                          const float *__restrict__ stress, const int32_t *__restrict__ labels, uint32_t none,
                                                          const unsigned long long *__restrict__ keys, uint32_t Wn, uint32_t *bst)
{
    __shared__ uint32_t s_acc[SBY_NBST];
    __shared__ uint32_t s_first;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < SBY_NBST) s_acc[tid] = tid == SBY_B_MINSTRESS ? SBB_KEY_MOST : 0u;
    if (tid == 0u) { // the group of the A end of the first slot, whether or not that beam counts
        const uint32_t u0 = blockIdx.x * (SBY_PER * SBY_BLOCK);
        const uint32_t lab = u0 < n ? (uint32_t)labels[tab[u0]] : none;
        s_first = lab < none ? lab : none;
    }
    __syncthreads();
    const uint32_t first = s_first;
    for (uint32_t j = 0; j < SBY_PER; j++) { // (uniform)
        const uint32_t u = blockIdx.x * (SBY_PER * SBY_BLOCK) + j * SBY_BLOCK + tid;
        uint32_t g = none;
        uint32_t v[SBY_NBST] = {0u, 0u, 0u, SBB_KEY_LEAST, SBB_KEY_LEAST, SBB_KEY_MOST};
        if (u < n && !(dead && dead[tab[2u * (size_t)n + u]] != 0u)) {
            const uint32_t la = (uint32_t)labels[tab[u]], lb = (uint32_t)labels[tab[(size_t)n + u]];
            if (la < none && la == lb) {
                g = la;
                const uint32_t c = tab[3u * (size_t)n + u];
                v[SBY_B_LIVE] = 1u;
                v[SBY_B_PENDING] = (broken[c >> 5] >> (c & 31u)) & 1u;
                double leaf;
                uint32_t bk[2];
                if (sbu_beam_leaf(strain[c], stress[c], leaf, bk)) {
                    v[SBY_B_MAXSTRAIN] = bk[0];
                    v[SBY_B_MAXSTRESS] = v[SBY_B_MINSTRESS] = bk[1];
                } else v[SBY_B_BAD] = 1u;
            }
        }
        // the runs of equal groups in the wave: a lane takes in the lanes of its run above it, doubling
        const uint32_t left = __shfl_up(g, 1);
        const bool head = lane == 0u || left != g;
        const unsigned long long heads = __ballot(head);
        const unsigned long long upto = heads & (lane == 63u ? ~0ull : (1ull << (lane + 1u)) - 1ull);
        const uint32_t run = 63u - (uint32_t)__clzll((long long)upto); // the lane my run starts at
#pragma unroll
        for (uint32_t off = 1u; off < 64u; off <<= 1) {
            uint32_t o[SBY_NBST];
#pragma unroll
            for (uint32_t k = 0; k < SBY_NBST; k++) o[k] = __shfl_down(v[k], off);
            const uint32_t orun = __shfl_down(run, off);
            if (lane + off < 64u && orun == run) sby_beam_merge(v, o);
        }
        if (head && g != none && v[SBY_B_LIVE]) {
            if (g == first) sby_beam_push(s_acc, 1, v);
            else {
                const uint32_t h = sby_head_of(keys, Wn, g);
                if (h < Wn) sby_beam_push(bst + h, Wn, v);
            }
        }
    }
    __syncthreads();
    if (tid == 0u && s_acc[SBY_B_LIVE]) {
        const uint32_t h = sby_head_of(keys, Wn, first);
        if (h < Wn) {
            uint32_t v[SBY_NBST];
#pragma unroll
            for (uint32_t k = 0; k < SBY_NBST; k++) v[k] = s_acc[k];
            sby_beam_push(bst + h, Wn, v);
        }
    }
}

// ord: the exclusive scan of the head flags; ctl[SBY_C_HEADS] its total.  Per group j (label ascending): its first sorted
// position, its particles, its rank key  (~particles & cmask) << 32 | j
__global__ __launch_bounds__(SBY_BLOCK) void k_bsum_groups(const unsigned long long *__restrict__ keys, uint32_t Wn, uint32_t none,
                                                           const uint32_t *__restrict__ ord, uint32_t cmask, uint32_t *ghead, uint32_t *gcnt,
                                                           unsigned long long *rkeys, uint32_t *ctl)
{
    const uint32_t q = blockIdx.x * SBY_BLOCK + threadIdx.x;
    if (q >= Wn) return;
    if (q == 0u) ctl[SBY_C_GROUPS] = ctl[SBY_C_HEADS] - (sby_label(keys[Wn - 1u]) == none ? 1u : 0u);
    const uint32_t g = sby_label(keys[q]);
    if (g == none || (q != 0u && sby_label(keys[q - 1u]) == g)) return;
    const unsigned long long want = (unsigned long long)(g + 1u) << 32; // (g < none <= 2^31)
    uint32_t lo = q + 1u, hi = Wn;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < want) lo = mid + 1u;
        else hi = mid;
    }
    const uint32_t j = ord[q], cnt = lo - q;
    ghead[j] = q;
    gcnt[j] = cnt;
    rkeys[j] = ((unsigned long long)(~cnt & cmask) << 32) | j;
}

__global__ __launch_bounds__(SBY_BLOCK) void k_bsum_rank_of(const unsigned long long *__restrict__ sorted, uint32_t Wn,
                                                            const uint32_t *__restrict__ ctl, uint32_t *rank_of)
{
    const uint32_t k = blockIdx.x * SBY_BLOCK + threadIdx.x;
    if (k < min(ctl[SBY_C_GROUPS], Wn)) rank_of[(uint32_t)sorted[k]] = k;
}

// a thread per row
__global__ __launch_bounds__(SBY_BLOCK) void k_bsum_rows(const unsigned long long *__restrict__ sorted, uint32_t Wn, const uint32_t *__restrict__ ctl,
                                                         const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ ghead,
                                                         const uint32_t *__restrict__ gcnt, const double *__restrict__ col,
                                                         const uint32_t *__restrict__ pst, const uint32_t *__restrict__ bst,
                                                         uint64_t max_rows, float *rows, long long *rows64)
{
    const uint64_t k = (uint64_t)blockIdx.x * SBY_BLOCK + threadIdx.x;
    if (k >= max_rows) return;
    float row[SB_BODY_SUMMARY_WORDS];
    long long c8[SB_BODY_SUMMARY_COUNT_WORDS] = {0, 0, -1, 0, 0, 0, 0, 0};
    if (k >= min(ctl[SBY_C_GROUPS], Wn)) { // behind the last group: the empty row
#pragma unroll
        for (uint32_t w = 0; w < SB_BODY_SUMMARY_WORDS; w++)
            row[w] = sbu_empty_body_word(w);
    } else {
        const uint32_t j = (uint32_t)sorted[k], h = ghead[j], cnt = gcnt[j];
        uint32_t p[SBY_NPST], b[SBY_NBST];
#pragma unroll
        for (uint32_t w = 0; w < SBY_NPST; w++) p[w] = pst[(size_t)w * Wn + h];
#pragma unroll
        for (uint32_t w = 0; w < SBY_NBST; w++) b[w] = bst[(size_t)w * Wn + h];
        const uint32_t np = cnt - p[SBY_P_BAD], nb = b[SBY_B_LIVE] - b[SBY_B_BAD];
        c8[0] = cnt, c8[1] = b[SBY_B_LIVE], c8[2] = sby_label(keys[h]), c8[3] = b[SBY_B_PENDING], c8[4] = p[SBY_P_BAD], c8[5] = b[SBY_B_BAD];
        c8[6] = np;
#pragma unroll
        for (uint32_t w = 0; w < 6u; w++) row[w] = (float)c8[w];
        double tot[SBY_NSUM]; // (a zero sum as +0.0)
#pragma unroll
        for (uint32_t w = 0; w < SBY_NSUM; w++) tot[w] = sbu_canon(col[(size_t)w * Wn + h]);
        sbu_row_sums(row, np, tot);
        sbu_row_extremes(row, np, nb, SbuRowKeys{p[SBY_P_MINX], p[SBY_P_MINY], p[SBY_P_MAXX], p[SBY_P_MAXY], __uint_as_float(p[SBY_P_MAXV2]),
                                                 b[SBY_B_MAXSTRAIN], b[SBY_B_MAXSTRESS], b[SBY_B_MINSTRESS]});
        row[19] = (float)tot[5];
        row[20] = row[21] = row[22] = row[23] = 0.0f;
    }
    if (rows) {
#pragma unroll
        for (uint32_t w = 0; w < SB_BODY_SUMMARY_WORDS; w++) rows[k * SB_BODY_SUMMARY_WORDS + w] = row[w];
    }
    if (rows64) {
#pragma unroll
        for (uint32_t w = 0; w < SB_BODY_SUMMARY_COUNT_WORDS; w++) rows64[k * SB_BODY_SUMMARY_COUNT_WORDS + w] = c8[w];
    }
}

// grid over max(Wn, maxP): the rank at the data index of every sorted position; -1 at every other index below maxP
__global__ __launch_bounds__(SBY_BLOCK) void k_bsum_rank(const unsigned long long *__restrict__ keys, uint32_t Wn, uint32_t none,
                                                         const uint32_t *__restrict__ ord, const uint32_t *__restrict__ rank_of,
                                                         uint32_t maxP, int32_t *rank)
{
    const uint32_t t = blockIdx.x * SBY_BLOCK + threadIdx.x;
    if (t >= Wn) {
        if (t < maxP) rank[t] = -1;
        return;
    }
    const unsigned long long key = keys[t];
    const uint32_t g = sby_label(key), d = sby_data_index(key);
    if (d >= maxP) return;
    if (g == none) {
        rank[d] = -1;
        return;
    }
    const bool head = t == 0u || sby_label(keys[t - 1u]) != g;
    rank[d] = (int32_t)rank_of[ord[t] - (head ? 0u : 1u)];
}

// ---------------------------------------------------------------- host side

static uint32_t sby_bits(uint64_t most) // bits that hold every value 0 .. most
{
    uint32_t b = 1u;
    while (b < 64u && (most >> b) != 0u) b++;
    return b;
}

static uint32_t sby_blocks(uint64_t k, uint32_t per) { return (uint32_t)((k + per - 1u) / per); }

// Stable sort of at most n_max keys (the number on the device where n_dev is given) by their bits 32 .. 32 + bits - 1, between
// the buffers a and b; returns the one that holds the result.  hist: SBY_RADIX words per sort block; bsum: a word per scan block.
// (sbq_sort of sb_report.h: sb_graph.hip orders its half-edges with the same launches)
unsigned long long *sbq_sort(sb_engine *e, unsigned long long *a, unsigned long long *b, uint32_t n_max, const uint32_t *n_dev, uint32_t bits,
                             uint32_t *hist, uint32_t *bsum)
{
    const uint32_t nb = sby_blocks(n_max, SBY_SORT), passes = (bits + SBY_RADIX_BITS - 1u) / SBY_RADIX_BITS;
    const uint32_t per = (bits + passes - 1u) / passes; // digits of equal width: 21 bits are three passes of 7
    for (uint32_t p = 0, at = 0; p < passes; p++, at += per) {
        const uint32_t width = std::min(per, bits - at), shift = 32u + at, mask = (1u << width) - 1u;
        k_bsum_hist<<<nb, SBY_BLOCK, 0, e->stream>>>(a, n_max, n_dev, shift, mask, hist, nb);
        sbq_scan<uint32_t>(e, hist, (uint64_t)SBY_RADIX * nb, bsum, hist, nullptr);
        k_bsum_scatter<<<nb, SBY_BLOCK, 0, e->stream>>>(a, b, n_max, n_dev, shift, mask, hist, nb);
        std::swap(a, b);
    }
    return a;
}

std::vector<const void *> sbq_sort_kernels() { return {(const void *)k_bsum_hist, (const void *)k_bsum_scatter}; }

// the call's scratch, carved out of one allocation: bytes per position of Wn (sb_get_info "body_summary_scratch_bytes")
struct SbyCarve {
    size_t at = 0;
    size_t take(size_t bytes)
    {
        const size_t o = at;
        at += (bytes + 255u) & ~(size_t)255u;
        return o;
    }
};

static sb_status sby_enqueue(sb_engine *e, const sb_body_summary_options *o, const void *labels, void *rows, void *rows64, void *rank, bool host)
{
    if (!e) return SB_ERR_INVALID;
    const char *what = host ? "sb_body_summary" : "sb_body_summary_device";
    const bool given = o && o->struct_size == sizeof(sb_body_summary_options);
    const uint32_t maxP = e->opt.max_particles;
    const uint64_t max_rows = given ? o->max_rows : std::min<uint64_t>(SB_BODY_SUMMARY_DEFAULT_ROWS, maxP);
    if (!rows && !rows64 && !rank) SB_FAIL(e, SB_ERR_INVALID, "%s: no output asked for", what);
    if (max_rows == 0 || max_rows > maxP)
        SB_FAIL(e, SB_ERR_INVALID, "%s: max_rows %llu is not in 1 .. max_particles (%u)", what, (unsigned long long)max_rows, maxP);
    if (((uintptr_t)labels & 3u) || ((uintptr_t)rows & 3u) || ((uintptr_t)rank & 3u))
        SB_FAIL(e, SB_ERR_INVALID, "%s: labels, rows and rank must be 4-byte aligned", what);
    if ((uintptr_t)rows64 & 7u) SB_FAIL(e, SB_ERR_INVALID, "%s: rows_i64 must be 8-byte aligned", what);
    SB_TRY(sbq_preflight(e, what, o, "handled", "bodies across ranks are not handled"));
    SB_TRY(sbq_need(e, "sb_body_summary", SBQ_PARTICLES | SBQ_BEAMS | SBQ_COPIES));
    SbStateIoState &s = *e->sio;
    s.bsm_build_ms = s.part_ms + s.beam_ms + s.copy_ms;

    const uint32_t np = s.np, n = s.nslots, Wn = sbb_pow2_at_least(std::max(np, 1u));
    uint32_t logWn = 0u;
    while ((1u << logWn) < Wn) logWn++;
    // the word of "no group" in a key: above every label that names a group (the engine's own labels are data indices in use)
    const uint32_t none = labels ? maxP : std::max(np, 1u);
    const uint32_t nb_sort = sby_blocks(Wn, SBY_SORT);
    const uint64_t hist_words = (uint64_t)SBY_RADIX * nb_sort;

    SbyCarve cv;
    const size_t o_keys_a = cv.take((size_t)Wn * 8), o_keys_b = cv.take((size_t)Wn * 8), o_rkeys = cv.take((size_t)Wn * 8);
    const size_t o_col = cv.take((size_t)Wn * 8 * SBY_NSUM), o_pst = cv.take((size_t)Wn * 4 * SBY_NPST), o_bst = cv.take((size_t)Wn * 4 * SBY_NBST);
    const size_t o_ord = cv.take((size_t)Wn * 4), o_ghead = cv.take((size_t)Wn * 4), o_gcnt = cv.take((size_t)Wn * 4), o_rank_of = cv.take((size_t)Wn * 4);
    const size_t o_hist = cv.take((size_t)hist_words * 4), o_bsum = cv.take((size_t)sby_blocks(std::max<uint64_t>(hist_words, Wn), SBQ_SCAN) * 4);
    const size_t o_ctl = cv.take(SBY_NCTL * 4);
    SB_TRY(s.buf[SBY_B_SCRATCH].grow(e, cv.at));
    char *m = s.buf[SBY_B_SCRATCH].as<char>();
    unsigned long long *keys_a = (unsigned long long *)(m + o_keys_a), *keys_b = (unsigned long long *)(m + o_keys_b);
    unsigned long long *rkeys = (unsigned long long *)(m + o_rkeys);
    double *col = (double *)(m + o_col);
    uint32_t *pst = (uint32_t *)(m + o_pst), *bst = (uint32_t *)(m + o_bst), *ord = (uint32_t *)(m + o_ord), *ghead = (uint32_t *)(m + o_ghead);
    uint32_t *gcnt = (uint32_t *)(m + o_gcnt), *rank_of = (uint32_t *)(m + o_rank_of), *hist = (uint32_t *)(m + o_hist);
    uint32_t *bsum = (uint32_t *)(m + o_bsum), *ctl = (uint32_t *)(m + o_ctl);

    // where the launches read and write: the caller's device memory, or (sb_body_summary) the engine's own, copied below
    // (the outputs of sb_body_summary lie in one block, SBY_B_OUT: "body_summary_scratch_bytes" counts it)
    const size_t b_labels = (size_t)maxP * sizeof(int32_t), b_rows = (size_t)max_rows * SB_BODY_SUMMARY_WORDS * sizeof(float),
                 b_rows64 = (size_t)max_rows * SB_BODY_SUMMARY_COUNT_WORDS * sizeof(int64_t), b_rank = (size_t)maxP * sizeof(int32_t);
    SbqMirror mir(e, host);
    const int32_t *d_labels = mir.in<int32_t>(SBY_B_LABELS, labels, b_labels, b_labels);
    SbyCarve out;
    const size_t o_r64 = out.take(rows64 ? b_rows64 : 0), o_r = out.take(rows ? b_rows : 0), o_k = out.take(rank ? b_rank : 0);
    if (host) SB_TRY(s.buf[SBY_B_OUT].grow(e, out.at));
    void *w = s.buf[SBY_B_OUT].p;
    long long *d_rows64 = mir.out_at<long long>(rows64, w, o_r64, b_rows64);
    float *d_rows = mir.out_at<float>(rows, w, o_r, b_rows);
    int32_t *d_rank = mir.out_at<int32_t>(rank, w, o_k, b_rank);
    SB_TRY(mir.st);
    if (!labels) { // the engine's own bodies: sb_bodies_device's labelling, on the same stream, nothing waits
        SB_TRY(s.buf[SBY_B_LABELS].grow(e, b_labels));
        const sb_status st = sb_bodies_device(e, nullptr, s.buf[SBY_B_LABELS].p, nullptr, nullptr);
        if (st != SB_OK) return st;
        d_labels = s.buf[SBY_B_LABELS].as<int32_t>();
    }

    const SbParticleArrays &c = e->part[e->cur];
    const uint32_t *dead = sbq_dead(e);
    const uint32_t *pinv = s.buf[SBQ_B_PINV].as<uint32_t>(), *tab = s.buf[SBQ_B_TAB].as<uint32_t>();
    const uint32_t grid_w = sby_blocks(Wn, SBY_BLOCK);

    k_bsum_stage<<<grid_w, SBY_BLOCK, 0, e->stream>>>(pinv, np, d_labels, none, Wn, logWn, keys_a);
    unsigned long long *keys = sbq_sort(e, keys_a, keys_b, Wn, nullptr, sby_bits(none), hist, bsum);
    unsigned long long *spare = keys == keys_a ? keys_b : keys_a;
    k_bsum_leaves<<<grid_w, SBY_BLOCK, 0, e->stream>>>(keys, Wn, none, pinv, c.pos, c.vel, c.acc, col, pst, bst, ord);
    for (uint32_t l = 0; l < logWn; l++) // (no key has a bit below 32 - log2 Wn set: those levels add nothing)
        k_bsum_level<<<grid_w, SBY_BLOCK, 0, e->stream>>>(keys, Wn, none, 32u - logWn + l, 1u << l, col, pst);
    if (n)
        k_bsum_beams<<<sby_blocks(n, SBY_PER * SBY_BLOCK), SBY_BLOCK, 0, e->stream>>>(tab, n, dead, e->d_broken, e->beams.strain, e->beams.stress,
                                                                                      d_labels, none, keys, Wn, bst);
    sbq_scan<uint32_t>(e, ord, Wn, bsum, ord, ctl + SBY_C_HEADS);
    const uint32_t cbits = logWn + 1u, cmask = (uint32_t)((1ull << cbits) - 1ull); // a group holds at most Wn particles
    k_bsum_groups<<<grid_w, SBY_BLOCK, 0, e->stream>>>(keys, Wn, none, ord, cmask, ghead, gcnt, rkeys, ctl);
    const unsigned long long *sorted = sbq_sort(e, rkeys, spare, Wn, ctl + SBY_C_GROUPS, cbits, hist, bsum);
    if (rows || rows64)
        k_bsum_rows<<<sby_blocks(max_rows, SBY_BLOCK), SBY_BLOCK, 0, e->stream>>>(sorted, Wn, ctl, keys, ghead, gcnt, col, pst, bst, max_rows,
                                                                                 d_rows, d_rows64);
    if (rank) {
        k_bsum_rank_of<<<grid_w, SBY_BLOCK, 0, e->stream>>>(sorted, Wn, ctl, rank_of);
        k_bsum_rank<<<sby_blocks(std::max(Wn, maxP), SBY_BLOCK), SBY_BLOCK, 0, e->stream>>>(keys, Wn, none, ord, rank_of, maxP, d_rank);
    }
    SB_HIP(e, hipGetLastError());
    return mir.finish();
}

// what sb_get_info reads ("body_summary_table_build_us", "body_summary_scratch_bytes", "body_summary_kernel_vgprs",
// "body_summary_kernel_scratch_bytes")
bool sby_info(sb_engine *e, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "body_summary_table_build_us") *value = e->sio ? (uint64_t)(e->sio->bsm_build_ms * 1000.0 + 0.5) : 0u;
    else if (k == "body_summary_scratch_bytes") { // everything its calls so far hold on the device: scratch, labels, the two tables they read, sb_body_summary's result
        const SbStateIoState *s = e->sio;
        *value = s && s->buf[SBY_B_SCRATCH].cap ? (uint64_t)(s->buf[SBY_B_SCRATCH].cap + s->buf[SBY_B_LABELS].cap + s->buf[SBQ_B_PINV].cap + s->buf[SBQ_B_TAB].cap + s->buf[SBY_B_OUT].cap) : 0u;
    }
    else if (k == "body_summary_kernel_vgprs" || k == "body_summary_kernel_scratch_bytes") { // the most over every kernel a call may launch
        std::vector<const void *> ks = {(const void *)k_bsum_stage, (const void *)k_bsum_hist, (const void *)k_bsum_scatter, (const void *)k_bsum_leaves,
                                        (const void *)k_bsum_level, (const void *)k_bsum_beams, (const void *)k_bsum_groups, (const void *)k_bsum_rank_of,
                                        (const void *)k_bsum_rows, (const void *)k_bsum_rank};
        for (const void *f : sbq_scan_kernels(false)) ks.push_back(f); // (32-bit words only)
        return sbq_kernel_most(e, ks, k == "body_summary_kernel_vgprs", value);
    }
    else return false;
    return true;
}

extern "C" {

sb_status sb_body_summary_device(sb_engine *e, const sb_body_summary_options *opts, const void *device_labels_i32, void *device_rows_f32,
                                 void *device_rows_i64, void *device_rank_i32)
{
    SB_GUARDED(e, sby_enqueue(e, opts, device_labels_i32, device_rows_f32, device_rows_i64, device_rank_i32, false))
}

sb_status sb_body_summary(sb_engine *e, const sb_body_summary_options *opts, const int32_t *labels, float *rows, int64_t *rows_i64, int32_t *rank)
{
    SB_GUARDED(e, sby_enqueue(e, opts, labels, rows, rows_i64, rank, true))
}

} // extern "C"
