// sb_batch_body_summary.hip -- statistics per GROUP of particles (with sb_batch_bodies_device's labels: per body) of every scene
// of a batch in ONE launch, reproducible bit for bit (gfx950, wave64).
//
// One workgroup per scene reads the caller's labels, the scene's metadata words, its constant blob and its state blob; nothing is
// written but the rows and the ranks.
//
// The sums are PINNED to sb_batch_summary_device's tree (sb_summary_math.h): the sum of a group is what that tree gives for a scene holding only the
// group's finite particles -- double precision, leaf i = the value at DATA index i if particle i is finite and in the group, else
// +0.0, i = 0 .. W-1, reduced by  for h = W/2 .. 1: s[i] += s[i + h].  That tree is never evaluated per group.  Every partial sum
// is finite (at most 1024 finite floats, in double), so the +0.0 of an absent leaf changes no partial sum but a zero's sign, and
// the masked tree is a tree over the members alone.  With r = bitrev(i) over log2 W bits the stride-halving tree is the
// ADJACENT-PAIR tree in r order (level l adds the block whose r has bit l set onto its left sibling), so
//   sort     the finite members of all groups by the key  label * W + r  (unique; a bitonic network over W keys in LDS: the order
//            comes from the keys alone, never from which atomic won)
//   reduce   log2 W levels, one barrier each: at level l a sorted position is the HEAD of its block iff its predecessor's key
//            differs in key >> l; a head whose key has bit l set and whose predecessor shares key >> (l + 1) adds its six partial
//            sums onto the head of the left sibling block (the lower bound of ((key >> l) - 1) << l).  Nobody else touches either
//            operand at that level; after the last level a group's sums sit at the first sorted position of its label.
// All groups are reduced at once.  A sum that is zero is written as +0.0 (sbu_canon): the masked tree gives that in every case but
// a group that fills all W leaves with -0.0.
// Everything else in a row (counts, extremes) is order-free and goes through LDS atomics on integer keys; the ranking sorts the
// keys  particles << 10 | (1023 - label)  with the same network.
#include <algorithm>
#include <string>

#include "sb_batch_group_sort.h" // SBQ_BLOCK, sbq_sort, the rank key

#define SBQ_NSUM 6u // x, y, vx, vy, 0.5 (vx^2 + vy^2), x vy - y vx

// per-label statistics words, each an array of max_particles entries
enum {
    SBQ_NP,      // particles | particles that are not finite << 16
    SBQ_NB,      // live beams | live beams that are not finite << 16
    SBQ_PENDING, // break flags pending among the group's live beam slots
    SBQ_MINX, SBQ_MINY, SBQ_MAXX, SBQ_MAXY, SBQ_MAX_V2, SBQ_MAX_STRAIN, SBQ_MAX_STRESS, SBQ_MIN_STRESS, SBQ_NSTAT
};

// LDS of a workgroup: double col[SBQ_NSUM][W]; uint32 key[W], rkey[W], grp[maxP], rank[maxP], stat[SBQ_NSTAT][maxP]
static inline uint32_t sbq_lds_bytes(uint32_t maxP)
{
    const uint32_t W = sbb_pow2_at_least(maxP);
    return W * (SBQ_NSUM * 8u + 2u * 4u) + maxP * (2u + SBQ_NSTAT) * 4u;
}

__global__ __launch_bounds__(SBQ_BLOCK) void k_batch_body_summary(SbBatchView V, const int32_t *__restrict__ labels, uint32_t max_rows,
                                                                  float *__restrict__ rows, int32_t *__restrict__ rank, uint32_t W, uint32_t logW)
{
    extern __shared__ __attribute__((aligned(16))) double sbq_lds[];
    const uint32_t scene = blockIdx.x, tid = threadIdx.x;
    if (scene >= V.n_scenes) return;
    const uint32_t maxP = V.maxP;
    double *s_col = sbq_lds;                      // [SBQ_NSUM][W] partial sums at sorted positions
    uint32_t *s_key = (uint32_t *)(s_col + SBQ_NSUM * W); // [W] label * W + bitrev(data index) of the finite members, SBQ_NONE behind them
    uint32_t *s_rkey = s_key + W;                 // [W] ~(particles << 10 | (1023 - label)) of the non-empty groups, SBQ_NONE behind them
    uint32_t *s_grp = s_rkey + W;                 // [maxP] per DATA index: its group, SBQ_NONE where there is none
    uint32_t *s_rank = s_grp + maxP;              // [maxP] per label: its rank
    uint32_t *s_stat = s_rank + maxP;             // [SBQ_NSTAT][maxP] per label

    const SbbScene hd = sbb_scene(V, scene);
    const uint32_t P = hd.P, Bc = hd.Bc;
    const unsigned char *cst = hd.cst, *st = hd.st;
    const uint32_t *g_pmap = (const uint32_t *)(cst + V.o_pmap), *g_bword = (const uint32_t *)(cst + V.o_bword);
    const uint32_t *g_bmap = (const uint32_t *)(st + V.o_bmap), *g_flags = (const uint32_t *)(st + V.o_bflags);
    const float2 *g_part = (const float2 *)(st + V.o_part);
    const float4 *g_bstate = (const float4 *)(st + V.o_bstate);
    const int32_t *lrow = labels + (size_t)scene * maxP;

    // ---- clear
    for (uint32_t q = tid; q < W; q += SBQ_BLOCK) s_key[q] = SBQ_NONE;
    for (uint32_t d = tid; d < maxP; d += SBQ_BLOCK) {
        s_grp[d] = SBQ_NONE;
#pragma unroll
        for (uint32_t k = 0; k < SBQ_NSTAT; k++)
            s_stat[k * maxP + d] = (k == SBQ_MINX || k == SBQ_MINY || k == SBQ_MIN_STRESS) ? SBB_KEY_MOST : 0u;
    }
    __syncthreads();

    // ---- particles (an upload is refused unless its data indices are distinct and inside the capacity): group, counts, extremes,
    // and the sort key of a finite member, parked at its data index
    for (uint32_t s = tid; s < P; s += SBQ_BLOCK) {
        const uint32_t d = g_pmap[s];
        const uint32_t g = (uint32_t)lrow[d]; // (a negative label is a large unsigned one)
        if (g >= maxP) continue;
        s_grp[d] = g;
        const float2 p = g_part[3u * d], v = g_part[3u * d + 1u];
        if (!sbu_particle_finite(p, v, g_part[3u * d + 2u])) {
            atomicAdd(&s_stat[SBQ_NP * maxP + g], 0x10001u);
            continue;
        }
        const SbuParticleKeys k = sbu_particle_keys(p, v); // (the leaves are taken once the members are sorted)
        atomicAdd(&s_stat[SBQ_NP * maxP + g], 1u);
        atomicMin(&s_stat[SBQ_MINX * maxP + g], k.x);
        atomicMin(&s_stat[SBQ_MINY * maxP + g], k.y);
        atomicMax(&s_stat[SBQ_MAXX * maxP + g], k.x);
        atomicMax(&s_stat[SBQ_MAXY * maxP + g], k.y);
        // (rounding to float is monotonic: the largest float is the float of the largest double; >= 0, so its bits order as it does)
        atomicMax(&s_stat[SBQ_MAX_V2 * maxP + g], __float_as_uint((float)k.v2));
        s_key[d] = g * W + (logW ? __brev(d) >> (32u - logW) : 0u);
    }
    __syncthreads();

    // ---- live beams: a beam belongs to group g iff both endpoints do
    for (uint32_t j = tid; j < Bc; j += SBQ_BLOCK) {
        const uint32_t bd = g_bmap[j], w = g_bword[bd];
        const uint32_t g = s_grp[g_pmap[w & 0xffffu]];
        if (g == SBQ_NONE || g != s_grp[g_pmap[w >> 16]]) continue;
        const float4 q = g_bstate[bd]; // {target_length, last_length, strain, stress}
        if ((j >> 5) < V.nflagw && ((g_flags[j >> 5] >> (j & 31u)) & 1u)) atomicAdd(&s_stat[SBQ_PENDING * maxP + g], 1u);
        double strain;
        uint32_t k[2];
        if (!sbu_beam_leaf(q.z, q.w, strain, k)) {
            atomicAdd(&s_stat[SBQ_NB * maxP + g], 0x10001u);
            continue;
        }
        atomicAdd(&s_stat[SBQ_NB * maxP + g], 1u);
        atomicMax(&s_stat[SBQ_MAX_STRAIN * maxP + g], k[0]);
        atomicMax(&s_stat[SBQ_MAX_STRESS * maxP + g], k[1]);
        atomicMin(&s_stat[SBQ_MIN_STRESS * maxP + g], k[1]);
    }
    // ---- the ranking: particles descending, then label ascending
    for (uint32_t q = tid; q < W; q += SBQ_BLOCK) {
        const uint32_t np = q < maxP ? (s_stat[SBQ_NP * maxP + q] & 0xffffu) : 0u;
        s_rkey[q] = sbq_rank_key(np, q);
    }
    __syncthreads();
    sbq_sort(s_rkey, W, tid);
    for (uint32_t q = tid; q < W; q += SBQ_BLOCK)
        if (s_rkey[q] != SBQ_NONE) s_rank[sbq_rank_label(s_rkey[q])] = q;

    // ---- the members in key order, their leaves behind them
    sbq_sort(s_key, W, tid);
    for (uint32_t q = tid; q < W; q += SBQ_BLOCK) {
        const uint32_t key = s_key[q];
        if (key == SBQ_NONE) continue;
        const uint32_t r = key & (W - 1u), d = logW ? __brev(r) >> (32u - logW) : 0u;
        double leaf[SBQ_NSUM];
        SbuParticleKeys k;
        sbu_particle_values(g_part[3u * d], g_part[3u * d + 1u], leaf, k); // (a member: finite)
#pragma unroll
        for (uint32_t c = 0; c < SBQ_NSUM; c++) s_col[c * W + q] = leaf[c];
    }
    __syncthreads();

    // ---- the tree over the members alone
    for (uint32_t l = 0u; l < logW; l++) {
        for (uint32_t q = tid + (tid == 0u ? SBQ_BLOCK : 0u); q < W; q += SBQ_BLOCK) { // (position 0 never adds)
            if (s_key[q] == SBQ_NONE) continue;
            const uint32_t lo = sbu_sparse_step(s_key, q, l, 0u);
            if (lo == SBU_NO_ADD) continue;
#pragma unroll
            for (uint32_t k = 0; k < SBQ_NSUM; k++) s_col[k * W + lo] = s_col[k * W + lo] + s_col[k * W + q];
        }
        __syncthreads();
    }

    // ---- the rank of every data index
    if (rank) {
        int32_t *krow = rank + (size_t)scene * maxP;
        for (uint32_t d = tid; d < maxP; d += SBQ_BLOCK) {
            const uint32_t g = s_grp[d];
            krow[d] = g == SBQ_NONE ? -1 : (int32_t)s_rank[g];
        }
    }
    if (!rows) return; // (uniform)
    float *out = rows + (size_t)scene * max_rows * SB_BATCH_BODY_SUMMARY_WORDS;
    // ---- the sums, from the first sorted position of every label that has a finite member
    for (uint32_t q = tid; q < W; q += SBQ_BLOCK) {
        const uint32_t key = s_key[q];
        if (key == SBQ_NONE || (q != 0u && (s_key[q - 1u] >> logW) == (key >> logW))) continue;
        const uint32_t g = key >> logW, r = s_rank[g];
        if (r >= max_rows) continue;
        const uint32_t cnt = s_stat[SBQ_NP * maxP + g];
        float *row = out + (size_t)r * SB_BATCH_BODY_SUMMARY_WORDS;
        double tot[SBQ_NSUM];
#pragma unroll
        for (uint32_t k = 0; k < SBQ_NSUM; k++) tot[k] = sbu_canon(s_col[k * W + q]);
        sbu_row_sums(row, (cnt & 0xffffu) - (cnt >> 16), tot);
        row[19] = (float)tot[5];
    }
    // ---- everything else, one row per thread
    for (uint32_t r = tid; r < max_rows; r += SBQ_BLOCK) {
        float *row = out + (size_t)r * SB_BATCH_BODY_SUMMARY_WORDS;
        const uint32_t rkey = r < W ? s_rkey[r] : SBQ_NONE;
        if (rkey == SBQ_NONE) { // behind the last group: the empty row
#pragma unroll
            for (uint32_t k = 0; k < SB_BATCH_BODY_SUMMARY_WORDS; k++)
                row[k] = sbu_empty_body_word(k);
            continue;
        }
        const uint32_t g = sbq_rank_label(rkey);
        const uint32_t cp = s_stat[SBQ_NP * maxP + g], cb = s_stat[SBQ_NB * maxP + g];
        const uint32_t np = (cp & 0xffffu) - (cp >> 16), nb = (cb & 0xffffu) - (cb >> 16);
        row[0] = (float)(cp & 0xffffu);
        row[1] = (float)(cb & 0xffffu);
        row[2] = (float)g;
        row[3] = (float)s_stat[SBQ_PENDING * maxP + g];
        row[4] = (float)(cp >> 16);
        row[5] = (float)(cb >> 16);
        if (np == 0u) { // no finite member: no sorted position wrote the sums
            row[6] = row[7] = row[8] = row[9] = __uint_as_float(SBB_QNAN);
            row[14] = row[19] = 0.0f;
        }
        sbu_row_extremes(row, np, nb, SbuRowKeys{s_stat[SBQ_MINX * maxP + g], s_stat[SBQ_MINY * maxP + g], s_stat[SBQ_MAXX * maxP + g],
                                                 s_stat[SBQ_MAXY * maxP + g], __uint_as_float(s_stat[SBQ_MAX_V2 * maxP + g]),
                                                 s_stat[SBQ_MAX_STRAIN * maxP + g], s_stat[SBQ_MAX_STRESS * maxP + g],
                                                 s_stat[SBQ_MIN_STRESS * maxP + g]});
        row[20] = row[21] = row[22] = row[23] = 0.0f;
    }
}

// ---------------------------------------------------------------- host
bool sbb_body_summary_info(sb_batch *b, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "body_summary_words") *value = SB_BATCH_BODY_SUMMARY_WORDS;
    else if (k == "body_summary_lds_bytes") *value = sbq_lds_bytes(b->V.maxP);
    else return sbb_kernel_info(b, "body_summary", (const void *)k_batch_body_summary, b->body_summary_res, key, value);
    return true;
}

sb_status sb_batch_body_summary_device(sb_batch *b, const void *device_labels_i32, uint32_t max_rows, void *device_rows_f32, void *device_rank_i32)
{
    if (!b) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_body_summary_device: null batch");
    if (!device_labels_i32) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_body_summary_device: null labels");
    if (!device_rows_f32 && !device_rank_i32) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_body_summary_device: rows and rank are both null: nothing to write");
    if (max_rows == 0u || max_rows > b->V.maxP)
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_body_summary_device: max_rows %u is not in 1 .. max_particles (%u)", max_rows, b->V.maxP);
    if (sbb_misaligned4({device_labels_i32, device_rows_f32, device_rank_i32}))
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_body_summary_device: the device buffers must be 4-byte aligned");
    SB_HIP(b, hipSetDevice(b->device));
    const SbBatchView &V = b->V;
    const uint32_t W = sbb_pow2_at_least(V.maxP), lds = sbq_lds_bytes(V.maxP);
    uint32_t logW = 0u;
    while ((1u << logW) < W) logW++;
    if (lds > SBQ_LDS_DEFAULT_LIMIT && !b->body_summary_lds_allowed) {
        SB_HIP(b, hipFuncSetAttribute((const void *)k_batch_body_summary, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        b->body_summary_lds_allowed = true;
    }
    k_batch_body_summary<<<b->opt.n_scenes, SBQ_BLOCK, lds, b->stream>>>(V, (const int32_t *)device_labels_i32, max_rows, (float *)device_rows_f32,
                                                                       (int32_t *)device_rank_i32, W, logW);
    return check_launch(b, "sb_batch_body_summary_device");
}
