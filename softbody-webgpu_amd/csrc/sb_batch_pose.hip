// sb_batch_pose.hip -- the pose of every GROUP of particles (with sb_batch_bodies_device's labels: of every body) of every scene of
// a batch against a reference shape, in ONE launch, reproducible bit for bit (gfx950, wave64): centroids, the
// moments of the 2-D rotation fit, moment of inertia, spin and angular velocity.
//
// One workgroup per scene reads the caller's labels, the caller's reference positions or the scene's RESET blob, the scene's
// metadata words, its constant blob and its state blob; nothing is written but the rows, the moments and the ranks.
//
// Groups and ranking are sb_batch_body_summary.hip's, and so is the route of the sums (sb_batch_group_sort.h, sb_summary_math.h):
// the MATCHED members -- finite, and with a finite reference -- of all groups are sorted by the key  label * W + bitrev(data
// index), their eleven leaves (sb_batch_pose_math.h) are taken behind the sort, log2 W levels of sbu_sparse_step add a block's
// head onto the head of its left sibling, and the first sorted position of a label holds the sums of summary()'s pinned tree over
// the group's matched members alone.  That position derives the five moments (sbp_fit) and writes them; counts and the rows of
// groups without a matched member come from one thread per row.
#include <string>

#include "sb_batch_group_sort.h" // SBQ_BLOCK, sbq_sort, the rank key
#include "sb_batch_pose_math.h"

// LDS of a workgroup: double col[SBP_NSUM][W]; uint32 key[W], rkey[W], grp[maxP], rank[maxP], cnt[maxP]
static inline uint32_t sbp_lds_bytes(uint32_t maxP)
{
    const uint32_t W = sbb_pow2_at_least(maxP);
    return W * (SBP_NSUM * 8u + 2u * 4u) + maxP * 3u * 4u;
}

__global__ __launch_bounds__(SBQ_BLOCK) void k_batch_pose(SbBatchView V, const int32_t *__restrict__ labels, const float *__restrict__ ref,
                                                          uint32_t max_rows, float *__restrict__ rows, double *__restrict__ moments,
                                                          int32_t *__restrict__ rank, uint32_t W, uint32_t logW)
{
    extern __shared__ __attribute__((aligned(16))) double sbp_lds[];
    const uint32_t scene = blockIdx.x, tid = threadIdx.x;
    if (scene >= V.n_scenes) return;
    const uint32_t maxP = V.maxP;
    double *s_col = sbp_lds;                              // [SBP_NSUM][W] partial sums at sorted positions
    uint32_t *s_key = (uint32_t *)(s_col + SBP_NSUM * W); // [W] label * W + bitrev(data index) of the matched members, SBQ_NONE behind them
    uint32_t *s_rkey = s_key + W;                         // [W] the rank keys of the non-empty groups, SBQ_NONE behind them
    uint32_t *s_grp = s_rkey + W;                         // [maxP] per DATA index: its group, SBQ_NONE where there is none
    uint32_t *s_rank = s_grp + maxP;                      // [maxP] per label: its rank
    uint32_t *s_cnt = s_rank + maxP;                      // [maxP] per label: particles | particles that are not matched << 16

    const SbbScene hd = sbb_scene(V, scene);
    const uint32_t P = hd.P;
    // the particle slots of the reset state (rewritten between launches by checkpoint and fork: read at agent scope, as sbb_scene reads)
    const uint32_t P0 = sbb_uniform(SB_AGENT_LOAD(&V.meta[(size_t)scene * SB_BM_WORDS + SB_BM_P0]));
    const uint32_t *g_pmap = (const uint32_t *)(hd.cst + V.o_pmap);
    const float2 *g_part = (const float2 *)(hd.st + V.o_part);
    // the reference position at data index d, floats ref_step * d and the next: the caller's (4-byte aligned), or the reset
    // state's record
    const float *g_ref = ref ? ref + (size_t)scene * maxP * 2u : (const float *)(V.rst + (size_t)scene * V.st_bytes + V.o_part);
    const uint32_t ref_step = ref ? 2u : 6u;
    const int32_t *lrow = labels + (size_t)scene * maxP;

    // ---- clear
    for (uint32_t q = tid; q < W; q += SBQ_BLOCK) s_key[q] = SBQ_NONE;
    for (uint32_t d = tid; d < maxP; d += SBQ_BLOCK) s_grp[d] = SBQ_NONE, s_cnt[d] = 0u;
    __syncthreads();

    // ---- particles (an upload is refused unless its data indices are distinct and inside the capacity): group, counts, and the
    // sort key of a matched member, parked at its data index
    for (uint32_t s = tid; s < P; s += SBQ_BLOCK) {
        const uint32_t d = g_pmap[s];
        const uint32_t g = (uint32_t)lrow[d]; // (a negative label is a large unsigned one)
        if (g >= maxP) continue;
        s_grp[d] = g;
        // (without the caller's reference a particle spawned since the reset state -- slot >= P0 -- has none)
        const bool matched = sbu_particle_finite(g_part[3u * d], g_part[3u * d + 1u], g_part[3u * d + 2u]) && (ref || s < P0) &&
                             sbp_ref_finite(float2{g_ref[ref_step * d], g_ref[ref_step * d + 1u]});
        atomicAdd(&s_cnt[g], matched ? 1u : 0x10001u);
        if (matched) s_key[d] = g * W + (logW ? __brev(d) >> (32u - logW) : 0u);
    }
    __syncthreads();

    // ---- the ranking: particles descending, then label ascending
    for (uint32_t q = tid; q < W; q += SBQ_BLOCK) s_rkey[q] = sbq_rank_key(q < maxP ? (s_cnt[q] & 0xffffu) : 0u, q);
    __syncthreads();
    sbq_sort(s_rkey, W, tid);
    for (uint32_t q = tid; q < W; q += SBQ_BLOCK)
        if (s_rkey[q] != SBQ_NONE) s_rank[sbq_rank_label(s_rkey[q])] = q;

    // ---- the matched members in key order, their leaves behind them
    sbq_sort(s_key, W, tid);
    for (uint32_t q = tid; q < W; q += SBQ_BLOCK) {
        const uint32_t key = s_key[q];
        if (key == SBQ_NONE) continue;
        const uint32_t r = key & (W - 1u), d = logW ? __brev(r) >> (32u - logW) : 0u;
        double leaf[SBP_NSUM];
        sbp_leaves(g_part[3u * d], g_part[3u * d + 1u], float2{g_ref[ref_step * d], g_ref[ref_step * d + 1u]}, leaf);
#pragma unroll
        for (uint32_t c = 0; c < SBP_NSUM; c++) s_col[c * W + q] = leaf[c];
    }
    __syncthreads();

    // ---- the tree over the matched members alone
    for (uint32_t l = 0u; l < logW; l++) {
        for (uint32_t q = tid + (tid == 0u ? SBQ_BLOCK : 0u); q < W; q += SBQ_BLOCK) { // (position 0 never adds)
            if (s_key[q] == SBQ_NONE) continue;
            const uint32_t lo = sbu_sparse_step(s_key, q, l, 0u);
            if (lo == SBU_NO_ADD) continue;
#pragma unroll
            for (uint32_t k = 0; k < SBP_NSUM; k++) s_col[k * W + lo] = s_col[k * W + lo] + s_col[k * W + q];
        }
        __syncthreads();
    }

    float *out = rows ? rows + (size_t)scene * max_rows * SB_BATCH_POSE_WORDS : nullptr;
    double *mout = moments ? moments + (size_t)scene * max_rows * SB_BATCH_POSE_MOMENT_WORDS : nullptr;
    // ---- the sums and what derives from them, from the first sorted position of every label that has a matched member
    for (uint32_t q = tid; q < W; q += SBQ_BLOCK) {
        const uint32_t key = s_key[q];
        if (key == SBQ_NONE || (q != 0u && (s_key[q - 1u] >> logW) == (key >> logW))) continue;
        const uint32_t g = key >> logW, r = s_rank[g];
        if (r >= max_rows) continue;
        const uint32_t cnt = s_cnt[g];
        const double n = (double)((cnt & 0xffffu) - (cnt >> 16));
        double tot[SBP_NSUM];
#pragma unroll
        for (uint32_t k = 0; k < SBP_NSUM; k++) tot[k] = sbu_canon(s_col[k * W + q]);
        const SbpFit fit = sbp_fit(tot, n);
        if (out) sbp_row_fit(out + (size_t)r * SB_BATCH_POSE_WORDS, tot, n, fit);
        if (mout) sbp_moments(mout + (size_t)r * SB_BATCH_POSE_MOMENT_WORDS, n, fit);
    }
    // ---- everything else, one row per thread (max_rows <= maxP <= W)
    for (uint32_t r = tid; r < max_rows; r += SBQ_BLOCK) {
        const uint32_t rkey = s_rkey[r];
        uint32_t total = 0u, bad = 0u;
        float label = -1.0f; // behind the last group: the empty row
        if (rkey != SBQ_NONE) {
            const uint32_t g = sbq_rank_label(rkey), cnt = s_cnt[g];
            total = cnt & 0xffffu, bad = cnt >> 16, label = (float)g;
        }
        const bool unmatched = total == bad; // no matched member: no sorted position wrote words 4 .. 16 and the moments
        if (out) {
            float *row = out + (size_t)r * SB_BATCH_POSE_WORDS;
            row[0] = (float)total, row[1] = label, row[2] = (float)(total - bad), row[3] = (float)bad;
#pragma unroll
            for (uint32_t k = 4u; k < SB_BATCH_POSE_WORDS; k++)
                if (unmatched || k > 16u) row[k] = sbp_unmatched_word(k);
        }
        if (mout && unmatched) {
            double *m = mout + (size_t)r * SB_BATCH_POSE_MOMENT_WORDS;
#pragma unroll
            for (uint32_t k = 0; k < SB_BATCH_POSE_MOMENT_WORDS; k++) m[k] = sbp_unmatched_moment(k);
        }
    }
    // ---- the rank of every data index
    if (rank) {
        int32_t *krow = rank + (size_t)scene * maxP;
        for (uint32_t d = tid; d < maxP; d += SBQ_BLOCK) {
            const uint32_t g = s_grp[d];
            krow[d] = g == SBQ_NONE ? -1 : (int32_t)s_rank[g];
        }
    }
}

// ---------------------------------------------------------------- host
bool sbb_pose_info(sb_batch *b, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "pose_words") *value = SB_BATCH_POSE_WORDS;
    else if (k == "pose_moment_words") *value = SB_BATCH_POSE_MOMENT_WORDS;
    else if (k == "pose_lds_bytes") *value = sbp_lds_bytes(b->V.maxP);
    else return sbb_kernel_info(b, "pose", (const void *)k_batch_pose, b->pose_res, key, value);
    return true;
}

sb_status sb_batch_pose_device(sb_batch *b, const void *device_labels_i32, const void *device_ref_f32, uint32_t max_rows, void *device_rows_f32,
                               void *device_moments_f64, void *device_rank_i32)
{
    if (!b) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_pose_device: null batch");
    if (!device_labels_i32) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_pose_device: null labels");
    if (!device_rows_f32 && !device_moments_f64 && !device_rank_i32)
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_pose_device: rows, moments and rank are all null: nothing to write");
    if (max_rows == 0u || max_rows > b->V.maxP)
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_pose_device: max_rows %u is not in 1 .. max_particles (%u)", max_rows, b->V.maxP);
    if (sbb_misaligned4({device_labels_i32, device_ref_f32, device_rows_f32, device_rank_i32}) || ((uintptr_t)device_moments_f64 & 7u) != 0)
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_pose_device: the device buffers must be 4-byte aligned, the moments 8-byte aligned");
    SB_HIP(b, hipSetDevice(b->device));
    const SbBatchView &V = b->V;
    const uint32_t W = sbb_pow2_at_least(V.maxP), lds = sbp_lds_bytes(V.maxP);
    uint32_t logW = 0u;
    while ((1u << logW) < W) logW++;
    if (lds > SBQ_LDS_DEFAULT_LIMIT && !b->pose_lds_allowed) {
        SB_HIP(b, hipFuncSetAttribute((const void *)k_batch_pose, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        b->pose_lds_allowed = true;
    }
    k_batch_pose<<<b->opt.n_scenes, SBQ_BLOCK, lds, b->stream>>>(V, (const int32_t *)device_labels_i32, (const float *)device_ref_f32, max_rows,
                                                               (float *)device_rows_f32, (double *)device_moments_f64, (int32_t *)device_rank_i32, W,
                                                               logW);
    return check_launch(b, "sb_batch_pose_device");
}
