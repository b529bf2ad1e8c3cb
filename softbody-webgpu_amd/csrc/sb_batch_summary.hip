// sb_batch_summary.hip -- one row of SB_BATCH_SUMMARY_WORDS statistics per scene of a batch in ONE launch, and the rollout that
// strings inputs, frames and summaries together on the host (gfx950, wave64).
//
// The row is what a done-test or a planner's score reads of a scene: counts, means, extremes, the kinetic energy.  One workgroup
// per scene reads the scene's metadata words, the "holds a particle / beam" bytes of its constant blob and its state blob; nothing
// is written but the row.
//
// The sums are PINNED: double precision, leaf i = the value at DATA index i (+0.0 where nothing finite lives), i = 0 .. W-1 with W
// the smallest power of two >= the capacity, reduced by the stride-halving tree  for h = W/2 .. 1: s[i] += s[i + h] (i < h).
// That tree is evaluated here without ever holding W leaves:
//   h >= 256  both operands of every addition belong to the same thread (thread t owns the leaves t + 256 k), and the tree over a
//             thread's K = W / 256 leaves is again stride-halving: tree(e_0 .. e_K-1) = tree(even e) + tree(odd e).  sbu_tree<K>.
//   h = 128, 64  through LDS: ((s[i] + s[i+128]) + (s[i+64] + s[i+192]))
//   h = 32 .. 1  a butterfly in wave 0: lane i < h receives s[i] + s[i ^ h] = s[i] + s[i + h]; IEEE addition is commutative.
// Levels with h >= W do not exist and are skipped (W is uniform), so a -0.0 is never met by a +0.0 the tree does not hold.
// Everything else in the row (counts, extremes) is order-free and goes through LDS atomics on integer keys.
// The leaves, the tree, the keys and the row's words 6 .. 18 are sb_summary_math.h's: sb_summary.hip calls the same functions.
#include <algorithm>
#include <string>

#include "sb_batch.h"

#define SBS_BLOCK 256u
#define SBS_NSUM 6u  // px, py, vx, vy, kinetic energy | strain

// LDS statistics words
enum {
    SBS_P_FIN, SBS_P_BAD, SBS_B_FIN, SBS_B_BAD, SBS_B_REMOVED, SBS_PENDING,
    SBS_MINX, SBS_MINY, SBS_MAXX, SBS_MAXY, SBS_MAX_STRAIN, SBS_MAX_STRESS, SBS_MIN_STRESS, SBS_NSTAT
};

struct SbsScene {
    const unsigned char *pex, *bex, *balive;
    const float2 *part;
    const float4 *bstate;
    uint32_t maxP, maxB, tid;
};

// leaf k of this thread: the particle / the beam at data index tid + 256 k (sb_summary_math.h: its leaves, its share of `l`)
struct SbsParticleLeaf {
    const SbsScene &s;
    SbuLocal &l;
    SB_DEV void operator()(uint32_t k, double (&out)[5]) const
    {
#pragma unroll
        for (int c = 0; c < 5; c++) out[c] = 0.0;
        const uint32_t i = s.tid + k * SBS_BLOCK;
        if (i >= s.maxP || !s.pex[i]) return;
        sbu_local_particle(l, s.part[3u * i], s.part[3u * i + 1u], s.part[3u * i + 2u], out);
    }
};
struct SbsBeamLeaf {
    const SbsScene &s;
    SbuLocal &l;
    SB_DEV void operator()(uint32_t k, double (&out)[1]) const
    {
        out[0] = 0.0;
        const uint32_t i = s.tid + k * SBS_BLOCK;
        if (i >= s.maxB || !s.bex[i] || !s.balive[i]) return;
        const float4 q = s.bstate[i]; // {target_length, last_length, strain, stress}
        sbu_local_beam(l, q.z, q.w, out);
    }
};

__global__ __launch_bounds__(SBS_BLOCK) void k_batch_summary(SbBatchView V, float *__restrict__ rows, uint32_t Wp, uint32_t Wb)
{
    __shared__ double s_sum[SBS_NSUM][SBS_BLOCK];
    __shared__ unsigned long long s_max_v2;
    __shared__ uint32_t s_stat[SBS_NSTAT];
    const uint32_t scene = blockIdx.x, tid = threadIdx.x;
    if (scene >= V.n_scenes) return;
    float *row = rows + (size_t)scene * SB_BATCH_SUMMARY_WORDS;
    const SbbScene hd = sbb_scene(V, scene);
    if (hd.loaded == 0u) { // never uploaded: counts 0, no statistic
        if (tid < SB_BATCH_SUMMARY_WORDS) row[tid] = (tid <= 5u || tid == 14u || tid >= 20u) ? 0.0f : __uint_as_float(SBB_QNAN);
        return;
    }
    const uint32_t P = hd.P, Bc = hd.Bc; // (P: the metadata's own word, an upload is refused unless it fits the capacity)
    const unsigned char *cst = hd.cst, *st = hd.st;
    SbsScene s;
    s.pex = cst + V.o_pex, s.bex = cst + V.o_bex, s.balive = st + V.o_balive;
    s.part = (const float2 *)(st + V.o_part), s.bstate = (const float4 *)(st + V.o_bstate);
    s.maxP = V.maxP, s.maxB = V.maxB, s.tid = tid;

    if (tid < SBS_NSTAT) s_stat[tid] = (tid == SBS_MINX || tid == SBS_MINY || tid == SBS_MIN_STRESS) ? SBB_KEY_MOST : 0u;
    if (tid == 0u) s_max_v2 = 0ull;
    __syncthreads();

    // ---- leaves and the levels of the tree that stay inside a thread
    SbuLocal l;
    double ps[5], bs[1];
    const SbsParticleLeaf pleaf{s, l};
    const SbsBeamLeaf bleaf{s, l};
    switch (Wp > SBS_BLOCK ? Wp / SBS_BLOCK : 1u) { // (capacity <= SB_BATCH_MAX_PARTICLES = 1024)
    case 1u: sbu_tree<1, 5>(pleaf, 0u, 1u, ps); break;
    case 2u: sbu_tree<2, 5>(pleaf, 0u, 1u, ps); break;
    default: sbu_tree<4, 5>(pleaf, 0u, 1u, ps); break;
    }
    switch (Wb > SBS_BLOCK ? Wb / SBS_BLOCK : 1u) { // (capacity <= SB_BATCH_MAX_BEAMS = 4096)
    case 1u: sbu_tree<1, 1>(bleaf, 0u, 1u, bs); break;
    case 2u: sbu_tree<2, 1>(bleaf, 0u, 1u, bs); break;
    case 4u: sbu_tree<4, 1>(bleaf, 0u, 1u, bs); break;
    case 8u: sbu_tree<8, 1>(bleaf, 0u, 1u, bs); break;
    default: sbu_tree<16, 1>(bleaf, 0u, 1u, bs); break;
    }
#pragma unroll
    for (int k = 0; k < 5; k++) s_sum[k][tid] = ps[k];
    s_sum[5][tid] = bs[0];

    // ---- what does not depend on an order
    uint32_t removed = 0u, pending = 0u;
    for (uint32_t i = tid; i < V.maxB; i += SBS_BLOCK) removed += (s.bex[i] && !s.balive[i]) ? 1u : 0u;
    const uint32_t *flags = (const uint32_t *)(st + V.o_bflags);
    for (uint32_t w = tid; w < ((Bc + 31u) >> 5) && w < V.nflagw; w += SBS_BLOCK) { // one bit per beam SLOT; slots < Bc are live
        const uint32_t valid = (Bc - 32u * w >= 32u) ? 0xFFFFFFFFu : (1u << (Bc & 31u)) - 1u;
        pending += __popc(flags[w] & valid);
    }
    if (removed) atomicAdd(&s_stat[SBS_B_REMOVED], removed);
    if (pending) atomicAdd(&s_stat[SBS_PENDING], pending);
    if (l.p_bad) atomicAdd(&s_stat[SBS_P_BAD], l.p_bad);
    if (l.b_bad) atomicAdd(&s_stat[SBS_B_BAD], l.b_bad);
    if (l.p_fin) {
        atomicAdd(&s_stat[SBS_P_FIN], l.p_fin);
        atomicMin(&s_stat[SBS_MINX], l.minx);
        atomicMin(&s_stat[SBS_MINY], l.miny);
        atomicMax(&s_stat[SBS_MAXX], l.maxx);
        atomicMax(&s_stat[SBS_MAXY], l.maxy);
        atomicMax(&s_max_v2, (unsigned long long)__double_as_longlong(l.max_v2)); // (>= 0: its bits order as it does)
    }
    if (l.b_fin) {
        atomicAdd(&s_stat[SBS_B_FIN], l.b_fin);
        atomicMax(&s_stat[SBS_MAX_STRAIN], l.max_strain);
        atomicMax(&s_stat[SBS_MAX_STRESS], l.max_stress);
        atomicMin(&s_stat[SBS_MIN_STRESS], l.min_stress);
    }
    __syncthreads();
    if (tid >= 64u) return;

    // ---- the rest of the tree (wave 0), then the row
    double tot[SBS_NSUM];
#pragma unroll
    for (uint32_t k = 0; k < SBS_NSUM; k++) tot[k] = sbu_tree_tail(s_sum[k], tid, k < 5u ? Wp : Wb);
    if (tid != 0u) return;
    const uint32_t np = s_stat[SBS_P_FIN], nb = s_stat[SBS_B_FIN];
    row[0] = (float)P;
    row[1] = (float)Bc;
    row[2] = (float)s_stat[SBS_B_REMOVED];
    row[3] = (float)s_stat[SBS_PENDING];
    row[4] = (float)s_stat[SBS_P_BAD];
    row[5] = (float)s_stat[SBS_B_BAD];
    sbu_row_sums(row, np, tot);
    sbu_row_extremes(row, np, nb, SbuRowKeys{s_stat[SBS_MINX], s_stat[SBS_MINY], s_stat[SBS_MAXX], s_stat[SBS_MAXY],
                                             (float)__longlong_as_double((long long)s_max_v2), s_stat[SBS_MAX_STRAIN],
                                             s_stat[SBS_MAX_STRESS], s_stat[SBS_MIN_STRESS]});
    row[19] = nb ? (float)(tot[5] / (double)nb) : __uint_as_float(SBB_QNAN);
    row[20] = 1.0f;
    row[21] = row[22] = row[23] = 0.0f;
}

// ---------------------------------------------------------------- host
static sb_status launch_summary(sb_batch *b, float *rows)
{
    const SbBatchView &V = b->V;
    k_batch_summary<<<b->opt.n_scenes, SBS_BLOCK, 0, b->stream>>>(V, rows, sbb_pow2_at_least(V.maxP), sbb_pow2_at_least(V.maxB));
    return check_launch(b, "sb_batch_summary_device");
}

bool sbb_summary_info(sb_batch *b, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "summary_words") *value = SB_BATCH_SUMMARY_WORDS;
    else return sbb_kernel_info(b, "summary", (const void *)k_batch_summary, b->summary_res, key, value);
    return true;
}

sb_status sb_batch_summary_device(sb_batch *b, void *device_out_f32)
{
    if (!b) return SB_ERR_INVALID;
    if (!device_out_f32 || sbb_misaligned4({device_out_f32})) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_summary_device: null or misaligned device buffer");
    SB_HIP(b, hipSetDevice(b->device));
    return launch_summary(b, (float *)device_out_f32);
}

sb_status sb_batch_rollout_device(sb_batch *b, uint32_t n_frames, const void *device_inputs, void *device_summaries)
{
    if (!b) return SB_ERR_INVALID;
    if (sbb_misaligned4({device_inputs, device_summaries}))
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_rollout_device: input and summary buffers must be 4-byte aligned");
    const size_t n = b->opt.n_scenes;
    for (uint32_t t = 0; t < n_frames; t++) { // the individual calls, in their order: nothing here that they do not do
        if (device_inputs) SB_TRY(sb_batch_write_user_input_device(b, (const unsigned char *)device_inputs + (size_t)t * n * SB_USER_INPUT_BYTES));
        SB_TRY(sb_batch_frame(b, 1u));
        if (device_summaries) SB_TRY(launch_summary(b, (float *)device_summaries + (size_t)t * n * SB_BATCH_SUMMARY_WORDS));
    }
    return SB_OK;
}
