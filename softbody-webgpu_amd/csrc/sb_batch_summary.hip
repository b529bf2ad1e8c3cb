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
//             thread's K = W / 256 leaves is again stride-halving: tree(e_0 .. e_K-1) = tree(even e) + tree(odd e).  sbs_tree<K>.
//   h = 128, 64  through LDS: ((s[i] + s[i+128]) + (s[i+64] + s[i+192]))
//   h = 32 .. 1  a butterfly in wave 0: lane i < h receives s[i] + s[i ^ h] = s[i] + s[i + h]; IEEE addition is commutative.
// Levels with h >= W do not exist and are skipped (W is uniform), so a -0.0 is never met by a +0.0 the tree does not hold.
// Everything else in the row (counts, extremes) is order-free and goes through LDS atomics on integer keys.
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
// what a thread gathers beside its sums
struct SbsLocal {
    uint32_t p_fin = 0u, p_bad = 0u, b_fin = 0u, b_bad = 0u;
    float minx = 0.f, miny = 0.f, maxx = 0.f, maxy = 0.f, max_strain = 0.f, max_stress = 0.f, min_stress = 0.f;
    double max_v2 = 0.0;
};

// the particle leaves of data index i: {px, py, vx, vy, 0.5 (vx^2 + vy^2)}
SB_DEV void sbs_particle_leaf(const SbsScene &s, uint32_t i, double (&out)[5], SbsLocal &l)
{
#pragma unroll
    for (int k = 0; k < 5; k++) out[k] = 0.0;
    if (i >= s.maxP || !s.pex[i]) return;
    const float2 p = s.part[3u * i], v = s.part[3u * i + 1u], a = s.part[3u * i + 2u];
    if (!(sbb_finite(p.x) && sbb_finite(p.y) && sbb_finite(v.x) && sbb_finite(v.y) && sbb_finite(a.x) && sbb_finite(a.y))) {
        l.p_bad++;
        return;
    }
    const double v2 = (double)v.x * (double)v.x + (double)v.y * (double)v.y; // (the products are exact)
    out[0] = (double)p.x, out[1] = (double)p.y, out[2] = (double)v.x, out[3] = (double)v.y, out[4] = 0.5 * v2;
    if (l.p_fin == 0u) {
        l.minx = l.maxx = p.x, l.miny = l.maxy = p.y, l.max_v2 = v2;
    } else {
        l.minx = p.x < l.minx ? p.x : l.minx, l.maxx = p.x > l.maxx ? p.x : l.maxx;
        l.miny = p.y < l.miny ? p.y : l.miny, l.maxy = p.y > l.maxy ? p.y : l.maxy;
        l.max_v2 = v2 > l.max_v2 ? v2 : l.max_v2;
    }
    l.p_fin++;
}

// the beam leaf of data index i: strain
SB_DEV void sbs_beam_leaf(const SbsScene &s, uint32_t i, double (&out)[1], SbsLocal &l)
{
    out[0] = 0.0;
    if (i >= s.maxB || !s.bex[i] || !s.balive[i]) return;
    const float4 q = s.bstate[i]; // {target_length, last_length, strain, stress}
    if (!(sbb_finite(q.z) && sbb_finite(q.w))) {
        l.b_bad++;
        return;
    }
    out[0] = (double)q.z;
    if (l.b_fin == 0u) {
        l.max_strain = q.z, l.max_stress = l.min_stress = q.w;
    } else {
        l.max_strain = q.z > l.max_strain ? q.z : l.max_strain;
        l.max_stress = q.w > l.max_stress ? q.w : l.max_stress;
        l.min_stress = q.w < l.min_stress ? q.w : l.min_stress;
    }
    l.b_fin++;
}

// the stride-halving tree over this thread's K leaves e_j = leaf(tid + (base + j step) 256), j < K
template <int K, int N, bool BEAMS>
SB_DEV void sbs_tree(const SbsScene &s, uint32_t base, uint32_t step, double (&out)[N], SbsLocal &l)
{
    if constexpr (K == 1) {
        if constexpr (BEAMS) sbs_beam_leaf(s, s.tid + base * SBS_BLOCK, out, l);
        else sbs_particle_leaf(s, s.tid + base * SBS_BLOCK, out, l);
    } else {
        double even[N], odd[N];
        sbs_tree<K / 2, N, BEAMS>(s, base, 2u * step, even, l);
        sbs_tree<K / 2, N, BEAMS>(s, base + step, 2u * step, odd, l);
#pragma unroll
        for (int k = 0; k < N; k++) out[k] = even[k] + odd[k];
    }
}

// levels h = 128 .. 1 of the tree over W leaves, of which s_col[0 .. 255] holds what the levels above left; the sum is lane 0's
SB_DEV double sbs_tree_tail(const double *s_col, uint32_t lane, uint32_t W)
{
    double v = s_col[lane];
    if (W >= 256u) v = (v + s_col[lane + 128u]) + (s_col[lane + 64u] + s_col[lane + 192u]);
    else if (W == 128u) v = v + s_col[lane + 64u];
#pragma unroll
    for (uint32_t h = 32u; h != 0u; h >>= 1)
        if (h < W) v = v + __shfl_xor(v, (int)h);
    return v;
}

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

    if (tid < SBS_NSTAT) s_stat[tid] = (tid == SBS_MINX || tid == SBS_MINY || tid == SBS_MIN_STRESS) ? 0xFFFFFFFFu : 0u;
    if (tid == 0u) s_max_v2 = 0ull;
    __syncthreads();

    // ---- leaves and the levels of the tree that stay inside a thread
    SbsLocal l;
    double ps[5], bs[1];
    switch (Wp > SBS_BLOCK ? Wp / SBS_BLOCK : 1u) { // (capacity <= SB_BATCH_MAX_PARTICLES = 1024)
    case 1u: sbs_tree<1, 5, false>(s, 0u, 1u, ps, l); break;
    case 2u: sbs_tree<2, 5, false>(s, 0u, 1u, ps, l); break;
    default: sbs_tree<4, 5, false>(s, 0u, 1u, ps, l); break;
    }
    switch (Wb > SBS_BLOCK ? Wb / SBS_BLOCK : 1u) { // (capacity <= SB_BATCH_MAX_BEAMS = 4096)
    case 1u: sbs_tree<1, 1, true>(s, 0u, 1u, bs, l); break;
    case 2u: sbs_tree<2, 1, true>(s, 0u, 1u, bs, l); break;
    case 4u: sbs_tree<4, 1, true>(s, 0u, 1u, bs, l); break;
    case 8u: sbs_tree<8, 1, true>(s, 0u, 1u, bs, l); break;
    default: sbs_tree<16, 1, true>(s, 0u, 1u, bs, l); break;
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
        atomicMin(&s_stat[SBS_MINX], sbb_fkey(l.minx));
        atomicMin(&s_stat[SBS_MINY], sbb_fkey(l.miny));
        atomicMax(&s_stat[SBS_MAXX], sbb_fkey(l.maxx));
        atomicMax(&s_stat[SBS_MAXY], sbb_fkey(l.maxy));
        atomicMax(&s_max_v2, (unsigned long long)__double_as_longlong(l.max_v2)); // (>= 0: its bits order as it does)
    }
    if (l.b_fin) {
        atomicAdd(&s_stat[SBS_B_FIN], l.b_fin);
        atomicMax(&s_stat[SBS_MAX_STRAIN], sbb_fkey(l.max_strain));
        atomicMax(&s_stat[SBS_MAX_STRESS], sbb_fkey(l.max_stress));
        atomicMin(&s_stat[SBS_MIN_STRESS], sbb_fkey(l.min_stress));
    }
    __syncthreads();
    if (tid >= 64u) return;

    // ---- the rest of the tree (wave 0), then the row
    double tot[SBS_NSUM];
#pragma unroll
    for (uint32_t k = 0; k < SBS_NSUM; k++) tot[k] = sbs_tree_tail(s_sum[k], tid, k < 5u ? Wp : Wb);
    if (tid != 0u) return;
    const float nan = __uint_as_float(SBB_QNAN);
    const uint32_t np = s_stat[SBS_P_FIN], nb = s_stat[SBS_B_FIN];
    row[0] = (float)P;
    row[1] = (float)Bc;
    row[2] = (float)s_stat[SBS_B_REMOVED];
    row[3] = (float)s_stat[SBS_PENDING];
    row[4] = (float)s_stat[SBS_P_BAD];
    row[5] = (float)s_stat[SBS_B_BAD];
#pragma unroll
    for (int k = 0; k < 4; k++) row[6 + k] = np ? (float)(tot[k] / (double)np) : nan;
    row[10] = np ? sbb_unkey(s_stat[SBS_MINX]) : nan;
    row[11] = np ? sbb_unkey(s_stat[SBS_MINY]) : nan;
    row[12] = np ? sbb_unkey(s_stat[SBS_MAXX]) : nan;
    row[13] = np ? sbb_unkey(s_stat[SBS_MAXY]) : nan;
    row[14] = (float)tot[4]; // (round to nearest: +inf beyond the range of float)
    row[15] = np ? (float)__longlong_as_double((long long)s_max_v2) : nan;
    row[16] = nb ? sbb_unkey(s_stat[SBS_MAX_STRAIN]) : nan;
    row[17] = nb ? sbb_unkey(s_stat[SBS_MAX_STRESS]) : nan;
    row[18] = nb ? sbb_unkey(s_stat[SBS_MIN_STRESS]) : nan;
    row[19] = nb ? (float)(tot[5] / (double)nb) : nan;
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
    else if (k == "summary_kernel_vgprs" || k == "summary_kernel_scratch_bytes")
        *value = sbb_kernel_res(b, b->summary_res, (const void *)k_batch_summary, k == "summary_kernel_vgprs");
    else return false;
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
