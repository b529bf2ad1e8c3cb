// sb_summary.hip -- one row of SB_SUMMARY_WORDS statistics of the whole scene of an sb_engine, reduced on the device (sb_summary /
// sb_summary_device of include/softbody.h; gfx950, wave64).
//
// The row is sb_batch_summary_device's, word for word (both files call sb_summary_math.h; tests/test_gpu_summary.py compares the two
// rows bit for bit), and so is its pin: sums in double, leaf i = the value at DATA index i (+0.0
// where no finite particle / beam lives), i = 0 .. W-1 with W the smallest power of two >= the capacity, reduced by the
// stride-halving tree  for h = W/2 .. 1: s[i] += s[i + h] (i < h).  An engine holds millions of leaves, so the tree is cut into
// launches.  What makes that possible: after all levels h >= n, element g < n holds the tree-sum of the leaves g + n k
// (k < W / n), and the tree over those W / n values is again stride-halving: tree(e_0 .. e_K-1) = tree(even e) + tree(odd e)
// (sbu_tree<K>, the batch kernel's recursion).  So
//   k_summary_particles<R> / k_summary_beams<R>   n = W / R threads; thread g tree-sums its own R leaves g + n k and writes one
//                                                 partial per column (x, y, vx, vy, energy | strain); neighbouring threads read
//                                                 neighbouring data indices
//   k_summary_fold<R>                             the same step on a column of partials, in place, n -> n / R
//   k_summary_row                                 one workgroup, at most 256 partials a column: levels 128 and 64 through LDS, the
//                                                 rest by the xor butterfly of wave 0 (sbu_tree_tail); forms the row
// Every launch performs exactly the additions of its levels on exactly the tree's operands, so the bits do not depend on where
// the cuts are (sb_summary_options.partials moves them).  A leaf above the highest data index in use is +0.0 WITHOUT a load:
// the addition stays (x + +0.0 turns a -0.0 into +0.0, as the tree does), the read goes.  Levels h >= W do not exist: with
// W < 256 the row kernel starts its butterfly below W.
// Counts and extremes do not depend on an order: per thread, then LDS atomics, then global atomics on integer keys (SbmStat).
#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "sb_report.h"
#include "sb_batch.h" // (sb_summary_math.h: the row's arithmetic, shared with the batch)

#define SBM_BLOCK 256u
#define SBM_RMAX 64u      // partials a thread of a fold tree-sums, at most
#define SBM_RMAX_LEAF 16u // leaves a thread of a leaf launch tree-sums, at most (all its loads are in flight at once: 179 VGPRs)

// statistics words (unsigned long long each; extremes as ordered keys, so that the neutral values below never win)
enum {
    SBM_P_FIN, SBM_P_BAD, SBM_B_FIN, SBM_B_BAD, SBM_B_REMOVED, SBM_PENDING, SBM_MAX_V2, SBM_MAXX, SBM_MAXY, SBM_MAX_STRAIN,
    SBM_MAX_STRESS, SBM_MINX, SBM_MINY, SBM_MIN_STRESS, SBM_NSTAT
};
SB_DEV unsigned long long sbm_neutral(uint32_t k) { return k >= SBM_MINX ? ~0ull : 0ull; }

struct SbmParticles {
    const uint32_t *inv; // data index -> internal particle (0xFFFFFFFF: none), n_leaf entries
    const float2 *pos, *vel, *acc;
    uint32_t n_leaf;
};
struct SbmBeams {
    const uint2 *leaf;   // data index -> {engine slot (0xFFFFFFFF: none), copy read back for it}, n_leaf entries
    const uint32_t *dead, *broken; // per engine slot: delete pass that removed it (NULL: none has run); bit per copy
    const float *strain, *stress;
    uint32_t n_leaf;
};
struct SbmLocal : SbuLocal {
    uint32_t removed = 0u, pending = 0u;
};

// the particle leaves of data index d: {px, py, vx, vy, 0.5 (vx^2 + vy^2)}
struct SbmParticleLeaf {
    const SbmParticles &s;
    SbmLocal &l;
    uint32_t g, n;
    SB_DEV void operator()(uint32_t k, double (&out)[5]) const
    {
#pragma unroll
        for (int c = 0; c < 5; c++) out[c] = 0.0;
        const uint64_t d = (uint64_t)g + (uint64_t)n * k;
        if (d >= s.n_leaf) return;
        const uint32_t i = s.inv[d];
        if (i == 0xFFFFFFFFu) return;
        sbu_local_particle(l, s.pos[i], s.vel[i], s.acc[i], out);
    }
};

// the beam leaf of data index d: strain
struct SbmBeamLeaf {
    const SbmBeams &s;
    SbmLocal &l;
    uint32_t g, n;
    SB_DEV void operator()(uint32_t k, double (&out)[1]) const
    {
        out[0] = 0.0;
        const uint64_t d = (uint64_t)g + (uint64_t)n * k;
        if (d >= s.n_leaf) return;
        const uint2 t = s.leaf[d];
        if (t.x == 0xFFFFFFFFu) return;
        if (s.dead && s.dead[t.x] != 0u) {
            l.removed++;
            return;
        }
        l.pending += (s.broken[t.y >> 5] >> (t.y & 31u)) & 1u;
        sbu_local_beam(l, s.strain[t.y], s.stress[t.y], out);
    }
};

// a column of partials: element g + n k
struct SbmPartialLeaf {
    const double *col;
    uint32_t g, n;
    SB_DEV void operator()(uint32_t k, double (&out)[1]) const { out[0] = col[(size_t)g + (size_t)n * k]; }
};

// a workgroup's share of the order-free statistics: LDS first, then one global atomic per word that is not neutral
SB_DEV void sbm_push_stats(const SbmLocal &l, unsigned long long *s_stat, unsigned long long *stat, uint32_t tid)
{
    if (tid < SBM_NSTAT) s_stat[tid] = sbm_neutral(tid);
    __syncthreads();
    if (l.p_bad) atomicAdd(&s_stat[SBM_P_BAD], (unsigned long long)l.p_bad);
    if (l.b_bad) atomicAdd(&s_stat[SBM_B_BAD], (unsigned long long)l.b_bad);
    if (l.removed) atomicAdd(&s_stat[SBM_B_REMOVED], (unsigned long long)l.removed);
    if (l.pending) atomicAdd(&s_stat[SBM_PENDING], (unsigned long long)l.pending);
    if (l.p_fin) {
        atomicAdd(&s_stat[SBM_P_FIN], (unsigned long long)l.p_fin);
        atomicMin(&s_stat[SBM_MINX], (unsigned long long)l.minx);
        atomicMin(&s_stat[SBM_MINY], (unsigned long long)l.miny);
        atomicMax(&s_stat[SBM_MAXX], (unsigned long long)l.maxx);
        atomicMax(&s_stat[SBM_MAXY], (unsigned long long)l.maxy);
        atomicMax(&s_stat[SBM_MAX_V2], (unsigned long long)__double_as_longlong(l.max_v2)); // (>= 0: its bits order as it does)
    }
    if (l.b_fin) {
        atomicAdd(&s_stat[SBM_B_FIN], (unsigned long long)l.b_fin);
        atomicMax(&s_stat[SBM_MAX_STRAIN], (unsigned long long)l.max_strain);
        atomicMax(&s_stat[SBM_MAX_STRESS], (unsigned long long)l.max_stress);
        atomicMin(&s_stat[SBM_MIN_STRESS], (unsigned long long)l.min_stress);
    }
    __syncthreads();
    if (tid < SBM_NSTAT) {
        const unsigned long long v = s_stat[tid];
        if (v != sbm_neutral(tid)) {
            if (tid <= SBM_PENDING) atomicAdd(&stat[tid], v);
            else if (tid < SBM_MINX) atomicMax(&stat[tid], v);
            else atomicMin(&stat[tid], v);
        }
    }
}

__global__ __launch_bounds__(64) void k_summary_init(unsigned long long *stat)
{
    if (threadIdx.x < SBM_NSTAT) stat[threadIdx.x] = sbm_neutral(threadIdx.x);
}

// n threads; thread g: the tree over its R particle leaves g + n k, one partial per column into part[c * n + g]
template <int R>
__global__ __launch_bounds__(SBM_BLOCK) void k_summary_particles(SbmParticles s, uint32_t n, double *part, unsigned long long *stat)
{
    __shared__ unsigned long long s_stat[SBM_NSTAT];
    const uint32_t tid = threadIdx.x, g = blockIdx.x * SBM_BLOCK + tid;
    SbmLocal l;
    if (g < n) {
        double out[5];
        sbu_tree<R, 5>(SbmParticleLeaf{s, l, g, n}, 0u, 1u, out);
#pragma unroll
        for (int c = 0; c < 5; c++) part[(size_t)c * n + g] = out[c];
    }
    sbm_push_stats(l, s_stat, stat, tid);
}

template <int R>
__global__ __launch_bounds__(SBM_BLOCK) void k_summary_beams(SbmBeams s, uint32_t n, double *part, unsigned long long *stat)
{
    __shared__ unsigned long long s_stat[SBM_NSTAT];
    const uint32_t tid = threadIdx.x, g = blockIdx.x * SBM_BLOCK + tid;
    SbmLocal l;
    if (g < n) {
        double out[1];
        sbu_tree<R, 1>(SbmBeamLeaf{s, l, g, n}, 0u, 1u, out);
        part[g] = out[0];
    }
    sbm_push_stats(l, s_stat, stat, tid);
}

// column blockIdx.y of `part` (columns `stride` apart), in place: element g < n_out becomes the tree over the elements g + n_out k,
// k < R.  Thread g alone reads element g, and nobody writes an element >= n_out, so in place is safe.
template <int R>
__global__ __launch_bounds__(SBM_BLOCK) void k_summary_fold(double *part, uint32_t stride, uint32_t n_out)
{
    const uint32_t g = blockIdx.x * SBM_BLOCK + threadIdx.x;
    if (g >= n_out) return;
    double *col = part + (size_t)blockIdx.y * stride;
    double out[1];
    sbu_tree<R, 1>(SbmPartialLeaf{col, g, n_out}, 0u, 1u, out);
    col[g] = out[0];
}

// one workgroup: wp <= 256 partials of each particle column (columns stride_p apart), wb <= 256 of the strain column
__global__ __launch_bounds__(SBM_BLOCK) void k_summary_row(const double *__restrict__ pcol, uint32_t stride_p, uint32_t wp,
                                                           const double *__restrict__ bcol, uint32_t wb,
                                                           const unsigned long long *__restrict__ stat,
                                                           float *row, unsigned long long *counts)
{
    __shared__ double s_sum[6][SBM_BLOCK];
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (uint32_t c = 0; c < 5u; c++) s_sum[c][tid] = tid < wp ? pcol[(size_t)c * stride_p + tid] : 0.0;
    s_sum[5][tid] = tid < wb ? bcol[tid] : 0.0;
    __syncthreads();
    if (tid >= 64u) return;
    double tot[6];
#pragma unroll
    for (uint32_t c = 0; c < 6u; c++) tot[c] = sbu_tree_tail(s_sum[c], tid, c < 5u ? wp : wb);
    if (tid != 0u) return;
    const unsigned long long np = stat[SBM_P_FIN], nb = stat[SBM_B_FIN], removed = stat[SBM_B_REMOVED];
    // (the engine keeps no metadata buffer on the device: particle_i_c is the particles the leaf launches met, beam_i_c the beams
    // they met alive -- counted on the device, no host shadow enters the row)
    const unsigned long long c8[8] = {np + stat[SBM_P_BAD], nb + stat[SBM_B_BAD], removed, stat[SBM_PENDING], stat[SBM_P_BAD], stat[SBM_B_BAD], 1ull, 0ull};
#pragma unroll
    for (int k = 0; k < 6; k++) row[k] = (float)c8[k];
    sbu_row_sums(row, np, tot);
    sbu_row_extremes(row, np, nb, SbuRowKeys{(uint32_t)stat[SBM_MINX], (uint32_t)stat[SBM_MINY], (uint32_t)stat[SBM_MAXX], (uint32_t)stat[SBM_MAXY],
                                             (float)__longlong_as_double((long long)stat[SBM_MAX_V2]), (uint32_t)stat[SBM_MAX_STRAIN],
                                             (uint32_t)stat[SBM_MAX_STRESS], (uint32_t)stat[SBM_MIN_STRESS]});
    row[19] = nb ? (float)(tot[5] / (double)nb) : __uint_as_float(SBB_QNAN);
    row[20] = 1.0f;
    row[21] = row[22] = row[23] = 0.0f;
    if (counts) {
#pragma unroll
        for (int k = 0; k < 8; k++) counts[k] = c8[k];
    }
}

// ---------------------------------------------------------------- host side

// The tree is over DATA indices, the engine's arrays are in its own order.  Particles: the shared table data index -> internal
// particle (sbq_need).  Beams, this file's own: per beam data index the engine slot and the copy sb_load_buffers reads back for it
// (its beam loop; the caller's slots of the latest upload).  Both end at the highest data index in use: a capacity far above the
// scene costs no reads.
static sb_status sbm_build_bleaf(sb_engine *e)
{
    const auto t0 = std::chrono::steady_clock::now();
    SbStateIoState &s = *e->sio;
    const uint32_t Bu = sb_user_beams(e);
    if (e->h_copy_of_slot.size() < e->B) SB_FAIL(e, SB_ERR_STATE, "sb_summary: host shadows of the scene are inconsistent");
    std::vector<uint2> slots;
    SB_TRY(sbq_user_slots(e, "sb_summary", slots));
    uint32_t nb = 0;
    for (uint32_t u = 0; u < Bu; u++) nb = std::max(nb, slots[u].y + 1u);
    std::vector<uint2> leaf(std::max<uint32_t>(nb, 1), make_uint2(0xFFFFFFFFu, 0u));
    for (uint32_t u = 0; u < Bu; u++) leaf[slots[u].y] = make_uint2(slots[u].x, e->h_copy_of_slot[slots[u].x]);
    for (uint32_t u = 0; u < Bu; u++)
        if (leaf[slots[u].y].y >= e->nbeam) SB_FAIL(e, SB_ERR_STATE, "sb_summary: beam copy outside the scene");
    SB_TRY(s.buf[SBM_B_BLEAF].grow(e, leaf.size() * sizeof(uint2)));
    SB_HIP(e, hipMemcpyAsync(s.buf[SBM_B_BLEAF].p, leaf.data(), leaf.size() * sizeof(uint2), hipMemcpyHostToDevice, e->stream));
    SB_HIP(e, hipStreamSynchronize(e->stream)); // (the host vectors go out of scope)
    s.sum_nb = nb;
    s.bleaf_valid = true;
    s.bleaf_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SB_OK;
}

// the widths a tree over W leaves is cut at with `m` partials asked for: the leaf launch writes first() partials a column
// (a thread sums at most SBM_RMAX_LEAF leaves), folds go on to m and then to at most 256, each by at most SBM_RMAX
struct SbmCut {
    uint32_t W, m;
    uint32_t first() const { return W <= m ? W : std::max(m, W / SBM_RMAX_LEAF); }
    uint32_t next(uint32_t n) const { return n > m ? std::max(m, n / SBM_RMAX) : std::max(std::min(n, SBM_BLOCK), n / SBM_RMAX); }
};
static uint32_t sbm_default_partials(uint32_t W) { return std::min(std::max(W / 4u, SBM_BLOCK), (uint32_t)SB_SUMMARY_MAX_PARTIALS); }

#define SBM_SWITCH_LEAF(R, CALL)                                \
    switch (R) {                                                \
    case 1u: { constexpr int R_ = 1; CALL; } break;             \
    case 2u: { constexpr int R_ = 2; CALL; } break;             \
    case 4u: { constexpr int R_ = 4; CALL; } break;             \
    case 8u: { constexpr int R_ = 8; CALL; } break;             \
    case 16u: { constexpr int R_ = 16; CALL; } break;           \
    default: SB_FAIL(e, SB_ERR_STATE, "sb_summary: no kernel sums %u values a thread", (unsigned)(R)); \
    }
#define SBM_SWITCH_FOLD(R, CALL)                                \
    switch (R) {                                                \
    case 32u: { constexpr int R_ = 32; CALL; } break;           \
    case 64u: { constexpr int R_ = 64; CALL; } break;           \
    default: SBM_SWITCH_LEAF(R, CALL)                           \
    }

static sb_status sbm_fold(sb_engine *e, const SbmCut &cut, double *part, uint32_t stride, uint32_t ncols, uint32_t *width)
{
    uint32_t n = *width;
    while (n > SBM_BLOCK) {
        const uint32_t n_out = cut.next(n), R = n / n_out;
        const dim3 grid((n_out + SBM_BLOCK - 1) / SBM_BLOCK, ncols);
        SBM_SWITCH_FOLD(R, (k_summary_fold<R_><<<grid, SBM_BLOCK, 0, e->stream>>>(part, stride, n_out)));
        n = n_out;
    }
    *width = n;
    return SB_OK;
}

static sb_status sbm_enqueue(sb_engine *e, const sb_summary_options *o, void *row, void *counts, bool host)
{
    if (!e) return SB_ERR_INVALID;
    const char *what = host ? "sb_summary" : "sb_summary_device";
    if (!row || ((uintptr_t)row & 3u)) SB_FAIL(e, SB_ERR_INVALID, "%s: null or misaligned row", what);
    if ((uintptr_t)counts & 7u) SB_FAIL(e, SB_ERR_INVALID, "%s: counts must be 8-byte aligned", what);
    const uint32_t m_asked = o && o->struct_size == sizeof(sb_summary_options) ? o->partials : 0u;
    if (m_asked && (m_asked < SBM_BLOCK || (m_asked & (m_asked - 1u)) || m_asked > SB_SUMMARY_MAX_PARTIALS))
        SB_FAIL(e, SB_ERR_INVALID, "%s: partials %u is not a power of two in [256, %u]", what, m_asked, (unsigned)SB_SUMMARY_MAX_PARTIALS);
    SB_TRY(sbq_preflight(e, what, o, "summed", "per-rank rows are not handled"));
    SB_TRY(sbq_need(e, "sb_summary", SBQ_PARTICLES));
    SbStateIoState &s = *e->sio;
    if (!s.bleaf_valid) SB_TRY(sbm_build_bleaf(e));
    s.sum_build_ms = s.part_ms + s.bleaf_ms;

    const SbmCut cp{sbb_pow2_at_least(e->opt.max_particles), m_asked ? m_asked : sbm_default_partials(sbb_pow2_at_least(e->opt.max_particles))};
    const SbmCut cb{sbb_pow2_at_least(e->opt.max_beams), m_asked ? m_asked : sbm_default_partials(sbb_pow2_at_least(e->opt.max_beams))};
    uint32_t np = cp.first(), nb = cb.first();
    const uint32_t stride_p = np;
    SB_TRY(s.buf[SBM_B_PART].grow(e, ((size_t)5 * np + nb) * sizeof(double)));
    SB_TRY(s.buf[SBM_B_STAT].grow(e, (size_t)SBM_NSTAT * sizeof(unsigned long long)));
    if (host) SB_TRY(s.buf[SBM_B_OUT].grow(e, ((size_t)8 + SB_SUMMARY_WORDS / 2) * sizeof(unsigned long long))); // 8 counts, then the row
    double *pcol = s.buf[SBM_B_PART].as<double>(), *bcol = pcol + (size_t)5 * np;
    unsigned long long *d_stat = s.buf[SBM_B_STAT].as<unsigned long long>(), *d_out = s.buf[SBM_B_OUT].as<unsigned long long>();
    SbqMirror mir(e, host);
    unsigned long long *d_counts = mir.out_at<unsigned long long>(counts, d_out, 0, 8 * sizeof(uint64_t));
    float *d_row = mir.out_at<float>(row, d_out, 8 * sizeof(uint64_t), SB_SUMMARY_WORDS * sizeof(float));

    k_summary_init<<<1, 64, 0, e->stream>>>(d_stat);
    const SbParticleArrays &c = e->part[e->cur];
    const SbmParticles sp{s.buf[SBQ_B_PINV].as<uint32_t>(), c.pos, c.vel, c.acc, s.np};
    const SbmBeams sbm{s.buf[SBM_B_BLEAF].as<uint2>(), sbq_dead(e),
                       e->d_broken, e->beams.strain, e->beams.stress, s.sum_nb};
    SBM_SWITCH_LEAF(cp.W / np, (k_summary_particles<R_><<<(np + SBM_BLOCK - 1) / SBM_BLOCK, SBM_BLOCK, 0, e->stream>>>(sp, np, pcol, d_stat)));
    SBM_SWITCH_LEAF(cb.W / nb, (k_summary_beams<R_><<<(nb + SBM_BLOCK - 1) / SBM_BLOCK, SBM_BLOCK, 0, e->stream>>>(sbm, nb, bcol, d_stat)));
    SB_TRY(sbm_fold(e, cp, pcol, stride_p, 5u, &np));
    SB_TRY(sbm_fold(e, cb, bcol, nb, 1u, &nb));
    k_summary_row<<<1, SBM_BLOCK, 0, e->stream>>>(pcol, stride_p, np, bcol, nb, d_stat, d_row, d_counts);
    SB_HIP(e, hipGetLastError());
    s.sum_partials = cp.m;
    return mir.finish();
}

// what sb_get_info reads ("summary_partials", "summary_table_build_us", "summary_kernel_vgprs", "summary_kernel_scratch_bytes")
bool sbm_info(sb_engine *e, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "summary_partials") *value = e->sio ? e->sio->sum_partials : 0u;
    else if (k == "summary_table_build_us") *value = e->sio ? (uint64_t)(e->sio->sum_build_ms * 1000.0 + 0.5) : 0u;
    else if (k == "summary_kernel_vgprs" || k == "summary_kernel_scratch_bytes") { // the most over every kernel a call may launch
#define SBM_LEAVES(K) (const void *)K<1>, (const void *)K<2>, (const void *)K<4>, (const void *)K<8>, (const void *)K<16>
        const std::vector<const void *> ks = {SBM_LEAVES(k_summary_particles), SBM_LEAVES(k_summary_beams), SBM_LEAVES(k_summary_fold),
                            (const void *)k_summary_fold<32>, (const void *)k_summary_fold<64>, (const void *)k_summary_row,
                            (const void *)k_summary_init};
#undef SBM_LEAVES
        return sbq_kernel_most(e, ks, k == "summary_kernel_vgprs", value);
    }
    else return false;
    return true;
}

extern "C" {

sb_status sb_summary_device(sb_engine *e, const sb_summary_options *opts, void *device_row_f32, void *device_counts_u64)
{
    SB_GUARDED(e, sbm_enqueue(e, opts, device_row_f32, device_counts_u64, false))
}

sb_status sb_summary(sb_engine *e, const sb_summary_options *opts, float *row, uint64_t *counts)
{
    SB_GUARDED(e, sbm_enqueue(e, opts, row, counts, true))
}

} // extern "C"
