// sb_nearest.hip -- proximity queries over the whole scene of an sb_engine: for every point the nearest among the particles
// (centres), the live beams (segments) and the four walls, the closest point on it, and how many particles and beams lie within
// reach, found on the device (sb_nearest / sb_nearest_device of include/softbody.h; gfx950, wave64).
//
// The definition is sb_batch_nearest_device's, word for word: the distances of sb_batch_near_math.h, the winner the smallest key --
// here the WIDE key (bits(d2) << 32 | kind << 30 | index).  The scene is sorted into the ray casts' grid by the ray casts' sort
// (sbw_sort, sb_report.h), and a point looks only into the rings of cells that sb_near_walk.h proves sufficient.  One launch per
// stage, all on the engine's stream:
//   sbw_sort         the counting sort: particles, short beams, the leftover list; counts words 5 and 6
//   k_near_ends      a thread per caller beam slot: both endpoints at the beam's data index (the closest point and the label of a
//                    winning beam are computed from them)
//   k_near_walk      a thread per row: the verdict, the walls, and for a local row snw::walk over the rings; each run of neighbouring
//                    cells is read as ONE range of records, so the loads of a run do not wait for one another.  The winner and both
//                    within words stay in registers; the walk is the first writer of its row, so it STORES key, within and the
//                    swept mark (no memset, no atomic).  A row whose walk is not complete, or that is not local, is put on the
//                    sweep's list (device memory: no read-back)
//   k_near_sweep     a fixed grid strides over ALL records, each against the listed rows, which go through LDS a tile of 64 at a
//                    time.  Under rmax = +inf every (row, record) pair is kept, so nothing here costs an atomic per pair: a wave
//                    reduces each row's keys (cross-lane minimum) and counts (ballot, popcount) and lane k KEEPS row k's partial
//                    answer in registers over all the wave's records; per tile a wave then meets the workgroup in LDS and the
//                    workgroup meets memory with at most three atomics per row
//   k_near_leftover  a thread per valid row the sweep does not answer, against the leftover list, accumulating in registers
//   k_near_finish    a thread per row: d, hit, point and within; counts words 0 .. 3 by ballots
//   k_near_counts    the eight int64 words
// Nothing of the engine is written, nothing is read back, no workgroup waits for another.
#include <algorithm>
#include <string>
#include <vector>

#include "sb_report.h"
#include "sb_near_walk.h"

#define SBV_BLOCK 256u
#define SBV_SWEEP_BLOCKS 1024u
#define SBV_SWEEP_TILE 64u // the wave's width: lane k of a wave keeps row k of the tile
#define SBV_MAX_POINTS (1u << 24)
#define SBV_NONE 0xFFFFFFFFu
enum { SBV_A_VALID, SBV_A_PART, SBV_A_BEAM, SBV_A_WALL, SBV_A_SWEPT, SBV_A_OUTSIDE, SBV_A_LONG, SBV_A_ZERO, SBV_NACC }; // = the count words (5, 6: k_ray_bin's)

static_assert(SB_NEAREST_COUNT_WORDS == SBV_NACC && SB_NEAREST_COUNT_WORDS == SB_RAYCAST_COUNT_WORDS, "an accumulator per count word, the sort's among them");
static_assert(sizeof(sb_batch_near_point) == SBN_ROW_WORDS * 4u && SB_BATCH_NEAR_HIT_WORDS == SBN_HIT_WORDS, "the row and the hit row");
static_assert(SBN_WIDE_INDEX_BITS == SBR_WIDE_INDEX_BITS, "one wide key for both queries");

// one record against one row: the wide key, SBN_NO_KEY where the mask, the label or the reach leaves it out
SB_DEV uint64_t sbv_meet(const sbn::Probe &p, const srw::Rec &c, const int32_t *__restrict__ labels)
{
    const bool beam = (c.index & SRW_KIND_BIT) != 0u;
    if (!(p.mask & (beam ? sbn::MASK_BEAMS : sbn::MASK_PARTICLES))) return SBN_NO_KEY;
    if (p.skip != -1 && labels && labels[c.lsrc] == p.skip) return SBN_NO_KEY;
    const uint32_t index = c.index & ~SRW_KIND_BIT;
    return beam ? sbn::segment_wide(p, c.ax, c.ay, c.bx, c.by, index) : sbn::particle_wide(p, c.ax, c.ay, index);
}

// a row's running answer over the records it is tested against
struct SbvBest {
    uint64_t key;
    uint32_t in_p, in_b;
    SB_DEV void take(const sbn::Probe &p, const srw::Rec &c, const int32_t *__restrict__ labels)
    {
        const uint64_t k = sbv_meet(p, c, labels);
        const bool kept = k != SBN_NO_KEY, beam = (c.index & SRW_KIND_BIT) != 0u;
        in_p += kept && !beam, in_b += kept && beam;
        key = sbn::nearer(key, k);
    }
};

SB_DEV void sbv_load_row(const uint32_t *__restrict__ points, uint32_t j, uint32_t *w)
{
    const uint32_t *row = points + (size_t)j * SBN_ROW_WORDS; // (the caller's rows need only be 4-byte aligned)
#pragma unroll
    for (uint32_t i = 0; i < SBN_ROW_WORDS; i++) w[i] = row[i];
}

// tab: [4][n] = data index of A, of B, engine slot, copy; row: per caller slot the data index of its beam record
__global__ __launch_bounds__(SBV_BLOCK) void k_near_ends(const uint32_t *__restrict__ tab, uint32_t n, const uint32_t *__restrict__ row, uint32_t nd,
                                                         uint2 *__restrict__ ends)
{
    const uint32_t u = blockIdx.x * SBV_BLOCK + threadIdx.x;
    if (u >= n) return;
    const uint32_t d = row[u];
    if (d < nd) ends[d] = make_uint2(tab[u], tab[(size_t)n + u]);
}

// end: per bin the END of its records (bin 0 starts at 0).  within: NULL where the call does not ask for it.
__global__ __launch_bounds__(SBV_BLOCK) void k_near_walk(const uint32_t *__restrict__ points, uint32_t n_points, const int32_t *__restrict__ labels,
                                                         const srw::Rec *__restrict__ sorted, const uint32_t *__restrict__ end, srw::Grid g,
                                                         uint32_t max_rings, unsigned long long *__restrict__ keys, uint2 *__restrict__ within,
                                                         uint8_t *__restrict__ swept_of, uint32_t *list, uint32_t *n_list, unsigned long long *acc)
{
    const uint32_t j = blockIdx.x * SBV_BLOCK + threadIdx.x;
    bool swept = false;
    if (j < n_points) {
        uint32_t w[SBN_ROW_WORDS];
        sbv_load_row(points, j, w);
        SbvBest b{SBN_NO_KEY, 0u, 0u};
        if (sbn::row_verdict(w, labels != nullptr) == sbn::MISS) {
            const sbn::Probe p = sbn::probe_of(w);
            if (p.mask & sbn::MASK_WALLS) b.key = sbn::walls_wide(p, g.bounds);
            if (snw::local(p, g.bounds)) {
                swept = !snw::walk(
                    p, g, max_rings, within != nullptr,
                    [&](uint32_t first, uint32_t count) {
                        const uint32_t to = end[first + count - 1u];
                        for (uint32_t q = first ? end[first - 1u] : 0u; q < to; q++) b.take(p, sorted[q], labels);
                    },
                    [&]() { return b.key == SBN_NO_KEY ? -1.0f : sbn::word_as_float(sbn::key_d2(b.key)); });
            } else {
                swept = true;
            }
            if (swept) {
                list[atomicAdd(n_list, 1u)] = j; // (at most one place per row: n_points places)
                b.in_p = b.in_b = 0u;            // the sweep counts afresh; the key may stay
            }
        }
        keys[j] = b.key;
        swept_of[j] = swept;
        if (within) within[j] = make_uint2(b.in_p, b.in_b);
    }
    sbw_count(acc, SBV_A_SWEPT, swept);
}

// the smallest key of the wave, in every lane.  Every lane of the wave calls it.
SB_DEV unsigned long long sbv_wave_min(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned long long x = __shfl_xor(v, o);
        v = x < v ? x : v;
    }
    return v;
}

// a fixed grid over all `total` records (*total_dev: the scan's sum), each against the listed rows, a tile of 64 at a time.  Every
// trip count is uniform over the workgroup, so every lane meets every ballot, shuffle and barrier.
__global__ __launch_bounds__(SBV_BLOCK) void k_near_sweep(const uint32_t *__restrict__ points, const int32_t *__restrict__ labels,
                                                          const srw::Rec *__restrict__ sorted, const uint32_t *__restrict__ total_dev,
                                                          const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list,
                                                          unsigned long long *keys, uint32_t *within)
{
    __shared__ uint32_t s_row[SBV_SWEEP_TILE * SBN_ROW_WORDS];
    __shared__ uint32_t s_at[SBV_SWEEP_TILE];
    __shared__ unsigned long long s_key[SBV_SWEEP_TILE];
    __shared__ uint32_t s_in[SBV_SWEEP_TILE * 2u];
    const uint32_t rows = *n_list, total = *total_dev;
    if (rows == 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t base = 0u; base < rows; base += SBV_SWEEP_TILE) {
        const uint32_t tile = min(SBV_SWEEP_TILE, rows - base);
        __syncthreads(); // (the tile before has been read)
        for (uint32_t i = threadIdx.x; i < tile * SBN_ROW_WORDS; i += SBV_BLOCK) s_row[i] = points[(size_t)list[base + i / SBN_ROW_WORDS] * SBN_ROW_WORDS + i % SBN_ROW_WORDS];
        if (threadIdx.x < SBV_SWEEP_TILE) {
            s_at[threadIdx.x] = threadIdx.x < tile ? list[base + threadIdx.x] : 0u;
            s_key[threadIdx.x] = SBN_NO_KEY, s_in[2u * threadIdx.x] = 0u, s_in[2u * threadIdx.x + 1u] = 0u;
        }
        __syncthreads();
        SbvBest mine{SBN_NO_KEY, 0u, 0u}; // lane k: row k of the tile over all records of this wave
        for (uint32_t q0 = blockIdx.x * SBV_BLOCK; q0 < total; q0 += gridDim.x * SBV_BLOCK) {
            const uint32_t q = q0 + threadIdx.x;
            const bool have = q < total;
            const srw::Rec c = have ? sorted[q] : srw::Rec{0.0f, 0.0f, 0.0f, 0.0f, 0u, 0u};
            const bool beam = (c.index & SRW_KIND_BIT) != 0u;
            for (uint32_t k = 0u; k < tile; k++) {
                const uint64_t key = have ? sbv_meet(sbn::probe_of(s_row + k * SBN_ROW_WORDS), c, labels) : SBN_NO_KEY;
                const unsigned long long kept = __ballot(key != SBN_NO_KEY);
                if (!kept) continue; // (uniform over the wave)
                const uint32_t beams = (uint32_t)__popcll(__ballot(key != SBN_NO_KEY && beam));
                const unsigned long long least = sbv_wave_min(key);
                if (lane == k) mine.key = sbn::nearer(mine.key, least), mine.in_b += beams, mine.in_p += (uint32_t)__popcll(kept) - beams;
            }
        }
        if (lane < tile) { // the workgroup's four waves meet in LDS
            if (mine.key != SBN_NO_KEY) atomicMin(&s_key[lane], (unsigned long long)mine.key);
            if (mine.in_p) atomicAdd(&s_in[2u * lane], mine.in_p);
            if (mine.in_b) atomicAdd(&s_in[2u * lane + 1u], mine.in_b);
        }
        __syncthreads();
        if (threadIdx.x < tile) { // and the workgroups in memory
            const uint32_t j = s_at[threadIdx.x];
            if (s_key[threadIdx.x] != SBN_NO_KEY) atomicMin(&keys[j], s_key[threadIdx.x]);
            if (within && s_in[2u * threadIdx.x]) atomicAdd(&within[2u * (size_t)j], s_in[2u * threadIdx.x]);
            if (within && s_in[2u * threadIdx.x + 1u]) atomicAdd(&within[2u * (size_t)j + 1u], s_in[2u * threadIdx.x + 1u]);
        }
    }
}

// a thread per row: a valid row the sweep does not answer against the leftover list sorted[from .. to).  The row is this thread's
// alone by now (the walk is done, the sweep only touches swept rows): plain loads and stores.
__global__ __launch_bounds__(SBV_BLOCK) void k_near_leftover(const uint32_t *__restrict__ points, uint32_t n_points, const int32_t *__restrict__ labels,
                                                             const srw::Rec *__restrict__ sorted, const uint32_t *__restrict__ end, uint32_t cells,
                                                             const uint8_t *__restrict__ swept_of, unsigned long long *__restrict__ keys,
                                                             uint2 *__restrict__ within)
{
    const uint32_t j = blockIdx.x * SBV_BLOCK + threadIdx.x;
    const uint32_t from = end[cells - 1u], to = end[cells];
    if (j >= n_points || from >= to || swept_of[j]) return;
    uint32_t w[SBN_ROW_WORDS];
    sbv_load_row(points, j, w);
    if (sbn::row_verdict(w, labels != nullptr) != sbn::MISS) return;
    const sbn::Probe p = sbn::probe_of(w);
    if (!(p.mask & (sbn::MASK_PARTICLES | sbn::MASK_BEAMS))) return;
    SbvBest b{SBN_NO_KEY, 0u, 0u};
    for (uint32_t q = from; q < to; q++) b.take(p, sorted[q], labels);
    if (b.key < keys[j]) keys[j] = b.key;
    if (within && (b.in_p | b.in_b)) {
        const uint2 in = within[j];
        within[j] = make_uint2(in.x + b.in_p, in.y + b.in_b);
    }
}

// pinv: per particle data index < np its slot in pos (SBV_NONE: none); ends: per beam data index < nd the data indices of A and B
__global__ __launch_bounds__(SBV_BLOCK) void k_near_finish(const uint32_t *__restrict__ points, uint32_t n_points, const int32_t *__restrict__ labels,
                                                           const unsigned long long *__restrict__ keys, const uint2 *__restrict__ within,
                                                           const uint32_t *__restrict__ pinv, uint32_t np, const float2 *__restrict__ pos,
                                                           const uint2 *__restrict__ ends, uint32_t nd, uint32_t max_particles, float bounds,
                                                           uint32_t *out_d, int32_t *out_hit, uint32_t *out_point, int32_t *out_within,
                                                           unsigned long long *acc)
{
    const uint32_t j = blockIdx.x * SBV_BLOCK + threadIdx.x;
    int32_t kind = sbn::EMPTY;
    if (j < n_points) {
        uint32_t w[SBN_ROW_WORDS];
        sbv_load_row(points, j, w);
        const int verdict = sbn::row_verdict(w, labels != nullptr);
        const uint64_t key = keys[j];
        kind = sbn::out_kind_wide(verdict, key);
        const int32_t index = sbn::out_index_wide(verdict, key);
        if (out_d) out_d[j] = sbn::out_d(verdict, key, w[3]);
        uint2 ab = make_uint2(SBV_NONE, SBV_NONE); // the winning beam's endpoints, by data index
        if (kind == sbn::BEAM && ends && (uint32_t)index < nd) ab = ends[index];
        if (out_hit) {
            int32_t label = -1;
            if (labels && (kind == sbn::PARTICLE || kind == sbn::BEAM)) {
                const uint32_t a = kind == sbn::BEAM ? ab.x : (uint32_t)index; // the particle whose label it is
                if (a < max_particles) label = labels[a];
            }
            int32_t *h = out_hit + (size_t)j * SBN_HIT_WORDS;
            h[0] = kind, h[1] = index, h[2] = label;
        }
        if (out_point) {
            float qx = 0.0f, qy = 0.0f; // (an empty or invalid row)
            if (verdict == sbn::MISS) {
                const sbn::Probe p = sbn::probe_of(w);
                qx = p.px, qy = p.py; // (a miss: the query point's bits)
                if (kind == sbn::PARTICLE && (uint32_t)index < np && pinv[index] != SBV_NONE) {
                    const float2 c = pos[pinv[index]];
                    qx = c.x, qy = c.y;
                } else if (kind == sbn::BEAM && ab.x < np && ab.y < np && pinv[ab.x] != SBV_NONE && pinv[ab.y] != SBV_NONE) {
                    const float2 pa = pos[pinv[ab.x]], pb = pos[pinv[ab.y]];
                    sbn::segment_q(p, pa.x, pa.y, pb.x, pb.y, &qx, &qy);
                } else if (kind == sbn::WALL) {
                    sbn::wall_q(p, bounds, (uint32_t)index, &qx, &qy);
                }
            }
            out_point[2u * (size_t)j] = __float_as_uint(qx), out_point[2u * (size_t)j + 1u] = __float_as_uint(qy);
        }
        if (out_within) {
            const uint2 in = within[j];
            out_within[2u * (size_t)j] = (int32_t)in.x, out_within[2u * (size_t)j + 1u] = (int32_t)in.y;
        }
    }
    if (!acc) return; // (uniform)
    sbw_count(acc, SBV_A_VALID, kind >= 0);
    sbw_count(acc, SBV_A_PART, kind == sbn::PARTICLE);
    sbw_count(acc, SBV_A_BEAM, kind == sbn::BEAM);
    sbw_count(acc, SBV_A_WALL, kind == sbn::WALL);
}

__global__ __launch_bounds__(64) void k_near_counts(const unsigned long long *__restrict__ acc, long long *counts)
{
    if (threadIdx.x < SBV_NACC) counts[threadIdx.x] = threadIdx.x == SBV_A_ZERO ? 0ll : (long long)acc[threadIdx.x];
}

// ---------------------------------------------------------------- host side

static size_t sbv_up(size_t bytes) { return (bytes + 255u) & ~(size_t)255u; }

static sb_status sbv_enqueue(sb_engine *e, const sb_nearest_options *o, const void *points, uint32_t n_points, const void *labels, void *d, void *hit,
                             void *point, void *within, void *counts, bool host)
{
    if (!e) return SB_ERR_INVALID;
    const char *what = host ? "sb_nearest" : "sb_nearest_device";
    uint32_t cells_per_side = 0u, max_rings = SNW_DEFAULT_RINGS;
    if (o && o->struct_size == sizeof(sb_nearest_options)) {
        if (o->flags) SB_FAIL(e, SB_ERR_INVALID, "%s: flags 0x%x: no flag is defined", what, o->flags);
        cells_per_side = o->cells_per_side;
        if (cells_per_side > SRW_MAX_CELLS_PER_SIDE) SB_FAIL(e, SB_ERR_INVALID, "%s: cells_per_side %u, at most %u", what, cells_per_side, SRW_MAX_CELLS_PER_SIDE);
        if (o->max_rings > SNW_MAX_RINGS) SB_FAIL(e, SB_ERR_INVALID, "%s: max_rings %u, at most %u", what, o->max_rings, SNW_MAX_RINGS);
        if (o->max_rings) max_rings = o->max_rings;
    }
    if (n_points && !points) SB_FAIL(e, SB_ERR_INVALID, "%s: null points", what);
    if (!d && !hit && !point && !within && !counts) SB_FAIL(e, SB_ERR_INVALID, "%s: d, hit, point, within and counts are all null: nothing to write", what);
    if (((uintptr_t)points | (uintptr_t)labels | (uintptr_t)d | (uintptr_t)hit | (uintptr_t)point | (uintptr_t)within) & 3u)
        SB_FAIL(e, SB_ERR_INVALID, "%s: points, labels, d, hit, point and within must be 4-byte aligned", what);
    if ((uintptr_t)counts & 7u) SB_FAIL(e, SB_ERR_INVALID, "%s: counts must be 8-byte aligned", what);
    if (n_points > SBV_MAX_POINTS) SB_FAIL(e, SB_ERR_INVALID, "%s: %u points, at most 2^24 in a call", what, n_points);
    SB_TRY(sbq_preflight(e, what, o, "handled", "points across ranks are not handled"));
    if (e->opt.max_particles > (1u << SBN_WIDE_INDEX_BITS) || e->opt.max_beams > (1u << SBN_WIDE_INDEX_BITS))
        SB_FAIL(e, SB_ERR_UNSUPPORTED, "%s: capacities above 2^30 do not fit the key's index", what);
    if (n_points == 0u) return SB_OK; // nothing is asked
    SB_TRY(sbq_need(e, what, SBQ_PARTICLES | SBQ_BEAMS | SBQ_COPIES));
    SbStateIoState &s = *e->sio;
    if (!s.cut_valid) SB_TRY(sbx_build_rows(e, what));

    const srw::Grid g = sbw_grid(e, cells_per_side);
    const uint32_t np = s.np, n = s.nslots, maxP = e->opt.max_particles, nd = s.cut_nd, cells = g.G * g.G;
    const SbwSortPlan plan = sbw_sort_plan(e, g.G);
    const bool want_ends = (hit && labels) || point;
    // the call's scratch, one block: the accumulators, the sweep's row count and the scan's total; the bins; the scan's block sums;
    // the records; per row its key, its within pair, its swept mark and its place on the sweep's list; per beam data index its endpoints
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t o0 = at; at += sbv_up(bytes); return o0; };
    const size_t o_acc = take(SBV_NACC * 8 + 8), o_cells = take(plan.nbin * 4), o_bsum = take(plan.nb_scan * 4),
                 o_sorted = take(plan.items * sizeof(srw::Rec)), o_keys = take((size_t)n_points * 8), o_within = take(within ? (size_t)n_points * 8 : 0),
                 o_swept = take(n_points), o_list = take((size_t)n_points * 4), o_ends = take(want_ends ? (size_t)nd * 8 : 0);
    SB_TRY(s.buf[SBV_B_SCRATCH].grow(e, at));
    unsigned char *base = s.buf[SBV_B_SCRATCH].as<unsigned char>();
    unsigned long long *acc = (unsigned long long *)(base + o_acc), *keys = (unsigned long long *)(base + o_keys);
    uint32_t *n_list = (uint32_t *)(acc + SBV_NACC), *total = n_list + 1, *d_cells = (uint32_t *)(base + o_cells), *bsum = (uint32_t *)(base + o_bsum);
    uint32_t *list = (uint32_t *)(base + o_list);
    uint2 *in = within ? (uint2 *)(base + o_within) : nullptr, *ends = want_ends ? (uint2 *)(base + o_ends) : nullptr;
    uint8_t *swept_of = (uint8_t *)(base + o_swept);
    srw::Rec *sorted = (srw::Rec *)(base + o_sorted);

    SbqMirror mir(e, host);
    const uint32_t *d_points = mir.in<uint32_t>(SBV_B_POINTS, points, (size_t)n_points * sizeof(sb_batch_near_point), (size_t)n_points * sizeof(sb_batch_near_point));
    const int32_t *d_labels = mir.in<int32_t>(SBV_B_LABELS, labels, (size_t)maxP * 4, (size_t)maxP * 4);
    uint32_t *d_d = mir.out<uint32_t>(SBV_B_D, d, (size_t)n_points * 4);
    int32_t *d_hit = mir.out<int32_t>(SBV_B_HIT, hit, (size_t)n_points * SBN_HIT_WORDS * 4);
    uint32_t *d_point = mir.out<uint32_t>(SBV_B_POINT, point, (size_t)n_points * 8);
    int32_t *d_within = mir.out<int32_t>(SBV_B_WITHIN, within, (size_t)n_points * 8);
    long long *d_counts = mir.out<long long>(SBV_B_COUNTS, counts, SB_NEAREST_COUNT_WORDS * 8);
    SB_TRY(mir.st);

    auto blocks = [](uint64_t k) { return (uint32_t)((k + SBV_BLOCK - 1u) / SBV_BLOCK); };
    const uint32_t *d_pinv = s.buf[SBQ_B_PINV].as<uint32_t>(), *d_tab = s.buf[SBQ_B_TAB].as<uint32_t>(), *d_row = s.buf[SBX_B_ROW].as<uint32_t>();
    SB_TRY(sbw_sort(e, g, acc, SBV_NACC * 8 + 8, d_cells, bsum, sorted, nullptr, total));
    if (ends && n) k_near_ends<<<blocks(n), SBV_BLOCK, 0, e->stream>>>(d_tab, n, d_row, nd, ends);
    k_near_walk<<<blocks(n_points), SBV_BLOCK, 0, e->stream>>>(d_points, n_points, d_labels, sorted, d_cells, g, max_rings, keys, in, swept_of, list, n_list, acc);
    k_near_sweep<<<SBV_SWEEP_BLOCKS, SBV_BLOCK, 0, e->stream>>>(d_points, d_labels, sorted, total, list, n_list, keys, (uint32_t *)in);
    k_near_leftover<<<blocks(n_points), SBV_BLOCK, 0, e->stream>>>(d_points, n_points, d_labels, sorted, d_cells, cells, swept_of, keys, in);
    k_near_finish<<<blocks(n_points), SBV_BLOCK, 0, e->stream>>>(d_points, n_points, d_labels, keys, in, d_pinv, np, e->part[e->cur].pos, ends, nd, maxP, g.bounds,
                                                                d_d, d_hit, d_point, d_within, d_counts ? acc : nullptr);
    if (d_counts) k_near_counts<<<1, 64, 0, e->stream>>>(acc, d_counts);
    SB_HIP(e, hipGetLastError());
    return mir.finish();
}

// what sb_get_info reads ("nearest_cells_per_side", "nearest_max_rings", "nearest_kernel_vgprs", "nearest_kernel_scratch_bytes")
bool sbv_info(sb_engine *e, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "nearest_cells_per_side") *value = sbw_grid(e, 0u).G; // the default rule on the scene as it is now
    else if (k == "nearest_max_rings") *value = SNW_DEFAULT_RINGS;
    else if (k == "nearest_kernel_vgprs" || k == "nearest_kernel_scratch_bytes") {
        std::vector<const void *> ks = {(const void *)k_near_ends, (const void *)k_near_walk, (const void *)k_near_sweep, (const void *)k_near_leftover,
                                        (const void *)k_near_finish, (const void *)k_near_counts};
        for (const void *f : sbw_sort_kernels()) ks.push_back(f);
        return sbq_kernel_most(e, ks, k == "nearest_kernel_vgprs", value);
    }
    else return false;
    return true;
}

extern "C" {

sb_status sb_nearest_device(sb_engine *e, const sb_nearest_options *opts, const void *device_points, uint32_t n_points, const void *device_labels_i32,
                            void *device_d_f32, void *device_hit_i32, void *device_point_f32, void *device_within_i32, void *device_counts_i64)
{
    SB_GUARDED(e, sbv_enqueue(e, opts, device_points, n_points, device_labels_i32, device_d_f32, device_hit_i32, device_point_f32, device_within_i32,
                              device_counts_i64, false))
}

sb_status sb_nearest(sb_engine *e, const sb_nearest_options *opts, const sb_batch_near_point *points, uint32_t n_points, const int32_t *labels, float *d,
                     int32_t *hit, float *point, int32_t *within, int64_t *counts)
{
    SB_GUARDED(e, sbv_enqueue(e, opts, points, n_points, labels, d, hit, point, within, counts, true))
}

} // extern "C"
