// sb_raycast.hip -- range sensors over the whole scene of an sb_engine: for every ray the nearest hit among the particles (discs),
// the live beams (segments) and the four walls, found on the device (sb_raycast / sb_raycast_device of include/softbody.h; gfx950,
// wave64).
//
// The definition is sb_batch_raycast_device's, word for word: the meetings of sb_batch_ray_math.h, the winner the smallest key --
// here the WIDE key (bits(t) << 32 | kind << 30 | index), the same order with room for 2^30 indices.  k_batch_raycast tests every
// ray against every primitive in LDS; here the scene lies in HBM, so the primitives are sorted into the cells of sb_ray_walk.h and
// a ray looks only into the cells that header proves sufficient.  One launch per stage, all on the engine's stream:
//   k_ray_bin       a thread per particle data index and per caller beam slot: its bin (a cell; the leftover list for what is
//                   outside the grid or longer than two cells), one atomicAdd on the bin's count; counts words 5 and 6
//   sbq_scan        exclusive scan of the G^2 + 2 counts
//   k_ray_bin again the record {coordinates, data index, label source} to the next place of its bin (the order inside a bin is the
//                   one thing the atomics decide; a minimum over keys does not observe it)
//   k_ray_walk      a thread per ray: the row's verdict, the walls, and for a walkable row srw::walk over the cells; a valid row that
//                   is not walkable is put on the sweep's list (device memory: no read-back)
//   k_ray_sweep     a fixed grid strides over ALL records, each against the listed rows, which go through LDS a tile at a time
//                   (nothing to do: it returns at once)
//   k_ray_leftover  a thread per ray: every valid row against the leftover list
//   k_ray_finish    a thread per ray: the smallest key into t and the hit row; counts words 0 .. 3 by ballots
//   k_ray_counts    the eight int64 words
// The three producers meet in one 64-bit atomicMin per ray and key found.  Nothing of the engine is written, nothing is read back,
// no workgroup waits for another.
#include <algorithm>
#include <string>
#include <vector>

#include "sb_report.h"
#include "sb_batch.h" // sb_batch_cell_geometry: the cell side's rule
#include "sb_ray_walk.h"

#define SBW_BLOCK 256u
#define SBW_SWEEP_BLOCKS 1024u
#define SBW_MAX_RAYS (1u << 24)
#define SBW_NONE 0xFFFFFFFFu
enum { SBW_A_VALID, SBW_A_PART, SBW_A_BEAM, SBW_A_WALL, SBW_A_SWEPT, SBW_A_OUTSIDE, SBW_A_LONG, SBW_A_ZERO, SBW_NACC }; // = the count words

static_assert(SB_RAYCAST_COUNT_WORDS == SBW_NACC, "an accumulator per count word");
static_assert(sizeof(sb_batch_ray) == SBR_ROW_WORDS * 4u && sizeof(srw::Rec) == 24u, "the row and the record");

// threads [0, np): particle data indices; [np, np + n): caller beam slots.  tab: [4][n] = data index of A, of B, engine slot, copy.
// scatter == 0: count the bins; 1: place the records (the same bins: nothing moves between the two launches).
__global__ __launch_bounds__(SBW_BLOCK) void k_ray_bin(const uint32_t *__restrict__ pinv, uint32_t np, const float2 *__restrict__ pos,
                                                       const uint32_t *__restrict__ tab, uint32_t n, const uint32_t *__restrict__ row,
                                                       const uint32_t *__restrict__ dead, uint32_t max_beams, srw::Grid g, uint32_t scatter,
                                                       uint32_t *count, srw::Rec *sorted, uint32_t *a_of, uint32_t nd,
                                                       unsigned long long *acc)
{
    const uint32_t i = blockIdx.x * SBW_BLOCK + threadIdx.x;
    uint32_t bin = SBW_NONE;
    srw::Rec rec{0.0f, 0.0f, 0.0f, 0.0f, 0u, 0u};
    bool beam = false;
    if (i < np) {
        const uint32_t p = pinv[i];
        if (p != SBW_NONE) {
            const float2 c = pos[p];
            rec.ax = c.x, rec.ay = c.y, rec.index = i, rec.lsrc = i;
            bin = srw::particle_bin(c.x, c.y, g);
        }
    } else if (i - np < n) {
        const uint32_t u = i - np, slot = tab[2u * (size_t)n + u], a = tab[u], b = tab[(size_t)n + u], d = row[u];
        // (the table builders refuse a scene whose endpoints are not live particles below np; d is checked against the capacity here)
        if (!(dead && dead[slot] != 0u) && d < max_beams && a < np && b < np) {
            const float2 pa = pos[pinv[a]], pb = pos[pinv[b]];
            rec.ax = pa.x, rec.ay = pa.y, rec.bx = pb.x, rec.by = pb.y, rec.index = d | SRW_KIND_BIT, rec.lsrc = a;
            bin = srw::beam_bin(pa.x, pa.y, pb.x, pb.y, g);
            beam = true;
            if (!scatter && a_of && d < nd) a_of[d] = a;
        }
    }
    if (!scatter) {
        const uint32_t run = sbq_run_length(bin, bin != SBW_NONE);
        if (run) atomicAdd(&count[bin], run);
        const bool left = bin == g.G * g.G;
        sbw_count(acc, SBW_A_OUTSIDE, left && !beam);
        sbw_count(acc, SBW_A_LONG, left && beam);
    } else if (bin != SBW_NONE) {
        sorted[atomicAdd(&count[bin], 1u)] = rec; // (count: the scan's starts; every bin's END is left in its word)
    }
}

// one record against one row: the wide key, SBR_NO_KEY where the mask, the label or the test leaves it out
SB_DEV uint64_t sbw_meet(const sbr::Ray &r, const srw::Rec &c, float r2, const int32_t *__restrict__ labels)
{
    const bool beam = (c.index & SRW_KIND_BIT) != 0u;
    if (!(r.mask & (beam ? sbr::MASK_BEAMS : sbr::MASK_PARTICLES))) return SBR_NO_KEY;
    if (r.skip != -1 && labels && labels[c.lsrc] == r.skip) return SBR_NO_KEY;
    const uint32_t index = c.index & ~SRW_KIND_BIT;
    return beam ? sbr::segment_wide(r, c.ax, c.ay, c.bx, c.by, index) : sbr::disc_wide(r, c.ax, c.ay, r2, index);
}

SB_DEV void sbw_load_row(const uint32_t *__restrict__ rays, uint32_t j, uint32_t *w)
{
    const uint32_t *row = rays + (size_t)j * SBR_ROW_WORDS; // (the caller's rows need only be 4-byte aligned)
#pragma unroll
    for (uint32_t i = 0; i < SBR_ROW_WORDS; i++) w[i] = row[i];
}

// end: per bin the END of its records (bin 0 starts at 0)
__global__ __launch_bounds__(SBW_BLOCK) void k_ray_walk(const uint32_t *__restrict__ rays, uint32_t n_rays, const int32_t *__restrict__ labels,
                                                        const srw::Rec *__restrict__ sorted, const uint32_t *__restrict__ end, srw::Grid g,
                                                        unsigned long long *keys, uint32_t *list, uint32_t *n_list, unsigned long long *acc)
{
    const uint32_t j = blockIdx.x * SBW_BLOCK + threadIdx.x;
    bool swept = false;
    if (j < n_rays) {
        uint32_t w[SBR_ROW_WORDS];
        sbw_load_row(rays, j, w);
        if (sbr::row_verdict(w, labels != nullptr) == sbr::MISS) {
            const sbr::Ray r = sbr::ray_of(w);
            uint64_t key = (r.mask & sbr::MASK_WALLS) ? sbr::walls_wide(r, g.bounds) : SBR_NO_KEY;
            if (srw::walkable(r, g.bounds)) {
                const float r2 = g.radius * g.radius;
                srw::walk(
                    r, g,
                    [&](uint32_t first, uint32_t count, uint32_t stride) {
                        if (stride == 1u) { // neighbouring bins: one run
                            const uint32_t to = end[first + count - 1u];
                            for (uint32_t q = first ? end[first - 1u] : 0u; q < to; q++) key = sbr::nearer(key, sbw_meet(r, sorted[q], r2, labels));
                        } else {
                            for (uint32_t k = 0u, c = first; k < count; k++, c += stride) {
                                const uint32_t to = end[c];
                                for (uint32_t q = c ? end[c - 1u] : 0u; q < to; q++) key = sbr::nearer(key, sbw_meet(r, sorted[q], r2, labels));
                            }
                        }
                    },
                    [&]() { return key == SBR_NO_KEY ? -1.0f : sbr::word_as_float((uint32_t)(key >> 32)); });
            } else {
                swept = true;
                list[atomicAdd(n_list, 1u)] = j;
            }
            if (key != SBR_NO_KEY) atomicMin(&keys[j], (unsigned long long)key);
        }
    }
    sbw_count(acc, SBW_A_SWEPT, swept);
}

// a fixed grid over all `total` records (*total_dev: the scan's sum), each against the listed rows.  The rows go through LDS a tile at a
// time (every thread of the workgroup meets the same rows); a thread's records are read again per tile, not its rows per record.
#define SBW_SWEEP_TILE 64u
__global__ __launch_bounds__(SBW_BLOCK) void k_ray_sweep(const uint32_t *__restrict__ rays, const int32_t *__restrict__ labels,
                                                         const srw::Rec *__restrict__ sorted, const uint32_t *__restrict__ total_dev, float radius,
                                                         const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list, unsigned long long *keys)
{
    __shared__ uint32_t s_row[SBW_SWEEP_TILE * SBR_ROW_WORDS];
    __shared__ uint32_t s_ray[SBW_SWEEP_TILE];
    const uint32_t rows = *n_list, total = *total_dev; // (uniform: every thread takes the same trips and meets every barrier)
    if (rows == 0u) return;
    const float r2 = radius * radius;
    for (uint32_t base = 0u; base < rows; base += SBW_SWEEP_TILE) {
        const uint32_t tile = min(SBW_SWEEP_TILE, rows - base);
        __syncthreads(); // (the tile before has been read)
        for (uint32_t i = threadIdx.x; i < tile * SBR_ROW_WORDS; i += SBW_BLOCK) s_row[i] = rays[(size_t)list[base + i / SBR_ROW_WORDS] * SBR_ROW_WORDS + i % SBR_ROW_WORDS];
        if (threadIdx.x < tile) s_ray[threadIdx.x] = list[base + threadIdx.x];
        __syncthreads();
        for (uint32_t q = blockIdx.x * SBW_BLOCK + threadIdx.x; q < total; q += gridDim.x * SBW_BLOCK) {
            const srw::Rec c = sorted[q];
            for (uint32_t k = 0u; k < tile; k++) {
                const uint64_t key = sbw_meet(sbr::ray_of(s_row + k * SBR_ROW_WORDS), c, r2, labels);
                if (key != SBR_NO_KEY) atomicMin(&keys[s_ray[k]], (unsigned long long)key);
            }
        }
    }
}

// a thread per ray: a valid, walkable row against the leftover list sorted[from .. to) (the listed rows met it in the sweep)
__global__ __launch_bounds__(SBW_BLOCK) void k_ray_leftover(const uint32_t *__restrict__ rays, uint32_t n_rays, const int32_t *__restrict__ labels,
                                                            const srw::Rec *__restrict__ sorted, const uint32_t *__restrict__ end, uint32_t cells,
                                                            float bounds, float radius, unsigned long long *keys)
{
    const uint32_t j = blockIdx.x * SBW_BLOCK + threadIdx.x;
    const uint32_t from = end[cells - 1u], to = end[cells];
    if (j >= n_rays || from >= to) return;
    uint32_t w[SBR_ROW_WORDS];
    sbw_load_row(rays, j, w);
    if (sbr::row_verdict(w, labels != nullptr) != sbr::MISS) return;
    const sbr::Ray r = sbr::ray_of(w);
    if (!srw::walkable(r, bounds) || !(r.mask & (sbr::MASK_PARTICLES | sbr::MASK_BEAMS))) return;
    const float r2 = radius * radius;
    uint64_t key = SBR_NO_KEY;
    for (uint32_t q = from; q < to; q++) key = sbr::nearer(key, sbw_meet(r, sorted[q], r2, labels));
    if (key != SBR_NO_KEY) atomicMin(&keys[j], (unsigned long long)key);
}

__global__ __launch_bounds__(SBW_BLOCK) void k_ray_finish(const uint32_t *__restrict__ rays, uint32_t n_rays, const int32_t *__restrict__ labels,
                                                          const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ a_of, uint32_t nd,
                                                          uint32_t max_particles, uint32_t *out_t, int32_t *out_hit, unsigned long long *acc)
{
    const uint32_t j = blockIdx.x * SBW_BLOCK + threadIdx.x;
    int32_t kind = sbr::EMPTY;
    if (j < n_rays) {
        uint32_t w[SBR_ROW_WORDS];
        sbw_load_row(rays, j, w);
        const int verdict = sbr::row_verdict(w, labels != nullptr);
        const uint64_t key = keys[j];
        kind = sbr::out_kind_wide(verdict, key);
        if (out_t) out_t[j] = sbr::out_t(verdict, key, w[5]);
        if (out_hit) {
            const int32_t index = sbr::out_index_wide(verdict, key);
            int32_t label = -1;
            if (labels && (kind == sbr::PARTICLE || kind == sbr::BEAM)) {
                uint32_t p = (uint32_t)index; // the particle whose label it is: the hit one, or the hit beam's endpoint A
                if (kind == sbr::BEAM) p = p < nd ? a_of[p] : max_particles;
                if (p < max_particles) label = labels[p];
            }
            int32_t *h = out_hit + (size_t)j * SBR_HIT_WORDS;
            h[0] = kind, h[1] = index, h[2] = label;
        }
    }
    if (!acc) return; // (uniform)
    sbw_count(acc, SBW_A_VALID, kind >= 0);
    sbw_count(acc, SBW_A_PART, kind == sbr::PARTICLE);
    sbw_count(acc, SBW_A_BEAM, kind == sbr::BEAM);
    sbw_count(acc, SBW_A_WALL, kind == sbr::WALL);
}

__global__ __launch_bounds__(64) void k_ray_counts(const unsigned long long *__restrict__ acc, long long *counts)
{
    if (threadIdx.x < SBW_NACC) counts[threadIdx.x] = threadIdx.x == SBW_A_ZERO ? 0ll : (long long)acc[threadIdx.x];
}

// ---------------------------------------------------------------- host side

// The grid of a call: the largest G <= cap (cells_per_side, or the default rule's) whose cells are at least 2r (1 + 1/64) wide
// (sb_batch_cell_geometry); one cell where radius or bounds are no numbers sb_ray_walk.h's derivation covers.
srw::Grid sbw_grid(const sb_engine *e, uint32_t cells_per_side)
{
    srw::Grid g{1u, 1.0f, e->prm.bounds_size, e->prm.particle_radius};
    float cell = 1.0f;
    const uint32_t cap = cells_per_side ? cells_per_side : srw::default_cap(e->P);
    const uint32_t G = srw::ordinary(g.bounds, g.radius) ? sb_batch_cell_geometry(g.bounds, g.radius, cap, &cell) : 0u;
    if (G) g.G = G, g.cell = cell;
    else g.cell = g.bounds > 0.0f ? g.bounds : 1.0f;
    return g;
}

static size_t sbw_up(size_t bytes) { return (bytes + 255u) & ~(size_t)255u; }

SbwSortPlan sbw_sort_plan(const sb_engine *e, uint32_t G)
{
    const SbStateIoState &s = *e->sio;
    SbwSortPlan p;
    p.nbin = (uint64_t)G * G + 2u, p.nb_scan = (p.nbin + SBQ_SCAN - 1u) / SBQ_SCAN, p.items = (uint64_t)s.np + s.nslots;
    return p;
}

// The counting sort of the scene into the cells of g, enqueued on the engine's stream (sb_report.h; sb_nearest.hip calls it too):
// the accumulators (acc_bytes: the count words and what the caller keeps behind them), the bins and a_of cleared, k_ray_bin,
// sbq_scan, k_ray_bin again.  It needs the shared scene tables and sbx_build_rows' rows.
sb_status sbw_sort(sb_engine *e, const srw::Grid &g, unsigned long long *acc, size_t acc_bytes, uint32_t *d_cells, uint32_t *bsum, srw::Rec *sorted,
                   uint32_t *a_of, uint32_t *total)
{
    SbStateIoState &s = *e->sio;
    const uint32_t np = s.np, n = s.nslots, maxB = e->opt.max_beams, nd = s.cut_nd;
    const SbwSortPlan plan = sbw_sort_plan(e, g.G);
    const uint32_t *d_pinv = s.buf[SBQ_B_PINV].as<uint32_t>(), *d_tab = s.buf[SBQ_B_TAB].as<uint32_t>(), *d_row = s.buf[SBX_B_ROW].as<uint32_t>();
    const float2 *pos = e->part[e->cur].pos;
    const uint32_t blocks = (uint32_t)((plan.items + SBW_BLOCK - 1u) / SBW_BLOCK);
    SB_HIP(e, hipMemsetAsync(acc, 0, acc_bytes, e->stream));
    SB_HIP(e, hipMemsetAsync(d_cells, 0, plan.nbin * 4, e->stream));
    if (a_of && nd) SB_HIP(e, hipMemsetAsync(a_of, 0xFF, (size_t)nd * 4, e->stream));
    if (plan.items)
        k_ray_bin<<<blocks, SBW_BLOCK, 0, e->stream>>>(d_pinv, np, pos, d_tab, n, d_row, sbq_dead(e), maxB, g, 0u, d_cells, sorted, a_of, nd, acc);
    sbq_scan<uint32_t>(e, d_cells, plan.nbin, bsum, d_cells, total);
    if (plan.items)
        k_ray_bin<<<blocks, SBW_BLOCK, 0, e->stream>>>(d_pinv, np, pos, d_tab, n, d_row, sbq_dead(e), maxB, g, 1u, d_cells, sorted, nullptr, nd, acc);
    return SB_OK;
}

std::vector<const void *> sbw_sort_kernels()
{
    std::vector<const void *> ks = {(const void *)k_ray_bin};
    for (const void *f : sbq_scan_kernels(false)) ks.push_back(f);
    return ks;
}

static sb_status sbw_enqueue(sb_engine *e, const sb_raycast_options *o, const void *rays, uint32_t n_rays, const void *labels, void *t, void *hit,
                             void *counts, bool host)
{
    if (!e) return SB_ERR_INVALID;
    const char *what = host ? "sb_raycast" : "sb_raycast_device";
    uint32_t cells_per_side = 0u;
    if (o && o->struct_size == sizeof(sb_raycast_options)) {
        if (o->flags) SB_FAIL(e, SB_ERR_INVALID, "%s: flags 0x%x: no flag is defined", what, o->flags);
        cells_per_side = o->cells_per_side;
        if (cells_per_side > SRW_MAX_CELLS_PER_SIDE) SB_FAIL(e, SB_ERR_INVALID, "%s: cells_per_side %u, at most %u", what, cells_per_side, SRW_MAX_CELLS_PER_SIDE);
    }
    if (n_rays && !rays) SB_FAIL(e, SB_ERR_INVALID, "%s: null rays", what);
    if (!t && !hit && !counts) SB_FAIL(e, SB_ERR_INVALID, "%s: t, hit and counts are all null: nothing to write", what);
    if (((uintptr_t)rays | (uintptr_t)labels | (uintptr_t)t | (uintptr_t)hit) & 3u)
        SB_FAIL(e, SB_ERR_INVALID, "%s: rays, labels, t and hit must be 4-byte aligned", what);
    if ((uintptr_t)counts & 7u) SB_FAIL(e, SB_ERR_INVALID, "%s: counts must be 8-byte aligned", what);
    if (n_rays > SBW_MAX_RAYS) SB_FAIL(e, SB_ERR_INVALID, "%s: %u rays, at most 2^24 in a call", what, n_rays);
    SB_TRY(sbq_preflight(e, what, o, "handled", "rays across ranks are not handled"));
    if (e->opt.max_particles > (1u << SBR_WIDE_INDEX_BITS) || e->opt.max_beams > (1u << SBR_WIDE_INDEX_BITS))
        SB_FAIL(e, SB_ERR_UNSUPPORTED, "%s: capacities above 2^30 do not fit the key's index", what);
    if (n_rays == 0u) return SB_OK; // nothing is asked
    SB_TRY(sbq_need(e, what, SBQ_PARTICLES | SBQ_BEAMS | SBQ_COPIES));
    SbStateIoState &s = *e->sio;
    if (!s.cut_valid) SB_TRY(sbx_build_rows(e, what));
    s.ray_build_ms = s.part_ms + s.beam_ms + s.copy_ms + s.cut_row_ms;

    const srw::Grid g = sbw_grid(e, cells_per_side);
    const uint32_t maxP = e->opt.max_particles, nd = s.cut_nd, cells = g.G * g.G;
    const SbwSortPlan plan = sbw_sort_plan(e, g.G);
    const bool want_a = labels && hit;
    // the call's scratch, one block: the accumulators, the sweep's row count and the scan's total, the bins, the scan's block sums,
    // the records, the keys, the sweep's rows, per beam data index its endpoint A
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t o0 = at; at += sbw_up(bytes); return o0; };
    const size_t o_acc = take(SBW_NACC * 8 + 8), o_cells = take(plan.nbin * 4), o_bsum = take(plan.nb_scan * 4),
                 o_sorted = take(plan.items * sizeof(srw::Rec)), o_keys = take((size_t)n_rays * 8), o_list = take((size_t)n_rays * 4),
                 o_aof = take(want_a ? (size_t)nd * 4 : 0);
    SB_TRY(s.buf[SBW_B_SCRATCH].grow(e, at));
    unsigned char *base = s.buf[SBW_B_SCRATCH].as<unsigned char>();
    unsigned long long *acc = (unsigned long long *)(base + o_acc), *keys = (unsigned long long *)(base + o_keys);
    uint32_t *n_list = (uint32_t *)(acc + SBW_NACC), *total = n_list + 1, *d_cells = (uint32_t *)(base + o_cells), *bsum = (uint32_t *)(base + o_bsum);
    uint32_t *list = (uint32_t *)(base + o_list), *a_of = want_a ? (uint32_t *)(base + o_aof) : nullptr;
    srw::Rec *sorted = (srw::Rec *)(base + o_sorted);

    SbqMirror mir(e, host);
    const uint32_t *d_rays = mir.in<uint32_t>(SBW_B_RAYS, rays, (size_t)n_rays * sizeof(sb_batch_ray), (size_t)n_rays * sizeof(sb_batch_ray));
    const int32_t *d_labels = mir.in<int32_t>(SBW_B_LABELS, labels, (size_t)maxP * 4, (size_t)maxP * 4);
    uint32_t *d_t = mir.out<uint32_t>(SBW_B_T, t, (size_t)n_rays * 4);
    int32_t *d_hit = mir.out<int32_t>(SBW_B_HIT, hit, (size_t)n_rays * SBR_HIT_WORDS * 4);
    long long *d_counts = mir.out<long long>(SBW_B_COUNTS, counts, SB_RAYCAST_COUNT_WORDS * 8);
    SB_TRY(mir.st);

    auto blocks = [](uint64_t k) { return (uint32_t)((k + SBW_BLOCK - 1u) / SBW_BLOCK); };
    SB_TRY(sbw_sort(e, g, acc, SBW_NACC * 8 + 8, d_cells, bsum, sorted, a_of, total));
    SB_HIP(e, hipMemsetAsync(keys, 0xFF, (size_t)n_rays * 8, e->stream)); // SBR_NO_KEY
    k_ray_walk<<<blocks(n_rays), SBW_BLOCK, 0, e->stream>>>(d_rays, n_rays, d_labels, sorted, d_cells, g, keys, list, n_list, acc);
    k_ray_sweep<<<SBW_SWEEP_BLOCKS, SBW_BLOCK, 0, e->stream>>>(d_rays, d_labels, sorted, total, g.radius, list, n_list, keys);
    k_ray_leftover<<<blocks(n_rays), SBW_BLOCK, 0, e->stream>>>(d_rays, n_rays, d_labels, sorted, d_cells, cells, g.bounds, g.radius, keys);
    k_ray_finish<<<blocks(n_rays), SBW_BLOCK, 0, e->stream>>>(d_rays, n_rays, d_labels, keys, a_of, nd, maxP, d_t, d_hit, d_counts ? acc : nullptr);
    if (d_counts) k_ray_counts<<<1, 64, 0, e->stream>>>(acc, d_counts);
    SB_HIP(e, hipGetLastError());
    return mir.finish();
}

// what sb_get_info reads ("raycast_cells_per_side", "raycast_kernel_vgprs", "raycast_kernel_scratch_bytes", "raycast_table_build_us")
bool sbw_info(sb_engine *e, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "raycast_cells_per_side") *value = sbw_grid(e, 0u).G; // the default rule on the scene as it is now
    else if (k == "raycast_table_build_us") *value = e->sio ? (uint64_t)(e->sio->ray_build_ms * 1000.0 + 0.5) : 0u;
    else if (k == "raycast_kernel_vgprs" || k == "raycast_kernel_scratch_bytes") {
        std::vector<const void *> ks = {(const void *)k_ray_walk, (const void *)k_ray_sweep, (const void *)k_ray_leftover, (const void *)k_ray_finish,
                                        (const void *)k_ray_counts};
        for (const void *f : sbw_sort_kernels()) ks.push_back(f);
        return sbq_kernel_most(e, ks, k == "raycast_kernel_vgprs", value);
    }
    else return false;
    return true;
}

extern "C" {

sb_status sb_raycast_device(sb_engine *e, const sb_raycast_options *opts, const void *device_rays, uint32_t n_rays, const void *device_labels_i32,
                            void *device_t_f32, void *device_hit_i32, void *device_counts_i64)
{
    SB_GUARDED(e, sbw_enqueue(e, opts, device_rays, n_rays, device_labels_i32, device_t_f32, device_hit_i32, device_counts_i64, false))
}

sb_status sb_raycast(sb_engine *e, const sb_raycast_options *opts, const sb_batch_ray *rays, uint32_t n_rays, const int32_t *labels, float *t,
                     int32_t *hit, int64_t *counts)
{
    SB_GUARDED(e, sbw_enqueue(e, opts, rays, n_rays, labels, t, hit, counts, true))
}

} // extern "C"
