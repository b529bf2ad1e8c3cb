// sb_contacts.hip -- who touches whom, and who touches a wall, in the whole scene of an sb_engine, found on the device (sb_contacts /
// sb_contacts_device of include/softbody.h; gfx950, wave64).
//
// The definition is sb_batch_contacts_device's, word for word: two distinct particles i, j TOUCH iff dist == 0 or
// dist < particle_radius * 2, dist = sb_length(xj - xi, yj - yi) of the current particle records (sb_touch of sb_contact_cells.h, the one
// test both files call), everything named by particle DATA index.
// k_batch_contacts holds a scene in the LDS of one workgroup; here the scene lies in HBM, and the call may only enqueue: nothing
// loops on a host read-back and no workgroup waits for another.  A counting sort by cell in global memory, one launch per stage:
//   k_contacts_bin      a thread per data index: the position (through the shared data index -> internal particle table, sb_report.hip, in
//                       the CURRENT particle arrays, as sb_summary.hip's leaf kernel finds it), its cell (sb_grid_coord over
//                       [0, bounds]^2: out-of-range and NaN coordinates clamp into edge cells), ONE atomicAdd on that cell's
//                       count per run of lanes with the same cell (sbc_count_runs); the defined row of every data index at which
//                       no particle lives, up to max_particles (the "fill" stage, fused: it depends on nothing)
//   sbq_scan            exclusive scan of the G^2 + 1 counts (sb_report.hip: three launches, no recursion, no workgroup waits)
//   k_contacts_scatter  sorted[atomicAdd(&start[cell], 1)] = {x, y, d}: every cell's END is left in its word; the order inside a
//                       cell is the one thing the atomics decide, and nothing below observes it
//   k_contacts_visit    a thread per sorted record (neighbouring lanes share cells: the nine cell runs hit in L2): the three rows
//                       of the 3 x 3 cells, columns x-1 .. x+1 of a row one run; partners, partners of another label, partners
//                       above, the smallest partner; touch[d], above[d]; the four counts by wave reduction, LDS, then one 64-bit
//                       global atomic per workgroup and word
//   k_contacts_list     (only with pairs) behind a 64-bit exclusive scan of above[] over the data indices (the same three
//                       launches): every particle whose place is below max_pairs writes its pairs j-ascending, by the batch's
//                       sweeps that keep the four smallest partners above the last one written; nothing at or behind max_pairs
//   k_contacts_tail / k_contacts_counts   {-1, -1} behind the last pair; the accumulators into the four int64 words
// Everything behind the float test is integers -- counts, minima, sums, a list ordered by its indices -- so neither the order
// inside a cell nor the schedule can change a bit.  The file only READS the engine: none of SbGrid's hash buffers, none of its
// decision state.  Cost: the sum over particles of the population of their 3 x 3 cells; a scene crowded into one cell is quadratic
// here, as it is in the step.
#include <algorithm>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "sb_scene_cells.h" // the cells of the whole scene: geometry, cell of a position, window, run counter (shared with sb_forces.hip)

#define SBC_BLOCK 256u

enum { SBC_PAIRS, SBC_CROSS, SBC_WALLED, SBC_TOUCHING, SBC_LISTED, SBC_NACC }; // accumulator words (unsigned long long)

struct SbcRec {
    float x, y;
    uint32_t d;
};

// grid over max(np, n_rows): bin (d < np where a particle lives) and fill (every other d < n_rows; n_rows = max_particles with
// touch, 0 without).  cell_of[d], d < np: the particle's cell, SBC_NONE where none lives (k_contacts_visit turns it into above[d]).
__global__ __launch_bounds__(SBC_BLOCK) void k_contacts_bin(const uint32_t *__restrict__ pinv, uint32_t np, const float2 *__restrict__ pos,
                                                            SbcGeo geo, uint32_t *count, uint32_t *cell_of, int32_t *touch,
                                                            uint32_t n_rows, int32_t no_label)
{
    const uint32_t d = blockIdx.x * SBC_BLOCK + threadIdx.x;
    uint32_t c = SBC_NONE;
    if (d < np) {
        const uint32_t i = pinv[d];
        if (i != SBC_NONE) {
            const float2 p = pos[i];
            c = sbc_cell(p.x, p.y, geo);
        }
        cell_of[d] = c;
    }
    sbc_count_runs(count, c);
    if (c == SBC_NONE && d < n_rows) {
        int32_t *t = touch + (size_t)d * SB_CONTACT_WORDS;
        t[0] = 0, t[1] = no_label, t[2] = 0, t[3] = -1;
    }
}

// a thread per data index: its record to the next place of its cell
__global__ __launch_bounds__(SBC_BLOCK) void k_contacts_scatter(const uint32_t *__restrict__ pinv, uint32_t np, const float2 *__restrict__ pos,
                                                                uint32_t *cell_of, uint32_t *start, SbcRec *sorted)
{
    const uint32_t d = blockIdx.x * SBC_BLOCK + threadIdx.x;
    if (d >= np) return;
    const uint32_t c = cell_of[d];
    if (c == SBC_NONE) {
        cell_of[d] = 0u; // (the word becomes above[d]: nobody lives here, nothing is listed)
        return;
    }
    const float2 p = pos[pinv[d]];
    SbcRec r;
    r.x = p.x, r.y = p.y, r.d = d;
    sorted[atomicAdd(&start[c], 1u)] = r;
}

struct SbcTest {
    float two_r, thr, lo, hi;
};

__global__ __launch_bounds__(SBC_BLOCK) void k_contacts_visit(const SbcRec *__restrict__ sorted, uint32_t P, const uint32_t *__restrict__ end,
                                                              SbcGeo geo, SbcTest ts, const int32_t *__restrict__ labels, uint32_t other_body,
                                                              int32_t *touch, uint32_t *above_of, unsigned long long *acc)
{
    __shared__ unsigned long long s_acc[4];
    const uint32_t tid = threadIdx.x, k = blockIdx.x * SBC_BLOCK + tid;
    if (tid < 4u) s_acc[tid] = 0ull;
    __syncthreads();
    uint32_t n = 0u, cross = 0u, above = 0u, above_cross = 0u, wall = 0u;
    if (k < P) {
        const SbcRec me = sorted[k];
        const int32_t my_lab = labels ? labels[me.d] : 0;
        const SbCellWindow w = sbc_window(me.x, me.y, geo);
        uint32_t first = SBC_NONE;
        for (uint32_t yy = w.y0; yy <= w.y1; yy++) {
            uint32_t from, to;
            w.run(end, yy, &from, &to);
            for (uint32_t q = from; q < to; q++) {
                const SbcRec o = sorted[q];
                if (o.d == me.d || !sb_touch(make_float2(me.x, me.y), make_float2(o.x, o.y), ts.thr, ts.two_r)) continue;
                const uint32_t differs = labels && labels[o.d] != my_lab ? 1u : 0u, up = o.d > me.d ? 1u : 0u;
                n++;
                cross += differs;
                above += up;
                above_cross += up & differs;
                first = min(first, o.d);
            }
        }
        wall = (me.x <= ts.lo ? SB_BATCH_WALL_LEFT : 0u) | (me.x >= ts.hi ? SB_BATCH_WALL_RIGHT : 0u) | (me.y <= ts.lo ? SB_BATCH_WALL_LOW : 0u) |
               (me.y >= ts.hi ? SB_BATCH_WALL_HIGH : 0u); // (NaN: no bit)
        if (touch) {
            int32_t *t = touch + (size_t)me.d * SB_CONTACT_WORDS;
            const int4 row = make_int4((int32_t)n, labels ? (int32_t)cross : -1, (int32_t)wall, (int32_t)first);
            if (((uintptr_t)touch & 15u) == 0u) *(int4 *)t = row;
            else t[0] = row.x, t[1] = row.y, t[2] = row.z, t[3] = row.w;
        }
        above_of[me.d] = other_body ? above_cross : above;
    }
    // the four counts: the wave's sum by the butterfly, then LDS, then one global atomic per workgroup and word
    unsigned long long v[4] = {above, above_cross, wall ? 1ull : 0ull, n ? 1ull : 0ull};
#pragma unroll
    for (int c = 0; c < 4; c++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[c] += __shfl_xor(v[c], off);
        if ((tid & 63u) == 0u && v[c]) atomicAdd(&s_acc[c], v[c]);
    }
    __syncthreads();
    if (tid < 4u && s_acc[tid]) atomicAdd(&acc[tid], s_acc[tid]);
}

// a thread per sorted record: its pairs to place[d] .. place[d] + above[d] - 1, the smallest partner first
__global__ __launch_bounds__(SBC_BLOCK) void k_contacts_list(const SbcRec *__restrict__ sorted, uint32_t P, const uint32_t *__restrict__ end,
                                                             SbcGeo geo, SbcTest ts, const int32_t *__restrict__ labels, uint32_t other_body,
                                                             const uint32_t *__restrict__ above_of, const unsigned long long *__restrict__ place,
                                                             int32_t *pairs, unsigned long long max_pairs)
{
    const uint32_t k = blockIdx.x * SBC_BLOCK + threadIdx.x;
    if (k >= P) return;
    const SbcRec me = sorted[k];
    unsigned long long at = place[me.d];
    const unsigned long long stop = min(at + (unsigned long long)above_of[me.d], max_pairs);
    if (at >= stop) return;
    const int32_t my_lab = other_body ? labels[me.d] : 0;
    const SbCellWindow w = sbc_window(me.x, me.y, geo);
    sb_select_ascending(true, me.d, [&](SbSelect4 &sel) { // (a listed partner is above d)
            for (uint32_t yy = w.y0; yy <= w.y1; yy++) {
                uint32_t from, to;
                w.run(end, yy, &from, &to);
                for (uint32_t q = from; q < to; q++) {
                    const SbcRec r = sorted[q];
                    if (sel.wants(r.d) && sb_touch(make_float2(me.x, me.y), make_float2(r.x, r.y), ts.thr, ts.two_r) && !(other_body && labels[r.d] == my_lab))
                        sel.insert(r.d);
                }
            }
        },
        [&](uint32_t o) {
            pairs[2ull * at] = (int32_t)me.d, pairs[2ull * at + 1ull] = (int32_t)o;
            return ++at < stop;
        });
}

// rows [listed, max_pairs) of the pair list
__global__ __launch_bounds__(SBC_BLOCK) void k_contacts_tail(const unsigned long long *__restrict__ acc, int32_t *pairs, unsigned long long max_pairs)
{
    const unsigned long long k = (unsigned long long)blockIdx.x * SBC_BLOCK + threadIdx.x;
    if (k < max_pairs && k >= acc[SBC_LISTED]) pairs[2ull * k] = -1, pairs[2ull * k + 1ull] = -1;
}

__global__ __launch_bounds__(64) void k_contacts_counts(const unsigned long long *__restrict__ acc, long long *counts, uint32_t with_labels)
{
    if (threadIdx.x != 0u) return;
    counts[0] = (long long)acc[SBC_PAIRS];
    counts[1] = with_labels ? (long long)acc[SBC_CROSS] : -1ll;
    counts[2] = (long long)acc[SBC_WALLED];
    counts[3] = (long long)acc[SBC_TOUCHING];
}

// ---------------------------------------------------------------- host side

static sb_status sbc_enqueue(sb_engine *e, const sb_contacts_options *o, const void *labels, void *touch, void *pairs, void *counts, bool host)
{
    if (!e) return SB_ERR_INVALID;
    const char *what = host ? "sb_contacts" : "sb_contacts_device";
    const bool given = o && o->struct_size == sizeof(sb_contacts_options);
    const uint32_t flags = given ? o->flags : 0u;
    const uint64_t max_pairs = given ? o->max_pairs : 0u;
    if (flags & ~SB_CONTACTS_OTHER_BODY) SB_FAIL(e, SB_ERR_INVALID, "%s: unknown flags 0x%x", what, flags);
    if ((flags & SB_CONTACTS_OTHER_BODY) && !labels) SB_FAIL(e, SB_ERR_INVALID, "%s: SB_CONTACTS_OTHER_BODY needs labels", what);
    if (!touch && !pairs && !counts) SB_FAIL(e, SB_ERR_INVALID, "%s: no output asked for", what);
    if (max_pairs > 0 && !pairs) SB_FAIL(e, SB_ERR_INVALID, "%s: max_pairs %llu without a pair list", what, (unsigned long long)max_pairs);
    if (((uintptr_t)labels & 3u) || ((uintptr_t)touch & 3u) || ((uintptr_t)pairs & 3u))
        SB_FAIL(e, SB_ERR_INVALID, "%s: labels, touch and pairs must be 4-byte aligned", what);
    if ((uintptr_t)counts & 7u) SB_FAIL(e, SB_ERR_INVALID, "%s: counts must be 8-byte aligned", what);
    if (max_pairs > 0x80000000ull) SB_FAIL(e, SB_ERR_INVALID, "%s: max_pairs above 2^31", what);
    SB_TRY(sbq_preflight(e, what, o, "handled", "contacts across ranks are not handled"));
    SbcGeo geo;
    if (!sbc_geometry(e, &geo) && e->P > SBC_ALL_PAIRS_MAX)
        SB_FAIL(e, SB_ERR_UNSUPPORTED, "%s: the cell side is no ordinary number and the scene has more than %u particles (an all-pairs test of it is not run)",
                what, SBC_ALL_PAIRS_MAX);
    SB_TRY(sbq_need(e, "sb_contacts", SBQ_PARTICLES));
    SbStateIoState &s = *e->sio;
    s.con_build_ms = s.part_ms;

    const uint32_t maxP = e->opt.max_particles, np = s.np, P = s.P;
    const uint64_t ncell = (uint64_t)geo.G * geo.G + 1u;
    const uint32_t nb_cells = (uint32_t)((ncell + SBQ_SCAN - 1u) / SBQ_SCAN), nb_np = (np + SBQ_SCAN - 1u) / SBQ_SCAN;
    const bool list = pairs && max_pairs > 0;
    SB_TRY(s.buf[SBC_B_CELLS].grow(e, ncell * sizeof(uint32_t)));
    uint32_t *d_cells = s.buf[SBC_B_CELLS].as<uint32_t>();
    SB_TRY(s.buf[SBC_B_BSUM].grow(e, (size_t)std::max(nb_cells, nb_np) * sizeof(unsigned long long)));
    void *d_bsum = s.buf[SBC_B_BSUM].p;
    SB_TRY(s.buf[SBC_B_SORTED].grow(e, (size_t)P * sizeof(SbcRec)));
    SbcRec *d_sorted = s.buf[SBC_B_SORTED].as<SbcRec>();
    SB_TRY(s.buf[SBC_B_ABOVE].grow(e, (size_t)np * sizeof(uint32_t)));
    uint32_t *d_above = s.buf[SBC_B_ABOVE].as<uint32_t>();
    SB_TRY(s.buf[SBC_B_ACC].grow(e, (SBC_NACC + SB_CONTACT_COUNT_WORDS) * sizeof(unsigned long long)));
    unsigned long long *d_acc = s.buf[SBC_B_ACC].as<unsigned long long>();
    unsigned long long *d_place = nullptr;
    if (list) {
        SB_TRY(s.buf[SBC_B_PLACE].grow(e, (size_t)np * sizeof(unsigned long long)));
        d_place = s.buf[SBC_B_PLACE].as<unsigned long long>();
    }
    // where the launches read and write: the caller's device memory, or (sb_contacts) the engine's own, copied below
    SbqMirror mir(e, host);
    const size_t b_labels = (size_t)maxP * sizeof(int32_t);
    const int32_t *d_labels = mir.in<int32_t>(SBC_B_LABELS, labels, b_labels, b_labels);
    int32_t *d_touch = mir.out<int32_t>(SBC_B_TOUCH, touch, (size_t)maxP * SB_CONTACT_WORDS * sizeof(int32_t));
    int32_t *d_pairs = mir.out<int32_t>(SBC_B_PAIRS, list ? pairs : nullptr, (size_t)max_pairs * 2 * sizeof(int32_t));
    long long *d_counts = mir.out_at<long long>(counts, d_acc, SBC_NACC * sizeof(unsigned long long), SB_CONTACT_COUNT_WORDS * sizeof(int64_t));
    SB_TRY(mir.st);

    const SbTouchTest tt = sb_touch_test(e->prm.particle_radius);
    const SbcTest ts{tt.two_r, tt.thr, e->prm.particle_radius, e->prm.bounds_size - e->prm.particle_radius}; // sb_particle_finish's lo / hi (compute.wgsl:190)
    const uint32_t other = flags & SB_CONTACTS_OTHER_BODY;
    const float2 *pos = e->part[e->cur].pos;
    const uint32_t *d_pinv = s.buf[SBQ_B_PINV].as<uint32_t>();
    auto blocks = [](uint64_t k) { return (uint32_t)((k + SBC_BLOCK - 1u) / SBC_BLOCK); };

    SB_HIP(e, hipMemsetAsync(d_cells, 0, ncell * sizeof(uint32_t), e->stream));
    SB_HIP(e, hipMemsetAsync(d_acc, 0, SBC_NACC * sizeof(unsigned long long), e->stream));
    const uint32_t n_rows = touch ? maxP : 0u;
    if (std::max(np, n_rows))
        k_contacts_bin<<<blocks(std::max(np, n_rows)), SBC_BLOCK, 0, e->stream>>>(d_pinv, np, pos, geo, d_cells, d_above, d_touch, n_rows, labels ? 0 : -1);
    if (P) {
        sbq_scan<uint32_t>(e, d_cells, ncell, (uint32_t *)d_bsum, d_cells, nullptr);
        k_contacts_scatter<<<blocks(np), SBC_BLOCK, 0, e->stream>>>(d_pinv, np, pos, d_above, d_cells, d_sorted);
        k_contacts_visit<<<blocks(P), SBC_BLOCK, 0, e->stream>>>(d_sorted, P, d_cells, geo, ts, d_labels, other, d_touch, d_above, d_acc);
        if (list) {
            sbq_scan<unsigned long long>(e, d_above, np, (unsigned long long *)d_bsum, d_place, d_acc + SBC_LISTED);
            k_contacts_list<<<blocks(P), SBC_BLOCK, 0, e->stream>>>(d_sorted, P, d_cells, geo, ts, d_labels, other, d_above, d_place, d_pairs, max_pairs);
        }
    }
    if (list) k_contacts_tail<<<blocks(max_pairs), SBC_BLOCK, 0, e->stream>>>(d_acc, d_pairs, max_pairs);
    if (counts) k_contacts_counts<<<1, 64, 0, e->stream>>>(d_acc, d_counts, labels ? 1u : 0u);
    SB_HIP(e, hipGetLastError());
    return mir.finish();
}

// what sb_get_info reads ("contacts_table_build_us", "contacts_cells_per_side", "contacts_kernel_vgprs", "contacts_kernel_scratch_bytes")
bool sbc_info(sb_engine *e, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "contacts_table_build_us") *value = e->sio ? (uint64_t)(e->sio->con_build_ms * 1000.0 + 0.5) : 0u;
    else if (k == "contacts_cells_per_side") { // of the scene as it is now (1: all pairs)
        SbcGeo geo;
        (void)sbc_geometry(e, &geo);
        *value = geo.G;
    }
    else if (k == "contacts_kernel_vgprs" || k == "contacts_kernel_scratch_bytes") { // the most over every kernel a call may launch
        std::vector<const void *> ks = {(const void *)k_contacts_bin, (const void *)k_contacts_scatter, (const void *)k_contacts_visit,
                                        (const void *)k_contacts_list, (const void *)k_contacts_tail, (const void *)k_contacts_counts};
        for (const void *f : sbq_scan_kernels(true)) ks.push_back(f); // (both widths)
        return sbq_kernel_most(e, ks, k == "contacts_kernel_vgprs", value);
    }
    else return false;
    return true;
}

extern "C" {

sb_status sb_contacts_device(sb_engine *e, const sb_contacts_options *opts, const void *device_labels_i32, void *device_touch_i32,
                             void *device_pairs_i32, void *device_counts_i64)
{
    SB_GUARDED(e, sbc_enqueue(e, opts, device_labels_i32, device_touch_i32, device_pairs_i32, device_counts_i64, false))
}

sb_status sb_contacts(sb_engine *e, const sb_contacts_options *opts, const int32_t *labels, int32_t *touch, int32_t *pairs, int64_t *counts)
{
    SB_GUARDED(e, sbc_enqueue(e, opts, labels, touch, pairs, counts, true))
}

} // extern "C"
