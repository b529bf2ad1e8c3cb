// sb_batch_contacts.hip -- who touches whom, and who touches a wall, in every scene of a batch in ONE launch (gfx950, wave64;
// DESIGN.md 5.15).
//
// Two distinct particles i, j of a scene TOUCH iff dist == 0 or dist < particle_radius * 2, dist = sb_length(xj - xi, yj - yi) of
// the current particle records: the expressions of the frame kernel's collision loop (sb_batch.hip, compute.wgsl:150-155), so the
// set reported here is the set the next substep acts on.  It is a property of the positions alone: the batch's collision_mode
// does not enter.  One workgroup per scene; nothing is written but the three outputs.
//
//   stage    positions (and the caller's labels) by particle DATA index in LDS; the cell of every particle (sb_grid_coord, the
//            frame kernel's geometry: G x G cells of side >= 2r (1 + 1/64) over [0, bounds]^2, sb_batch_cell_geometry), counted
//   sort     a counting sort of the data indices by cell: exclusive scan of the G^2 counts, scatter.  Every cell holds whatever
//            lands in it: no bucket can be full, so there is no fallback.  One cell (a width that is no ordinary number, or a
//            radius as wide as the box) is the all-pairs test.
//   visit    every particle tests the particles of the 3 x 3 cells around its own (whoever touches it sits there: the cells are
//            wider than 2r and the coordinate map is monotone) and counts: partners, partners of another label, the smallest
//            partner, partners above it (the pairs it will list)
//   list     exclusive scan of "pairs I list" over the data indices; particle i then writes its pairs {i, j}, j ascending, by
//            repeated selection of the four smallest partners above the last one written (sb_select_ascending); positions
//            >= max_pairs are not written, the tail behind the last pair is filled with -1
// Everything behind the float test is integers: counts, minima, sums (LDS integer atomics) and a list whose order is defined by
// the indices -- neither the order inside a cell nor the schedule can change a bit of the output.
#include <algorithm>
#include <string>

#include "sb_batch.h"

#define SBK_BLOCK 256u
#define SBK_WAVES (SBK_BLOCK / 64u)
#define SBK_NONE 0xFFFFFFFFu
// LDS words behind the arrays: the four sums of the count row, the wave totals of a scan
enum { SBK_PAIRS, SBK_CROSS, SBK_WALLED, SBK_TOUCHING, SBK_WAVE, SBK_NWORDS = SBK_WAVE + SBK_WAVES };

static_assert(SB_BATCH_MAX_PARTICLES <= 0x10000, "a cell coordinate pair is packed into 16 + 16 bits; G <= sqrt(2.5 * max_particles)");

// LDS of a workgroup: pos[maxP] (2 words each), label[maxP], cell[maxP], sorted[maxP], above[maxP], end[G * G + 1], SBK_NWORDS words
static inline uint32_t sbk_lds_bytes(uint32_t maxP, uint32_t g) { return (6u * maxP + g * g + 1u + SBK_NWORDS) * 4u; }

// cells per side of sb_batch_contacts_device and their width: sb_batch_create's rule, whatever the batch's collision_mode and
// threshold; a width that is no ordinary number gives ONE cell (the all-pairs test; its width is never looked at)
static uint32_t sbk_cells(const sb_batch *b, float *cell)
{
    const uint32_t g = sb_batch_cell_geometry(b->opt.bounds_size, b->opt.particle_radius, sb_batch_cell_cap(b->opt.max_particles), cell);
    if (g == 0u) *cell = 1.0f;
    return std::max(g, 1u);
}

// In-place exclusive scan of a[0 .. n) by the whole workgroup; returns the total.  The caller has a barrier between the last
// write of `a` and this call; the scan ends in one.  Thread t owns the words [t * per, (t + 1) * per).
SB_DEV uint32_t sbk_scan(uint32_t *a, uint32_t n, uint32_t *s_wave)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t per = (n + SBK_BLOCK - 1u) / SBK_BLOCK, lo = min(tid * per, n), hi = min(lo + per, n);
    uint32_t sum = 0u;
    for (uint32_t k = lo; k < hi; k++) sum += a[k];
    uint32_t inc = sum;
#pragma unroll
    for (uint32_t off = 1u; off < 64u; off <<= 1) {
        const uint32_t v = __shfl_up(inc, off, 64);
        if (lane >= off) inc += v;
    }
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    uint32_t base = inc - sum, total = 0u;
#pragma unroll
    for (uint32_t w = 0; w < SBK_WAVES; w++) {
        const uint32_t t = s_wave[w];
        base += w < wave ? t : 0u;
        total += t;
    }
    for (uint32_t k = lo; k < hi; k++) {
        const uint32_t v = a[k];
        a[k] = base;
        base += v;
    }
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(SBK_BLOCK) void k_batch_contacts(SbBatchView V, SbParams prm, uint32_t G, float cell, uint32_t other_body,
                                                              const int32_t *__restrict__ labels, int32_t *__restrict__ touch,
                                                              int32_t *__restrict__ pairs, uint32_t max_pairs, int32_t *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sbk_lds[];
    const uint32_t scene = blockIdx.x, tid = threadIdx.x;
    if (scene >= V.n_scenes) return;
    const uint32_t maxP = V.maxP, ncell = G * G;
    float2 *s_pos = (float2 *)sbk_lds;            // [maxP] per particle DATA index: position
    uint32_t *s_lab = sbk_lds + 2u * maxP;        // [maxP] per DATA index: the caller's label (only ever compared)
    uint32_t *s_cell = s_lab + maxP;              // [maxP] per DATA index: cx | cy << 16, SBK_NONE where no particle lives
    uint32_t *s_sorted = s_cell + maxP;           // [maxP] data indices in cell order
    uint32_t *s_above = s_sorted + maxP;          // [maxP] per DATA index: pairs it lists, then where its first one goes
    uint32_t *s_end = s_above + maxP;             // [ncell + 1] particles per cell, then the end of every cell in s_sorted
    uint32_t *s_red = s_end + ncell + 1u;         // [SBK_NWORDS]

    const SbbScene hd = sbb_scene(V, scene);
    const uint32_t P = hd.P;
    const uint32_t *g_pmap = (const uint32_t *)(hd.cst + V.o_pmap);
    const float2 *g_part = (const float2 *)(hd.st + V.o_part);
    const int32_t *lrow = labels ? labels + (size_t)scene * maxP : nullptr;
    int32_t *trow = touch ? touch + (size_t)scene * maxP * SB_BATCH_CONTACT_WORDS : nullptr;
    int32_t *prow = pairs ? pairs + (size_t)scene * max_pairs * 2u : nullptr;
    const int32_t no_label = lrow ? 0 : -1;

    if (P == 0u) { // no particles, or never uploaded: the defined rows (uniform)
        if (trow)
            for (uint32_t d = tid; d < maxP; d += SBK_BLOCK) {
                int32_t *t = trow + (size_t)d * SB_BATCH_CONTACT_WORDS;
                t[0] = 0, t[1] = no_label, t[2] = 0, t[3] = -1;
            }
        if (prow)
            for (unsigned long long k = tid; k < 2ull * max_pairs; k += SBK_BLOCK) prow[k] = -1;
        if (counts && tid < SB_BATCH_CONTACT_WORDS) counts[(size_t)scene * SB_BATCH_CONTACT_WORDS + tid] = tid == 1u ? no_label : 0;
        return;
    }

    // ---- stage (an upload is refused unless its data indices are distinct and inside the capacity)
    for (uint32_t d = tid; d < maxP; d += SBK_BLOCK) {
        s_cell[d] = SBK_NONE;
        s_above[d] = 0u;
        s_lab[d] = lrow ? (uint32_t)lrow[d] : 0u;
    }
    for (uint32_t c = tid; c <= ncell; c += SBK_BLOCK) s_end[c] = 0u;
    if (tid < SBK_NWORDS) s_red[tid] = 0u;
    __syncthreads();
    for (uint32_t s = tid; s < P; s += SBK_BLOCK) {
        const uint32_t d = g_pmap[s];
        const float2 p = g_part[3u * d];
        const uint32_t cx = sb_grid_coord(p.x, 0.0f, cell, G), cy = sb_grid_coord(p.y, 0.0f, cell, G); // monotone, clamped; NaN: cell 0
        s_pos[d] = p;
        s_cell[d] = cx | (cy << 16);
        atomicAdd(&s_end[cy * G + cx], 1u);
    }
    __syncthreads();

    // ---- counting sort by cell: starts, then every particle takes the next place of its cell, which leaves the cell's END behind
    (void)sbk_scan(s_end, ncell, s_red + SBK_WAVE);
    for (uint32_t d = tid; d < maxP; d += SBK_BLOCK) {
        const uint32_t c = s_cell[d];
        if (c != SBK_NONE) s_sorted[atomicAdd(&s_end[(c >> 16) * G + (c & 0xffffu)], 1u)] = d;
    }
    __syncthreads();

    // ---- visit
    const SbTouchTest tt = sb_touch_test(prm.particle_radius);
    const float lo = prm.particle_radius, hi = prm.bounds_size - prm.particle_radius; // sb_particle_finish's (compute.wgsl:190)
    const bool wide = ((uintptr_t)touch & 15u) == 0u; // (rows are 16 bytes: whole-row stores where the buffer allows them)
    uint32_t n_pairs = 0u, n_cross = 0u, n_walled = 0u, n_touching = 0u;
    for (uint32_t d = tid; d < maxP; d += SBK_BLOCK) {
        const uint32_t c = s_cell[d];
        int4 row = make_int4(0, no_label, 0, -1);
        if (c != SBK_NONE) {
            const uint32_t cx = c & 0xffffu, cy = c >> 16, my_lab = s_lab[d];
            const float2 me = s_pos[d];
            const SbCellWindow win(cx, cy, G);
            uint32_t n = 0u, cross = 0u, above = 0u, above_cross = 0u, first = SBK_NONE;
            for (uint32_t yy = win.y0; yy <= win.y1; yy++) {
                uint32_t from, to;
                win.run(s_end, yy, &from, &to);
                for (uint32_t k = from; k < to; k++) {
                    const uint32_t o = s_sorted[k];
                    if (o == d || !sb_touch(me, s_pos[o], tt.thr, tt.two_r)) continue;
                    const uint32_t differs = s_lab[o] != my_lab ? 1u : 0u, up = o > d ? 1u : 0u;
                    n++;
                    cross += differs;
                    above += up;
                    above_cross += up & differs;
                    first = min(first, o);
                }
            }
            const uint32_t wall = (me.x <= lo ? SB_BATCH_WALL_LEFT : 0u) | (me.x >= hi ? SB_BATCH_WALL_RIGHT : 0u) |
                                  (me.y <= lo ? SB_BATCH_WALL_LOW : 0u) | (me.y >= hi ? SB_BATCH_WALL_HIGH : 0u); // (NaN: no bit)
            row = make_int4((int32_t)n, lrow ? (int32_t)cross : -1, (int32_t)wall, (int32_t)first);
            s_above[d] = other_body ? above_cross : above;
            n_pairs += above;
            n_cross += above_cross;
            n_walled += wall ? 1u : 0u;
            n_touching += n ? 1u : 0u;
        }
        if (trow) {
            int32_t *t = trow + (size_t)d * SB_BATCH_CONTACT_WORDS;
            if (wide) *(int4 *)t = row;
            else t[0] = row.x, t[1] = row.y, t[2] = row.z, t[3] = row.w;
        }
    }
    if (n_pairs) atomicAdd(&s_red[SBK_PAIRS], n_pairs);
    if (n_cross) atomicAdd(&s_red[SBK_CROSS], n_cross);
    if (n_walled) atomicAdd(&s_red[SBK_WALLED], n_walled);
    if (n_touching) atomicAdd(&s_red[SBK_TOUCHING], n_touching);
    __syncthreads();
    if (counts && tid == 0u) {
        int32_t *c = counts + (size_t)scene * SB_BATCH_CONTACT_WORDS;
        c[0] = (int32_t)s_red[SBK_PAIRS];
        c[1] = lrow ? (int32_t)s_red[SBK_CROSS] : -1;
        c[2] = (int32_t)s_red[SBK_WALLED];
        c[3] = (int32_t)s_red[SBK_TOUCHING];
    }
    if (!prow) return; // (uniform)

    // ---- list: particle d's pairs go to s_above[d] .. s_above[d + 1] - 1, the smallest partner first
    const uint32_t listed = sbk_scan(s_above, maxP, s_red + SBK_WAVE);
    for (uint32_t d = tid; d < maxP; d += SBK_BLOCK) {
        const uint32_t c = s_cell[d];
        uint32_t at = s_above[d];
        const uint32_t stop = min(d + 1u < maxP ? s_above[d + 1u] : listed, max_pairs);
        if (c == SBK_NONE || at >= stop) continue;
        const uint32_t cx = c & 0xffffu, cy = c >> 16, my_lab = s_lab[d];
        const float2 me = s_pos[d];
        const SbCellWindow win(cx, cy, G);
        sb_select_ascending(true, d, [&](SbSelect4 &sel) { // (a listed partner is above d)
                for (uint32_t yy = win.y0; yy <= win.y1; yy++) {
                    uint32_t from, to;
                    win.run(s_end, yy, &from, &to);
                    for (uint32_t k = from; k < to; k++) {
                        const uint32_t o = s_sorted[k];
                        if (sel.wants(o) && !(other_body && s_lab[o] == my_lab) && sb_touch(me, s_pos[o], tt.thr, tt.two_r)) sel.insert(o);
                    }
                }
            },
            [&](uint32_t o) {
                prow[2ull * at] = (int32_t)d, prow[2ull * at + 1ull] = (int32_t)o;
                return ++at < stop;
            });
    }
    for (unsigned long long k = 2ull * min(listed, max_pairs) + tid; k < 2ull * max_pairs; k += SBK_BLOCK) prow[k] = -1;
}

// ---------------------------------------------------------------- host
bool sbb_contacts_info(sb_batch *b, const char *key, uint64_t *value)
{
    const std::string k(key);
    float cell = 0.f;
    if (k == "contact_words") *value = SB_BATCH_CONTACT_WORDS;
    else if (k == "contacts_cells_per_side") *value = sbk_cells(b, &cell);
    else if (k == "contacts_lds_bytes") *value = sbk_lds_bytes(b->V.maxP, sbk_cells(b, &cell));
    else return sbb_kernel_info(b, "contacts", (const void *)k_batch_contacts, b->contacts_res, key, value);
    return true;
}

sb_status sb_batch_contacts_device(sb_batch *b, uint32_t flags, const void *device_labels_i32, void *device_touch_i32, void *device_pairs_i32,
                                   uint32_t max_pairs, void *device_counts_i32)
{
    if (!b) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_contacts_device: null batch");
    if (flags & ~SB_BATCH_CONTACTS_OTHER_BODY) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_contacts_device: unknown flags 0x%x", flags);
    if ((flags & SB_BATCH_CONTACTS_OTHER_BODY) && !device_labels_i32)
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_contacts_device: SB_BATCH_CONTACTS_OTHER_BODY needs labels");
    if (!device_touch_i32 && !device_pairs_i32 && !device_counts_i32)
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_contacts_device: touch, pairs and counts are all null: nothing to write");
    if (device_pairs_i32 && max_pairs == 0u) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_contacts_device: a pair list of max_pairs 0");
    if (sbb_misaligned4({device_labels_i32, device_touch_i32, device_pairs_i32, device_counts_i32}))
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_contacts_device: the device buffers must be 4-byte aligned");
    SB_HIP(b, hipSetDevice(b->device));
    float cell = 0.f;
    const uint32_t g = sbk_cells(b, &cell);
    k_batch_contacts<<<b->opt.n_scenes, SBK_BLOCK, sbk_lds_bytes(b->V.maxP, g), b->stream>>>(
        b->V, b->prm, g, cell, flags & SB_BATCH_CONTACTS_OTHER_BODY, (const int32_t *)device_labels_i32, (int32_t *)device_touch_i32,
        (int32_t *)device_pairs_i32, max_pairs, (int32_t *)device_counts_i32);
    return check_launch(b, "sb_batch_contacts_device");
}
