// sb_batch_forces.hip -- the forces the NEXT substep would compute from the CURRENT state, per particle and per beam, in every scene
// of a batch in ONE launch that only reads the batch (gfx950, wave64; the definition is include/softbody.h's).
//
// One workgroup per scene; nothing is written but the caller's four outputs.
//   stage    positions and velocities by particle SLOT in LDS (the step's own order: internal index == slot), the caller's label
//            of every slot, a bit per particle / beam DATA index "somebody lives here", zeroed force sums
//   beams    a lane per live beam slot: sb_beam_eval<false> on the staged positions, the beam's current {target_length,
//            last_length} and its material row -- the call k_batch_frame's beam phase makes, with nothing stored back -- and its
//            four i32 contributions added into [P][2] LDS words (integer atomics: order-free).  force_mag (sbf_force_mag, the
//            same sub-expressions) goes to `tension` at the beam's data index.
//   bin      (scenes of at least grid_min_particles particles, beside the beam phase) every particle's slot into the cell of its
//            position: the frame kernel's G x G buckets of SB_BATCH_CELL_K slots (sb_batch_cell_geometry).  A full bucket
//            sends the whole workgroup through the loop over all slots.
//   contacts a lane per particle slot: its partners in ASCENDING SLOT ORDER -- the loop over all slots, or selection sweeps over
//            the 3 x 3 cells around its own (sb_contact_cells.h: window, buckets, sb_select_ascending) -- each through
//            sbf_contact_add: the terms sb_collide_pair_at would subtract from particle.a and particle.v.  The float sums depend
//            on the order alone, and the order is the slots': both paths give the same bits.
//   rows     the lane of a particle writes its row and its two force words at the particle's data index; rows of data indices
//            where nobody lives are written as zeros by whoever comes by: every word is written exactly once.
#include <algorithm>
#include <string>

#include "sb_batch.h"
#include "sb_batch_forces_math.h"

#define SBF_BLOCK 256u
enum { SBF_TOUCHING, SBF_NONFINITE, SBF_OVERFLOW, SBF_NWORDS = 4 }; // LDS words behind the arrays (the fourth keeps what follows 8-byte aligned)

// cells per side of sb_batch_forces_device and their width: sb_batch_create's rule, whatever the batch's collision_mode; 0: no
// cells (a width that is no ordinary number): every scene takes the loop over all slots
static uint32_t sbf_cells(const sb_batch *b, float *cell)
{
    *cell = 1.0f;
    return sb_batch_cell_geometry(b->opt.bounds_size, b->opt.particle_radius, sb_batch_cell_cap(b->opt.max_particles), cell);
}
// LDS words in front of the cells: pos, vel, f (2 words each), label per slot; the two bitmaps; SBF_NWORDS; made even
static __host__ __device__ inline uint32_t sbf_cell_off_words(uint32_t maxP, uint32_t maxB) { return (7u * maxP + (maxP + 31u) / 32u + (maxB + 31u) / 32u + SBF_NWORDS + 1u) & ~1u; }
// the cells behind them: the buckets of sb_contact_cells.h, then their counts
static inline uint32_t sbf_lds_bytes(uint32_t maxP, uint32_t maxB, uint32_t g)
{
    return (sbf_cell_off_words(maxP, maxB) + sb_bucket_entry_words(g) + sb_bucket_count_words(g)) * 4u;
}

__global__ __launch_bounds__(SBF_BLOCK) void k_batch_forces(SbBatchView V, SbParams prm, uint32_t G, float cell, uint32_t cell_min_p,
                                                            uint32_t other_body, const int32_t *__restrict__ labels, float *__restrict__ rows,
                                                            int32_t *__restrict__ beam_i32, float *__restrict__ tension,
                                                            int32_t *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sbf_lds[];
    const uint32_t scene = blockIdx.x, tid = threadIdx.x;
    if (scene >= V.n_scenes) return;
    const uint32_t maxP = V.maxP, maxB = V.maxB, pw = (maxP + 31u) >> 5, bw = (maxB + 31u) >> 5, ncell = G * G;
    float2 *s_pos = (float2 *)sbf_lds;           // [maxP] per particle SLOT
    float2 *s_vel = s_pos + maxP;                // [maxP]
    int *s_f = (int *)(s_vel + maxP);            // [maxP][2] fixed-point force sums (compute.wgsl:68-69)
    uint32_t *s_lab = (uint32_t *)(s_f + 2u * maxP); // [maxP] per slot: the caller's label (only ever compared)
    uint32_t *s_pbits = s_lab + maxP;            // [pw] per particle DATA index: a particle lives here
    uint32_t *s_bbits = s_pbits + pw;            // [bw] per beam DATA index: an evaluated beam lives here
    uint32_t *s_red = s_bbits + bw;              // [SBF_NWORDS]
    uint16_t *s_cent = (uint16_t *)(sbf_lds + sbf_cell_off_words(maxP, maxB)); // [ncell][SB_BATCH_CELL_K] slots
    uint32_t *s_ccnt = (uint32_t *)(s_cent + ncell * SB_BATCH_CELL_K);          // [sb_bucket_count_words(G)]

    const SbbScene hd = sbb_scene(V, scene);
    const uint32_t P = hd.P, Bc = hd.Bc;
    float *rrow = rows ? rows + (size_t)scene * maxP * SB_BATCH_FORCE_WORDS : nullptr;
    int32_t *frow = beam_i32 ? beam_i32 + (size_t)scene * maxP * 2u : nullptr;
    float *trow = tension ? tension + (size_t)scene * maxB : nullptr;
    const bool wide = ((uintptr_t)rows & 15u) == 0u; // (rows are 32 bytes: two 16-byte stores where the buffer allows them)
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    if (P == 0u) { // no particles, or never uploaded: zeros (uniform).  A beam needs two particles: none is evaluated.
        for (uint32_t d = tid; d < maxP; d += SBF_BLOCK) {
            if (rrow) {
                float *r = rrow + (size_t)d * SB_BATCH_FORCE_WORDS;
                if (wide) ((float4 *)r)[0] = zero4, ((float4 *)r)[1] = zero4;
                else
                    for (uint32_t k = 0; k < SB_BATCH_FORCE_WORDS; k++) r[k] = 0.f;
            }
            if (frow) frow[2u * d] = 0, frow[2u * d + 1u] = 0;
        }
        if (trow)
            for (uint32_t d = tid; d < maxB; d += SBF_BLOCK) trow[d] = 0.f;
        if (counts && tid < SB_BATCH_FORCE_COUNT_WORDS) counts[(size_t)scene * SB_BATCH_FORCE_COUNT_WORDS + tid] = 0;
        return;
    }

    const uint32_t *meta = V.meta + (size_t)scene * SB_BM_WORDS;
    const uint32_t *g_pmap = (const uint32_t *)(hd.cst + V.o_pmap);
    const uint32_t *g_bword = (const uint32_t *)(hd.cst + V.o_bword);
    const float *g_bmat = (const float *)(hd.cst + V.o_bmat);
    const float2 *g_part = (const float2 *)(hd.st + V.o_part);
    const float4 *g_bstate = (const float4 *)(hd.st + V.o_bstate);
    const uint32_t *g_bmap = (const uint32_t *)(hd.st + V.o_bmap);
    const int32_t *lrow = (labels && other_body) ? labels + (size_t)scene * maxP : nullptr;
    // SbConsts.elasticity / .friction (metadata words are rewritten between launches: read at agent scope, as k_batch_frame does)
    const float elasticity = sbb_uniform(__uint_as_float(SB_AGENT_LOAD(&meta[SB_BM_CONSTS + 4u])));
    const float friction = sbb_uniform(__uint_as_float(SB_AGENT_LOAD(&meta[SB_BM_CONSTS + 5u])));
    const bool cells = G != 0u && P >= cell_min_p; // workgroup-uniform

    // ---- stage (an upload is refused unless its data indices are distinct and inside the capacity; the bounds tests below keep
    // a blob that is not what an upload leaves from reaching past the caller's buffers all the same)
    for (uint32_t w = tid; w < pw + bw + SBF_NWORDS; w += SBF_BLOCK) s_pbits[w] = 0u; // (the three arrays are neighbours)
    if (cells)
        for (uint32_t w = tid; w < sb_bucket_count_words(G); w += SBF_BLOCK) s_ccnt[w] = 0u;
    __syncthreads();
    for (uint32_t s = tid; s < P; s += SBF_BLOCK) {
        const uint32_t d = g_pmap[s];
        const bool in = d < maxP;
        // (a slot whose data index lies outside the capacity -- no upload leaves one -- is staged as NaN: it lands in cell 0, is
        // nobody's partner (sb_touch), and a beam on it converts to 0)
        const uint32_t dd = in ? d : 0u;
        float2 p = g_part[3u * dd], v = g_part[3u * dd + 1u];
        if (!in) p.x = p.y = v.x = v.y = __uint_as_float(SBB_QNAN);
        s_pos[s] = p;
        s_vel[s] = v;
        s_f[2u * s] = 0;
        s_f[2u * s + 1u] = 0;
        s_lab[s] = (lrow && in) ? (uint32_t)lrow[d] : 0u;
        if (in) atomicOr(&s_pbits[d >> 5], 1u << (d & 31u));
        if (cells) { // bin (the counts were zeroed a barrier ago)
            const uint32_t cx = sb_grid_coord(p.x, 0.0f, cell, G), cy = sb_grid_coord(p.y, 0.0f, cell, G); // monotone, clamped; NaN: cell 0
            if (sb_bucket_push(s_cent, s_ccnt, cy * G + cx, s)) s_red[SBF_OVERFLOW] = 1u;
        }
    }
    __syncthreads();

    // ---- beam phase (compute.wgsl:96-131; sb_batch.hip's loop, with nothing stored back into the batch)
    uint32_t n_nonfinite = 0u;
    for (uint32_t j = tid; j < Bc; j += SBF_BLOCK) {
        const uint32_t d = min(g_bmap[j], maxB - 1u); // (Bc > 0: maxB > 0)
        const uint32_t word = g_bword[d], ia = min(word & 0xffffu, P - 1u), ib = min(word >> 16, P - 1u);
        const float4 bs = g_bstate[d];
        const float *m = &g_bmat[SB_BATCH_MAT_ROW * d];
        const float length = m[0], spring = m[1], damp = m[2], yield = m[3], limit = m[4], inv_length = m[5];
        const float2 pa = s_pos[ia], pb = s_pos[ib];
        const SbBeamResult r = sb_beam_eval<false>(pa, pb, length, inv_length, bs.x, bs.y, spring, damp, yield, limit);
        atomicAdd(&s_f[2u * ia], r.ax);
        atomicAdd(&s_f[2u * ia + 1u], r.ay);
        atomicAdd(&s_f[2u * ib], r.bx);
        atomicAdd(&s_f[2u * ib + 1u], r.by);
        const float force_mag = sbf_force_mag(pa.x, pa.y, pb.x, pb.y, bs.x, bs.y, spring, damp);
        n_nonfinite += sbf_finite(force_mag) ? 0u : 1u;
        atomicOr(&s_bbits[d >> 5], 1u << (d & 31u));
        if (trow) trow[d] = force_mag;
    }
    if (n_nonfinite) atomicAdd(&s_red[SBF_NONFINITE], n_nonfinite);
    __syncthreads();

    // ---- contact phase and the rows of the particles
    const float elasticity_coeff = sb_div(elasticity + 1.0f, 2.0f); // :143
    const SbTouchTest tt = sb_touch_test(prm.particle_radius);
    const float two_r = tt.two_r, thr = tt.thr;
    const float dt2 = prm.time_step * prm.time_step;
    const bool walk = !cells || sbb_uniform(s_red[SBF_OVERFLOW]) != 0u; // a cell was full: every thread takes the loop
    uint32_t n_touching = 0u;
    for (uint32_t s = tid; s < P; s += SBF_BLOCK) {
        const float2 me = s_pos[s], mv = s_vel[s];
        const uint32_t my_lab = s_lab[s];
        SbfContact c = sbf_contact_zero();
        if (walk) {
            for (uint32_t o = 0; o < P; o++) { // :144-170, ascending slot order
                const float2 op = s_pos[o];
                if (o == s || (other_body && s_lab[o] == my_lab) || !sb_touch(me, op, thr, two_r)) continue;
                const float dx = op.x - me.x, dy = op.y - me.y;
                const float2 ov = s_vel[o];
                sbf_contact_add(c, dx, dy, sb_sqrt(dx * dx + dy * dy), mv.x - ov.x, mv.y - ov.y, two_r, friction, elasticity_coeff, prm.inv_dt2, dt2);
            }
        } else {
            const uint32_t cx = sb_grid_coord(me.x, 0.0f, cell, G), cy = sb_grid_coord(me.y, 0.0f, cell, G);
            const SbCellWindow win(cx, cy, G);
            sb_select_ascending(false, 0u, [&](SbSelect4 &sel) {
                    sb_bucket_for_window(win, s_cent, s_ccnt, [&](uint32_t o) {
                        if (o != s && sel.wants(o) && !(other_body && s_lab[o] == my_lab) && sb_touch(me, s_pos[o], thr, two_r)) sel.insert(o);
                    });
                },
                [&](uint32_t o) {
                    const float2 op = s_pos[o], ov = s_vel[o];
                    const float dx = op.x - me.x, dy = op.y - me.y;
                    sbf_contact_add(c, dx, dy, sb_sqrt(dx * dx + dy * dy), mv.x - ov.x, mv.y - ov.y, two_r, friction, elasticity_coeff, prm.inv_dt2, dt2);
                    return true;
                });
        }
        n_touching += c.partners ? 1u : 0u;
        const uint32_t d = g_pmap[s];
        if (d >= maxP) continue;
        const int fx = s_f[2u * s], fy = s_f[2u * s + 1u];
        if (frow) frow[2u * d] = fx, frow[2u * d + 1u] = fy;
        if (rrow) {
            float *r = rrow + (size_t)d * SB_BATCH_FORCE_WORDS;
            const float4 lo = make_float4((float)fx * 0x1p-16f, (float)fy * 0x1p-16f, c.push_x, c.push_y); // sb_particle_integrate's product
            const float4 hi = make_float4(c.impulse_x, c.impulse_y, c.depth, (float)c.partners);
            if (wide) ((float4 *)r)[0] = lo, ((float4 *)r)[1] = hi;
            else r[0] = lo.x, r[1] = lo.y, r[2] = lo.z, r[3] = lo.w, r[4] = hi.x, r[5] = hi.y, r[6] = hi.z, r[7] = hi.w;
        }
    }
    if (n_touching) atomicAdd(&s_red[SBF_TOUCHING], n_touching);

    // ---- the rows where nobody lives
    for (uint32_t d = tid; d < maxP; d += SBF_BLOCK) {
        if (s_pbits[d >> 5] >> (d & 31u) & 1u) continue;
        if (rrow) {
            float *r = rrow + (size_t)d * SB_BATCH_FORCE_WORDS;
            if (wide) ((float4 *)r)[0] = zero4, ((float4 *)r)[1] = zero4;
            else
                for (uint32_t k = 0; k < SB_BATCH_FORCE_WORDS; k++) r[k] = 0.f;
        }
        if (frow) frow[2u * d] = 0, frow[2u * d + 1u] = 0;
    }
    if (trow)
        for (uint32_t d = tid; d < maxB; d += SBF_BLOCK)
            if (!(s_bbits[d >> 5] >> (d & 31u) & 1u)) trow[d] = 0.f;
    __syncthreads();
    if (counts && tid == 0u) {
        int32_t *c = counts + (size_t)scene * SB_BATCH_FORCE_COUNT_WORDS;
        c[0] = (int32_t)P;
        c[1] = (int32_t)Bc;
        c[2] = (int32_t)s_red[SBF_TOUCHING];
        c[3] = (int32_t)s_red[SBF_NONFINITE];
    }
}

// ---------------------------------------------------------------- host
bool sbb_forces_info(sb_batch *b, const char *key, uint64_t *value)
{
    const std::string k(key);
    float cell = 0.f;
    if (k == "force_words") *value = SB_BATCH_FORCE_WORDS;
    else if (k == "force_count_words") *value = SB_BATCH_FORCE_COUNT_WORDS;
    else if (k == "forces_cells_per_side") *value = sbf_cells(b, &cell);
    else if (k == "forces_lds_bytes") *value = sbf_lds_bytes(b->V.maxP, b->V.maxB, sbf_cells(b, &cell));
    else return sbb_kernel_info(b, "forces", (const void *)k_batch_forces, b->forces_res, key, value);
    return true;
}

sb_status sb_batch_forces_device(sb_batch *b, uint32_t flags, const void *device_labels_i32, void *device_rows_f32, void *device_beam_i32,
                                 void *device_tension_f32, void *device_counts_i32)
{
    // sbb_edit_entry's checks in its words, with the one of the labels between them: all of them before a device is selected
    if (!b) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_forces_device: null batch");
    if (flags & ~SB_BATCH_FORCES_OTHER_BODY)
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_forces_device: flags 0x%x: only SB_BATCH_FORCES_OTHER_BODY known", flags);
    if ((flags & SB_BATCH_FORCES_OTHER_BODY) && !device_labels_i32)
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_forces_device: SB_BATCH_FORCES_OTHER_BODY needs labels");
    if (sbb_misaligned4({device_labels_i32, device_rows_f32, device_beam_i32, device_tension_f32, device_counts_i32}))
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_forces_device: labels, rows, beam_i32, tension and counts must be 4-byte aligned");
    if (!device_rows_f32 && !device_beam_i32 && !device_tension_f32 && !device_counts_i32) return SB_OK; // nothing to write
    SB_HIP(b, hipSetDevice(b->device));
    float cell = 0.f;
    const uint32_t g = sbf_cells(b, &cell);
    k_batch_forces<<<b->opt.n_scenes, SBF_BLOCK, sbf_lds_bytes(b->V.maxP, b->V.maxB, g), b->stream>>>(
        b->V, b->prm, g, cell, b->grid_min_particles, flags & SB_BATCH_FORCES_OTHER_BODY, (const int32_t *)device_labels_i32,
        (float *)device_rows_f32, (int32_t *)device_beam_i32, (float *)device_tension_f32, (int32_t *)device_counts_i32);
    return check_launch(b, "sb_batch_forces_device");
}
