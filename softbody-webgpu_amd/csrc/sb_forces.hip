// sb_forces.hip -- how hard every beam pulls and every contact pushes in the whole scene of an sb_engine: the forces the NEXT substep
// would compute from the CURRENT state, per particle and per beam, found on the device (sb_forces / sb_forces_device of
// include/softbody.h; gfx950, wave64).
//
// The definition is sb_batch_forces_device's, word for word.  k_batch_forces holds a scene in the LDS of one workgroup; here the
// scene lies in HBM, and the call may only enqueue: nothing loops on a host read-back and no workgroup waits for another.  One launch
// per stage on the engine's stream, behind two memsets (the beam accumulators, the counts):
//   k_forces_beams    a thread per caller beam slot of the latest upload: live unless a delete pass removed it (sbq_dead; a pending
//                     break flag still counts).  sb_beam_eval<false> on the current positions of its endpoints, the {target_length,
//                     last_length} of the copy sb_read_state_device exports and its {spring, damp} as uploaded (the shared scene
//                     tables, sb_report.hip) -- EVERY lane of a wave makes the call, lanes without a live beam with a benign one, so
//                     the wave-uniform gate of the short sqrt sees one convergent call site -- and its four i32 contributions added
//                     to the [.][2] accumulators at the endpoints' DATA indices with returnless global atomics (integers: no order).
//                     force_mag (sbf_force_mag, the same sub-expressions) goes to `tension` at the beam's data index.
//   k_forces_bin, sbq_scan, k_forces_scatter
//                     sb_contacts.hip's counting sort by cell (sb_scene_cells.h), of records {x, y, mapping slot}
//   k_forces_visit    a thread per sorted record: its partners (sb_touch) in ASCENDING MAPPING-SLOT ORDER -- the order of the step's
//                     collision loop -- by selection sweeps over the runs of its 3 x 3 cells (sb_select_ascending), each fetched
//                     through the slot -> internal particle table and added by sbf_contact_add; then its row, with beam_x/y from the
//                     finished accumulators: the launch stands behind k_forces_beams on the stream.
//   k_forces_fill     eight +0 words at every data index up to max_particles at which nobody lives
//   k_forces_counts   the accumulators into the four int64 words
// The float sums depend on the order of the partners alone, and the order is the slots': neither the order inside a cell nor the
// schedule can change a bit.  The file only READS the engine.  Cost: the beams once; the contacts as sb_contacts.hip's visit, the sum
// over particles of the population of their 3 x 3 cells per sweep of four partners.
#include <algorithm>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "sb_scene_cells.h"
#include "sb_batch_forces_math.h"

#define SBFE_BLOCK 256u

enum { SBFE_EVALUATED, SBFE_TOUCHING, SBFE_NONFINITE, SBFE_NACC = 4 }; // accumulator words (unsigned long long)

struct SbfeRec {
    float x, y;
    uint32_t slot;
};

// tab: the four planes of the shared scene tables, n caller slots each; row: per caller slot the data index of its beam record;
// mat: per caller slot {spring, damp}; f: [.][2] accumulators at particle data indices
__global__ __launch_bounds__(SBFE_BLOCK) void k_forces_beams(const uint32_t *__restrict__ tab, uint32_t n, const uint32_t *__restrict__ row,
                                                             const float2 *__restrict__ mat, const uint32_t *__restrict__ pinv,
                                                             const float2 *__restrict__ pos, const float *__restrict__ target,
                                                             const float *__restrict__ last, const uint32_t *__restrict__ dead,
                                                             uint32_t max_beams, int32_t *f, float *tension, unsigned long long *acc)
{
    const uint32_t u = blockIdx.x * SBFE_BLOCK + threadIdx.x;
    bool live = false;
    // the benign beam of a lane that has none: length 1, at rest, no spring (inside the gate; nothing of it is kept)
    float2 pa = make_float2(0.0f, 0.0f), pb = make_float2(1.0f, 0.0f), m = make_float2(0.0f, 0.0f);
    float tg = 1.0f, ls = 1.0f;
    uint32_t da = 0u, db = 0u, d = 0u;
    if (u < n) {
        const uint32_t slot = tab[2u * (size_t)n + u];
        live = !(dead && dead[slot] != 0u);
        if (live) {
            da = tab[u], db = tab[(size_t)n + u];
            pa = pos[pinv[da]], pb = pos[pinv[db]];
            const uint32_t c = tab[3u * (size_t)n + u];
            tg = target[c], ls = last[c];
            m = mat[u];
            d = row[u];
        }
    }
    // (length, 1 / length, yield and limit only shape what the step would store back: nothing of that is read here)
    const SbBeamResult r = sb_beam_eval<false>(pa, pb, 1.0f, 1.0f, tg, ls, m.x, m.y, 1.0f, 1.0f);
    bool bad = false;
    if (live) {
        atomicAdd(&f[2u * (size_t)da], r.ax);
        atomicAdd(&f[2u * (size_t)da + 1u], r.ay);
        atomicAdd(&f[2u * (size_t)db], r.bx);
        atomicAdd(&f[2u * (size_t)db + 1u], r.by);
        const float force_mag = sbf_force_mag(pa.x, pa.y, pb.x, pb.y, tg, ls, m.x, m.y);
        bad = !sbf_finite(force_mag);
        if (tension && d < max_beams) tension[d] = force_mag;
    }
    sbw_count(acc, SBFE_EVALUATED, live);
    sbw_count(acc, SBFE_NONFINITE, bad);
}

// a thread per internal particle: its cell, one atomicAdd on the cell's count per run of lanes with the same cell
__global__ __launch_bounds__(SBFE_BLOCK) void k_forces_bin(uint32_t P, const float2 *__restrict__ pos, SbcGeo geo, uint32_t *count, uint32_t *cell_of)
{
    const uint32_t i = blockIdx.x * SBFE_BLOCK + threadIdx.x;
    uint32_t c = SBC_NONE;
    if (i < P) {
        const float2 p = pos[i];
        c = sbc_cell(p.x, p.y, geo);
        cell_of[i] = c;
    }
    sbc_count_runs(count, c);
}

// a thread per internal particle: its record to the next place of its cell (every cell's END is left in its word)
__global__ __launch_bounds__(SBFE_BLOCK) void k_forces_scatter(uint32_t P, const float2 *__restrict__ pos, const uint32_t *__restrict__ pslot,
                                                               const uint32_t *__restrict__ cell_of, uint32_t *start, SbfeRec *sorted)
{
    const uint32_t i = blockIdx.x * SBFE_BLOCK + threadIdx.x;
    if (i >= P) return;
    const float2 p = pos[i];
    SbfeRec r;
    r.x = p.x, r.y = p.y, r.slot = pslot[i];
    sorted[atomicAdd(&start[cell_of[i]], 1u)] = r;
}

struct SbfeConsts {
    float two_r, thr, friction, elasticity, inv_dt2, dt2;
};

__global__ __launch_bounds__(SBFE_BLOCK) void k_forces_visit(const SbfeRec *__restrict__ sorted, uint32_t P, const uint32_t *__restrict__ end,
                                                             SbcGeo geo, SbfeConsts k, const uint32_t *__restrict__ islot,
                                                             const uint32_t *__restrict__ pidx, const float2 *__restrict__ pos,
                                                             const float2 *__restrict__ vel, const int32_t *__restrict__ labels,
                                                             uint32_t max_particles, const int32_t *__restrict__ f, float *rows,
                                                             unsigned long long *acc)
{
    const uint32_t at = blockIdx.x * SBFE_BLOCK + threadIdx.x;
    bool touching = false;
    if (at < P) {
        const SbfeRec me = sorted[at];
        const uint32_t i = islot[me.slot], d = pidx[i];
        const float2 mp = make_float2(me.x, me.y), mv = vel[i];
        const int32_t my_lab = labels ? labels[d] : 0; // (labels: only with SB_FORCES_OTHER_BODY)
        const float elasticity_coeff = sb_div(k.elasticity + 1.0f, 2.0f); // :143
        const SbCellWindow w = sbc_window(me.x, me.y, geo);
        SbfContact c = sbf_contact_zero();
        sb_select_ascending(false, 0u, [&](SbSelect4 &sel) {
                for (uint32_t yy = w.y0; yy <= w.y1; yy++) {
                    uint32_t from, to;
                    w.run(end, yy, &from, &to);
                    for (uint32_t q = from; q < to; q++) {
                        const SbfeRec r = sorted[q];
                        if (r.slot != me.slot && sel.wants(r.slot) && sb_touch(mp, make_float2(r.x, r.y), k.thr, k.two_r) &&
                            !(labels && labels[pidx[islot[r.slot]]] == my_lab))
                            sel.insert(r.slot);
                    }
                }
            },
            [&](uint32_t o) {
                const uint32_t j = islot[o];
                const float2 op = pos[j], ov = vel[j];
                const float dx = op.x - mp.x, dy = op.y - mp.y;
                sbf_contact_add(c, dx, dy, sb_sqrt(dx * dx + dy * dy), mv.x - ov.x, mv.y - ov.y, k.two_r, k.friction, elasticity_coeff, k.inv_dt2, k.dt2);
                return true;
            });
        touching = c.partners != 0u;
        if (rows && d < max_particles) {
            float *r = rows + (size_t)d * SB_FORCE_WORDS;
            const float4 lo = make_float4((float)f[2u * (size_t)d] * 0x1p-16f, (float)f[2u * (size_t)d + 1u] * 0x1p-16f, c.push_x, c.push_y); // sb_particle_integrate's product
            const float4 hi = make_float4(c.impulse_x, c.impulse_y, c.depth, (float)c.partners);
            if (((uintptr_t)rows & 15u) == 0u) ((float4 *)r)[0] = lo, ((float4 *)r)[1] = hi;
            else r[0] = lo.x, r[1] = lo.y, r[2] = lo.z, r[3] = lo.w, r[4] = hi.x, r[5] = hi.y, r[6] = hi.z, r[7] = hi.w;
        }
    }
    sbw_count(acc, SBFE_TOUCHING, touching);
}

// a thread per data index < max_particles: eight +0 words where no particle lives
__global__ __launch_bounds__(SBFE_BLOCK) void k_forces_fill(const uint32_t *__restrict__ pinv, uint32_t np, uint32_t max_particles, float *rows)
{
    const uint32_t d = blockIdx.x * SBFE_BLOCK + threadIdx.x;
    if (d >= max_particles || (d < np && pinv[d] != SBQ_NONE)) return;
    float *r = rows + (size_t)d * SB_FORCE_WORDS;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (((uintptr_t)rows & 15u) == 0u) ((float4 *)r)[0] = zero4, ((float4 *)r)[1] = zero4;
    else
        for (uint32_t q = 0; q < SB_FORCE_WORDS; q++) r[q] = 0.f;
}

__global__ __launch_bounds__(64) void k_forces_counts(const unsigned long long *__restrict__ acc, long long *counts, uint32_t P)
{
    if (threadIdx.x != 0u) return;
    counts[0] = (long long)P;
    counts[1] = (long long)acc[SBFE_EVALUATED];
    counts[2] = (long long)acc[SBFE_TOUCHING];
    counts[3] = (long long)acc[SBFE_NONFINITE];
}

// ---------------------------------------------------------------- host side

static sb_status sbfe_enqueue(sb_engine *e, const sb_forces_options *o, const void *labels, void *rows, void *beam_i32, void *tension, void *counts,
                              bool host)
{
    if (!e) return SB_ERR_INVALID;
    const char *what = host ? "sb_forces" : "sb_forces_device";
    const bool given = o && o->struct_size == sizeof(sb_forces_options);
    const uint32_t flags = given ? o->flags : 0u;
    if (flags & ~SB_FORCES_OTHER_BODY) SB_FAIL(e, SB_ERR_INVALID, "%s: flags 0x%x: only SB_FORCES_OTHER_BODY is known", what, flags);
    if ((flags & SB_FORCES_OTHER_BODY) && !labels) SB_FAIL(e, SB_ERR_INVALID, "%s: SB_FORCES_OTHER_BODY needs labels", what);
    if (!rows && !beam_i32 && !tension && !counts) SB_FAIL(e, SB_ERR_INVALID, "%s: no output asked for", what);
    if (((uintptr_t)labels | (uintptr_t)rows | (uintptr_t)beam_i32 | (uintptr_t)tension) & 3u)
        SB_FAIL(e, SB_ERR_INVALID, "%s: labels, rows, beam_i32 and tension must be 4-byte aligned", what);
    if ((uintptr_t)counts & 7u) SB_FAIL(e, SB_ERR_INVALID, "%s: counts must be 8-byte aligned", what);
    SB_TRY(sbq_preflight(e, what, o, "handled", "forces across ranks are not handled"));
    SbcGeo geo;
    if (!sbc_geometry(e, &geo) && e->P > SBC_ALL_PAIRS_MAX)
        SB_FAIL(e, SB_ERR_UNSUPPORTED, "%s: the cell side is no ordinary number and the scene has more than %u particles (an all-pairs test of it is not run)",
                what, SBC_ALL_PAIRS_MAX);
    SB_TRY(sbq_need(e, what, SBQ_PARTICLES | SBQ_BEAMS | SBQ_COPIES | SBQ_SLOTS | SBQ_MATERIALS));
    SbStateIoState &s = *e->sio;
    if (!s.cut_valid) SB_TRY(sbx_build_rows(e, what));
    s.for_build_ms = s.part_ms + s.beam_ms + s.copy_ms + s.islot_ms + s.mat_ms + s.cut_row_ms;

    const uint32_t maxP = e->opt.max_particles, maxB = e->opt.max_beams, np = s.np, P = s.P, n = s.nslots;
    const bool contacts = rows || counts; // (beam_i32 and tension alone need no partner)
    const uint64_t ncell = (uint64_t)geo.G * geo.G + 1u;
    SB_TRY(s.buf[SBF_B_ACC].grow(e, (SBFE_NACC + SB_FORCE_COUNT_WORDS) * sizeof(unsigned long long)));
    unsigned long long *d_acc = s.buf[SBF_B_ACC].as<unsigned long long>();
    uint32_t *d_cells = nullptr, *d_bsum = nullptr, *d_cell_of = nullptr;
    SbfeRec *d_sorted = nullptr;
    if (contacts && P) {
        SB_TRY(s.buf[SBF_B_CELLS].grow(e, ncell * sizeof(uint32_t)));
        d_cells = s.buf[SBF_B_CELLS].as<uint32_t>();
        SB_TRY(s.buf[SBF_B_BSUM].grow(e, (size_t)((ncell + SBQ_SCAN - 1u) / SBQ_SCAN) * sizeof(uint32_t)));
        d_bsum = s.buf[SBF_B_BSUM].as<uint32_t>();
        SB_TRY(s.buf[SBF_B_SORTED].grow(e, (size_t)P * sizeof(SbfeRec)));
        d_sorted = s.buf[SBF_B_SORTED].as<SbfeRec>();
        SB_TRY(s.buf[SBF_B_CELL_OF].grow(e, (size_t)P * sizeof(uint32_t)));
        d_cell_of = s.buf[SBF_B_CELL_OF].as<uint32_t>();
    }
    // where the launches read and write: the caller's device memory, or (sb_forces) the engine's own, copied below
    SbqMirror mir(e, host);
    const size_t b_labels = (size_t)maxP * sizeof(int32_t);
    const int32_t *d_labels = mir.in<int32_t>(SBF_B_LABELS, (flags & SB_FORCES_OTHER_BODY) ? labels : nullptr, b_labels, b_labels);
    float *d_rows = mir.out<float>(SBF_B_ROWS, rows, (size_t)maxP * SB_FORCE_WORDS * sizeof(float));
    int32_t *d_beam = mir.out<int32_t>(SBF_B_BEAM_OUT, beam_i32, (size_t)maxP * 2 * sizeof(int32_t));
    float *d_tension = mir.out<float>(SBF_B_TENSION, tension, (size_t)maxB * sizeof(float));
    long long *d_counts = mir.out_at<long long>(counts, d_acc, SBFE_NACC * sizeof(unsigned long long), SB_FORCE_COUNT_WORDS * sizeof(int64_t));
    SB_TRY(mir.st);
    // the accumulators: the caller's beam_i32 itself where it is given ([max_particles][2]; nothing is ever added where nobody lives)
    int32_t *d_f = d_beam;
    size_t f_words = (size_t)maxP * 2;
    if (!d_f) {
        f_words = (size_t)std::max(np, 1u) * 2;
        SB_TRY(s.buf[SBF_B_BEAM].grow(e, f_words * sizeof(int32_t)));
        d_f = s.buf[SBF_B_BEAM].as<int32_t>();
    }

    const SbTouchTest tt = sb_touch_test(e->prm.particle_radius);
    const SbfeConsts k{tt.two_r, tt.thr, e->consts.friction, e->consts.elasticity, e->prm.inv_dt2, e->prm.time_step * e->prm.time_step};
    const SbParticleArrays &cur = e->part[e->cur];
    const uint32_t *d_pinv = s.buf[SBQ_B_PINV].as<uint32_t>(), *d_islot = s.buf[SBQ_B_ISLOT].as<uint32_t>();
    auto blocks = [](uint64_t c) { return (uint32_t)((c + SBFE_BLOCK - 1u) / SBFE_BLOCK); };

    if (f_words) SB_HIP(e, hipMemsetAsync(d_f, 0, f_words * sizeof(int32_t), e->stream));
    SB_HIP(e, hipMemsetAsync(d_acc, 0, SBFE_NACC * sizeof(unsigned long long), e->stream));
    if (d_tension && maxB) SB_HIP(e, hipMemsetAsync(d_tension, 0, (size_t)maxB * sizeof(float), e->stream)); // +0 where no evaluated beam lives
    if (n)
        k_forces_beams<<<blocks(n), SBFE_BLOCK, 0, e->stream>>>(s.buf[SBQ_B_TAB].as<uint32_t>(), n, s.buf[SBX_B_ROW].as<uint32_t>(),
                                                                s.buf[SBQ_B_MAT].as<float2>(), d_pinv, cur.pos, e->beams.target, e->beams.last, sbq_dead(e),
                                                                maxB, d_f, d_tension, d_acc);
    if (contacts && P) {
        SB_HIP(e, hipMemsetAsync(d_cells, 0, ncell * sizeof(uint32_t), e->stream));
        k_forces_bin<<<blocks(P), SBFE_BLOCK, 0, e->stream>>>(P, cur.pos, geo, d_cells, d_cell_of);
        sbq_scan<uint32_t>(e, d_cells, ncell, d_bsum, d_cells, nullptr);
        k_forces_scatter<<<blocks(P), SBFE_BLOCK, 0, e->stream>>>(P, cur.pos, e->d_pslot, d_cell_of, d_cells, d_sorted);
        k_forces_visit<<<blocks(P), SBFE_BLOCK, 0, e->stream>>>(d_sorted, P, d_cells, geo, k, d_islot, e->d_pidx, cur.pos, cur.vel, d_labels, maxP, d_f,
                                                                d_rows, d_acc);
    }
    if (d_rows && maxP) k_forces_fill<<<blocks(maxP), SBFE_BLOCK, 0, e->stream>>>(d_pinv, np, maxP, d_rows);
    if (d_counts) k_forces_counts<<<1, 64, 0, e->stream>>>(d_acc, d_counts, P);
    SB_HIP(e, hipGetLastError());
    return mir.finish();
}

// what sb_get_info reads ("forces_table_build_us", "forces_cells_per_side", "forces_kernel_vgprs", "forces_kernel_scratch_bytes")
bool sbfe_info(sb_engine *e, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "forces_table_build_us") *value = e->sio ? (uint64_t)(e->sio->for_build_ms * 1000.0 + 0.5) : 0u;
    else if (k == "forces_cells_per_side") { // of the scene as it is now (1: all pairs)
        SbcGeo geo;
        (void)sbc_geometry(e, &geo);
        *value = geo.G;
    }
    else if (k == "forces_kernel_vgprs" || k == "forces_kernel_scratch_bytes") { // the most over every kernel a call may launch
        std::vector<const void *> ks = {(const void *)k_forces_beams, (const void *)k_forces_bin, (const void *)k_forces_scatter,
                                        (const void *)k_forces_visit, (const void *)k_forces_fill, (const void *)k_forces_counts};
        for (const void *f : sbq_scan_kernels(false)) ks.push_back(f);
        return sbq_kernel_most(e, ks, k == "forces_kernel_vgprs", value);
    }
    else return false;
    return true;
}

extern "C" {

sb_status sb_forces_device(sb_engine *e, const sb_forces_options *opts, const void *device_labels_i32, void *device_rows_f32, void *device_beam_i32,
                           void *device_tension_f32, void *device_counts_i64)
{
    SB_GUARDED(e, sbfe_enqueue(e, opts, device_labels_i32, device_rows_f32, device_beam_i32, device_tension_f32, device_counts_i64, false))
}

sb_status sb_forces(sb_engine *e, const sb_forces_options *opts, const int32_t *labels, float *rows, int32_t *beam_i32, float *tension, int64_t *counts)
{
    SB_GUARDED(e, sbfe_enqueue(e, opts, labels, rows, beam_i32, tension, counts, true))
}

} // extern "C"
