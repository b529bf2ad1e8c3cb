// sb_state_io.hip -- the engine's state in device memory (sb_read_state_device / sb_write_particles_device of include/softbody.h)
// for gfx950 (CDNA4, wave64).
//
// Export: the bytes sb_load_buffers would write at this point of the stream, gathered on the device -- particle records
// (p.xy, v.xy, a.xy: 24 B) at each particle's DATA index, the four state floats of each beam of the latest upload at its data
// index, and a live byte per beam.  Import: p, v, a of every particle from records in the same layout, scattered
// into the current particle buffer; the per-tile acceleration flags are raised where an imported acceleration has a nonzero bit
// (as k_halo_unpack does), and the host side drops every promise about positions the engine carries across calls (the spatial
// hash, the hybrid's verdict).  Plain loads and stores: no arithmetic touches a value.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <stdexcept>
#include <vector>

#include "sb_engine.h"

#define SBS_BLOCK 256

// ---------------------------------------------------------------- kernels

// particle export: a lane per internal index, the 24-byte record at its data index (reads coalesce; writes scatter by the tile
// order of the internal indices, which keeps neighbouring lanes mostly on neighbouring records)
__global__ __launch_bounds__(SBS_BLOCK) void k_state_export_particles(const float2 *__restrict__ pos, const float2 *__restrict__ vel,
                                                                      const float2 *__restrict__ acc,
                                                                      const uint32_t *__restrict__ pidx, uint32_t P, float2 *out)
{
    const uint32_t i = blockIdx.x * SBS_BLOCK + threadIdx.x;
    if (i >= P) return;
    float2 *o = out + (size_t)pidx[i] * 3u;
    o[0] = pos[i];
    o[1] = vel[i];
    o[2] = acc[i];
}

// beam export: a lane per caller slot, {target_length, last_length, strain, stress} of the copy read back for its engine slot, and
// whether a delete pass (or a plan-keeping upload) removed it, at the slot's data index
__global__ __launch_bounds__(SBS_BLOCK) void k_state_export_beams(const uint2 *__restrict__ slots, uint32_t n,
                                                                  const uint32_t *__restrict__ copy, const float *__restrict__ target,
                                                                  const float *__restrict__ last, const float *__restrict__ strain,
                                                                  const float *__restrict__ stress,
                                                                  const uint32_t *__restrict__ dead, float4 *beams, uint8_t *alive)
{
    const uint32_t u = blockIdx.x * SBS_BLOCK + threadIdx.x;
    if (u >= n) return;
    const uint2 t = slots[u]; // engine slot, data index
    if (beams) {
        const uint32_t c = copy[t.x];
        beams[t.y] = make_float4(target[c], last[c], strain[c], stress[c]);
    }
    if (alive) alive[t.y] = (dead && dead[t.x] != 0u) ? 0u : 1u;
}

// particle import: a lane per internal index, its record read at its data index (k_halo_unpack's particle half)
__global__ __launch_bounds__(SBS_BLOCK) void k_state_import_particles(const float2 *__restrict__ src, const uint32_t *__restrict__ pidx,
                                                                      uint32_t P, float2 *pos, float2 *vel, float2 *acc,
                                                                      uint32_t *acc_flag, const uint32_t *__restrict__ tile_p0,
                                                                      uint32_t ntiles)
{
    const uint32_t i = blockIdx.x * SBS_BLOCK + threadIdx.x;
    if (i >= P) return;
    const float2 *in = src + (size_t)pidx[i] * 3u;
    const float2 a = in[2];
    pos[i] = in[0];
    vel[i] = in[1];
    acc[i] = a;
    if (acc_flag && ((__float_as_uint(a.x) | __float_as_uint(a.y)) != 0u)) // (-0.0 counts, as in the substep kernels)
        SB_AGENT_STORE(&acc_flag[sb_range_of(tile_p0, ntiles, i)], 1u);
}

// ---------------------------------------------------------------- host side

void sbs_invalidate(sb_engine *e)
{
    if (e && e->sio) e->sio->valid = e->sio->sum_valid = e->sio->bod_valid = e->sio->con_valid = e->sio->bsm_valid = false;
}

void sbs_release(sb_engine *e)
{
    if (!e || !e->sio) return;
    void *ps[] = {e->sio->d_slot, e->sio->d_sum_pinv, e->sio->d_sum_bleaf, e->sio->d_sum_part, e->sio->d_sum_stat, e->sio->d_sum_out,
                  e->sio->d_bod_pinv, e->sio->d_bod_tab, e->sio->d_bod_parent, e->sio->d_bod_sizes, e->sio->d_bod_acc,
                  e->sio->d_bsm_pinv, e->sio->d_bsm_tab, e->sio->d_bsm, e->sio->d_bsm_labels, e->sio->d_bsm_out};
    for (void *p : ps)
        if (p) (void)hipFree(p);
    for (void *p : e->sio->d_con)
        if (p) (void)hipFree(p);
    delete e->sio;
    e->sio = nullptr;
}

static sb_status sbs_check(sb_engine *e, const char *what)
{
    if (!e->loaded) SB_FAIL(e, SB_ERR_STATE, "%s before sb_write_buffers", what);
    if (e->halo_configured || e->n_ghost_p || e->n_send_p || e->n_ghost_b || e->n_send_b || e->n_peers || e->mailbox)
        SB_FAIL(e, SB_ERR_UNSUPPORTED, "%s: the engine has ghost zones or peers configured (ranks are not handled)", what);
    SB_HIP(e, hipSetDevice(e->device));
    return SB_OK;
}

// per caller beam slot of the latest upload: its engine slot and the data index of its record (sb_load_buffers' beam loop)
static sb_status sbs_build_tables(sb_engine *e)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (!e->sio) e->sio = new SbStateIoState();
    SbStateIoState &s = *e->sio;
    const uint32_t maxP = e->opt.max_particles, Bu = sb_user_beams(e);
    std::vector<uint2> slots(std::max<uint32_t>(Bu, 1));
    sbt::parallel_ranges(Bu, 1 << 16, [&](size_t u0, size_t u1) {
        for (size_t u = u0; u < u1; u++) slots[u] = make_uint2(sb_user_slot(e, u), map_get(e, e->h_mapping.data(), (size_t)maxP + u));
    });
    for (uint32_t u = 0; u < Bu; u++)
        if (slots[u].x >= e->B || slots[u].y >= e->opt.max_beams) SB_FAIL(e, SB_ERR_STATE, "sb_read_state_device: beam slot outside the scene");
    if (!s.d_slot || s.cap_slot < slots.size()) {
        if (s.d_slot) {
            SB_HIP(e, hipStreamSynchronize(e->stream)); // an export in flight may still read it
            SB_HIP(e, hipFree(s.d_slot));
            s.d_slot = nullptr;
            s.cap_slot = 0;
        }
        SB_HIP(e, hipMalloc((void **)&s.d_slot, slots.size() * sizeof(uint2)));
        s.cap_slot = slots.size();
    }
    SB_HIP(e, hipMemcpyAsync(s.d_slot, slots.data(), slots.size() * sizeof(uint2), hipMemcpyHostToDevice, e->stream));
    SB_HIP(e, hipStreamSynchronize(e->stream)); // (the host vector goes out of scope)
    s.nslots = Bu;
    s.valid = true;
    s.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SB_OK;
}

static sb_status sbs_read(sb_engine *e, void *particles, void *beams, void *alive)
{
    if (!e) return SB_ERR_INVALID;
    SB_TRY(sbs_check(e, "sb_read_state_device"));
    if (((uintptr_t)particles & 7u) || ((uintptr_t)beams & 15u))
        SB_FAIL(e, SB_ERR_INVALID, "sb_read_state_device: particle records need 8-byte, beam rows 16-byte aligned buffers");
    const uint32_t P = e->P;
    if (particles && P) {
        const SbParticleArrays &c = e->part[e->cur];
        k_state_export_particles<<<(P + SBS_BLOCK - 1) / SBS_BLOCK, SBS_BLOCK, 0, e->stream>>>(c.pos, c.vel, c.acc, e->d_pidx, P,
                                                                                              (float2 *)particles);
    }
    if ((beams || alive) && sb_user_beams(e)) {
        if (!e->sio || !e->sio->valid) SB_TRY(sbs_build_tables(e));
        const uint32_t *copy = nullptr;
        SB_TRY(sbr_copy_table(e, &copy));
        const SbStateIoState &s = *e->sio;
        const uint32_t *dead = e->B && e->delete_gen ? e->d_dead_gen : nullptr; // as sb_load_buffers (fetch_dead) sees it
        k_state_export_beams<<<(s.nslots + SBS_BLOCK - 1) / SBS_BLOCK, SBS_BLOCK, 0, e->stream>>>(
            s.d_slot, s.nslots, copy, e->beams.target, e->beams.last, e->beams.strain, e->beams.stress, dead, (float4 *)beams,
            (uint8_t *)alive);
    }
    SB_HIP(e, hipGetLastError());
    return SB_OK;
}

static sb_status sbs_write(sb_engine *e, const void *particles)
{
    if (!e) return SB_ERR_INVALID;
    SB_TRY(sbs_check(e, "sb_write_particles_device"));
    if (!particles) SB_FAIL(e, SB_ERR_INVALID, "sb_write_particles_device: null source");
    if ((uintptr_t)particles & 7u) SB_FAIL(e, SB_ERR_INVALID, "sb_write_particles_device: particle records need an 8-byte aligned buffer");
    const uint32_t P = e->P;
    if (P) {
        const SbParticleArrays &c = e->part[e->cur];
        uint32_t *flag = nullptr;
        const uint32_t *tile_p0 = nullptr;
        if (e->ntiles) { // (the blocked layout's tiles on the blocked path, as sbk_launch_halo_unpack)
            flag = e->d_acc_flag[e->cur];
            tile_p0 = e->bk.K ? e->bk.d_tile_p0 : e->d_tile_p0;
        }
        k_state_import_particles<<<(P + SBS_BLOCK - 1) / SBS_BLOCK, SBS_BLOCK, 0, e->stream>>>(
            (const float2 *)particles, e->d_pidx, P, c.pos, c.vel, c.acc, flag, tile_p0, e->ntiles);
        SB_HIP(e, hipGetLastError());
    }
    // Whatever the engine promised itself about where the particles are holds no more: the hash starts again (as after an upload
    // that keeps the plan), and the hybrid looks at the scene afresh at the start of the next call (hybrid_substeps honours
    // grid_force: single substeps until the new hash has made its lists).
    SB_TRY(sb_grid_reset_hash(e));
    e->hy.slow_chunk = e->hy.slow_left = 0;
    return SB_OK;
}

extern "C" {

sb_status sb_read_state_device(sb_engine *e, void *device_particles, void *device_beams, void *device_beam_alive)
{
    try {
        return sbs_read(e, device_particles, device_beams, device_beam_alive);
    } catch (const std::bad_alloc &) {
        if (e) e->err = "out of host memory";
        return SB_ERR_OOM;
    } catch (const std::exception &ex) {
        if (e) e->err = std::string("internal error: ") + ex.what();
        return SB_ERR_INVALID;
    }
}

sb_status sb_write_particles_device(sb_engine *e, const void *device_particles)
{
    try {
        return sbs_write(e, device_particles);
    } catch (const std::bad_alloc &) {
        if (e) e->err = "out of host memory";
        return SB_ERR_OOM;
    } catch (const std::exception &ex) {
        if (e) e->err = std::string("internal error: ") + ex.what();
        return SB_ERR_INVALID;
    }
}

} // extern "C"
