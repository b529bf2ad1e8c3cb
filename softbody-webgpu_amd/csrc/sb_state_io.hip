// sb_state_io.hip -- the engine's state in device memory (sb_read_state_device / sb_write_particles_device of include/softbody.h)
// for gfx950 (CDNA4, wave64).
//
// Export: the bytes sb_load_buffers would write at this point of the stream, gathered on the device -- particle records
// (p.xy, v.xy, a.xy: 24 B) at each particle's DATA index, the four state floats of each beam of the latest upload at its data
// index, and a live byte per beam.  Import: p, v, a of every particle from records in the same layout, scattered
// into the current particle buffer; the per-tile acceleration flags are raised where an imported acceleration has a nonzero bit
// (as k_halo_unpack does), and the host side drops every promise about positions the engine carries across calls (the spatial
// hash, the hybrid's verdict).  Plain loads and stores: no arithmetic touches a value.
// Beam import (sb_write_beams_device): target_length and / or last_length of every beam of the latest upload from rows in the
// export's layout, into every copy the engine keeps of the beam.  Checkpoint / restore (sb_checkpoint_device / sb_restore_device):
// a copy of everything a run mutates, in device memory, and back.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <stdexcept>
#include <vector>

#include "sb_report.h"

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

// beam import, tiled / atomic layout: a lane per beam COPY (a beam cut by tiles has one per tile, and each is written).  Its engine
// slot from the per-copy slot word, its row through the per-upload table engine slot -> data index; the two floats travel as words.
__global__ __launch_bounds__(SBS_BLOCK) void k_state_import_beams(const uint2 *__restrict__ src, const uint32_t *__restrict__ slot,
                                                                  const uint32_t *__restrict__ row_of_slot, uint32_t ncopies, uint32_t nslots,
                                                                  uint32_t max_beams, uint32_t fields, uint32_t *target, uint32_t *last)
{
    const uint32_t c = blockIdx.x * SBS_BLOCK + threadIdx.x;
    if (c >= ncopies) return;
    const uint32_t s = slot[c];
    if (s >= nslots) return; // (a padding copy: 0xFFFFFFFF)
    const uint32_t r = row_of_slot[s];
    if (r >= max_beams) return; // (a beam an upload removed: not in the caller's buffers any more)
    const uint2 v = src[(size_t)r * 2u]; // {target_length, last_length} of the 16-byte row
    if (fields & SB_BEAM_TARGET_LENGTH) target[c] = v.x;
    if (fields & SB_BEAM_LAST_LENGTH) last[c] = v.y;
}

// beam import, blocked layout: a lane per blocked beam (one state slot each, owner order).  The target goes into BOTH halves of the
// double buffer (a tile that never yields never stores its targets: blocked_state_to_device, sb_api.hip), last into the current
// half; a target that differs from the beam's rest length by bits raises its tile's plastic flag in both rows (the upload's own
// memcmp rule; a flag an import could lower again stays raised -- the next delete pass recounts, k_plastic_recount).  The rest
// length comes from a per-upload float table in owner order: one coalesced load, and the tile is searched only where it is needed.
__global__ __launch_bounds__(SBS_BLOCK) void k_state_import_beams_blocked(const uint2 *__restrict__ src, const uint32_t *__restrict__ slot,
                                                                          const uint32_t *__restrict__ row_of_slot,
                                                                          const uint32_t *__restrict__ rest, uint32_t nbeams, uint32_t nslots,
                                                                          uint32_t max_beams, uint32_t fields, uint32_t *target_a,
                                                                          uint32_t *target_b, uint32_t *last_cur, uint32_t *plastic_a,
                                                                          uint32_t *plastic_b, const uint32_t *__restrict__ tile_b0,
                                                                          uint32_t ntiles)
{
    const uint32_t g = blockIdx.x * SBS_BLOCK + threadIdx.x;
    if (g >= nbeams) return;
    const uint32_t s = slot[g];
    if (s >= nslots) return;
    const uint32_t r = row_of_slot[s];
    if (r >= max_beams) return;
    const uint2 v = src[(size_t)r * 2u];
    if (fields & SB_BEAM_TARGET_LENGTH) {
        target_a[g] = v.x;
        target_b[g] = v.x;
        if (v.x != rest[g]) {
            const uint32_t tile = sb_range_of(tile_b0, ntiles, g);
            SB_AGENT_STORE(&plastic_a[tile], 1u);
            SB_AGENT_STORE(&plastic_b[tile], 1u);
        }
    }
    if (fields & SB_BEAM_LAST_LENGTH) last_cur[g] = v.y;
}

// ---------------------------------------------------------------- host side

void sbs_drop_checkpoint(sb_engine *e)
{
    if (!e || !e->sio || !e->sio->buf[SBS_B_CKPT].p) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream); // (a restore in flight still reads it)
    e->sio->buf[SBS_B_CKPT].release();
    e->sio->ckpt_bytes = 0;
}

// every call of this file: an upload, no ranks (sbq_ready also makes the device current)
static sb_status sbs_check(sb_engine *e, const char *what) { return sbq_ready(e, what, "ranks are not handled"); }

// per caller beam slot of the latest upload: its engine slot and the data index of its record (sb_load_buffers' beam loop)
static sb_status sbs_build_tables(sb_engine *e)
{
    SbStateIoState &s = *e->sio;
    std::vector<uint2> slots;
    SB_TRY(sbq_user_slots(e, "sb_read_state_device", slots));
    SB_TRY(s.buf[SBS_B_SLOT].grow(e, slots.size() * sizeof(uint2)));
    SB_HIP(e, hipMemcpyAsync(s.buf[SBS_B_SLOT].p, slots.data(), slots.size() * sizeof(uint2), hipMemcpyHostToDevice, e->stream));
    SB_HIP(e, hipStreamSynchronize(e->stream)); // (the host vector goes out of scope)
    s.valid = true;
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
        if (!e->sio->valid) SB_TRY(sbs_build_tables(e));
        const uint32_t *copy = nullptr;
        SB_TRY(sbr_copy_table(e, &copy));
        const uint32_t nslots = sb_user_beams(e);
        const uint32_t *dead = sbq_dead(e);
        k_state_export_beams<<<(nslots + SBS_BLOCK - 1) / SBS_BLOCK, SBS_BLOCK, 0, e->stream>>>(
            e->sio->buf[SBS_B_SLOT].as<uint2>(), nslots, copy, e->beams.target, e->beams.last, e->beams.strain, e->beams.stress, dead, (float4 *)beams,
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

// ---- beam import

// per ENGINE beam slot the data index of its record in the latest upload (the caller's slots through sb_user_slot and the latest
// mapping: the call works after an upload that cut beams, whose slots get 0xFFFFFFFF); blocked layout: the rest length per blocked
// beam.  The first import after an upload builds them and waits once, as the first export does.
static sb_status sbs_build_import_tables(sb_engine *e)
{
    const auto t0 = std::chrono::steady_clock::now();
    SbStateIoState &s = *e->sio;
    const uint32_t Bu = sb_user_beams(e);
    std::vector<uint2> slots;
    SB_TRY(sbq_user_slots(e, "sb_write_beams_device", slots));
    std::vector<uint32_t> row(std::max<uint32_t>(e->B, 1), 0xFFFFFFFFu);
    for (uint32_t u = 0; u < Bu; u++) row[slots[u].x] = slots[u].y;
    std::vector<float> rest;
    if (e->bk.K) {
        if (e->bk.h_beam_slot.size() != e->nbeam) SB_FAIL(e, SB_ERR_STATE, "sb_write_beams_device: %zu beams in the host map, %u on the device", e->bk.h_beam_slot.size(), e->nbeam);
        rest.resize(std::max<uint32_t>(e->nbeam, 1), 0.0f);
        sbt::parallel_ranges(e->nbeam, 1 << 16, [&](size_t g0, size_t g1) {
            for (size_t g = g0; g < g1; g++) rest[g] = e->h_beams[e->bk.h_beam_slot[g]].f[0];
        });
    }
    SB_TRY(s.buf[SBS_B_IMP_ROW].grow(e, row.size() * 4));
    SB_HIP(e, hipMemcpyAsync(s.buf[SBS_B_IMP_ROW].p, row.data(), row.size() * 4, hipMemcpyHostToDevice, e->stream));
    if (!rest.empty()) {
        SB_TRY(s.buf[SBS_B_IMP_REST].grow(e, rest.size() * 4));
        SB_HIP(e, hipMemcpyAsync(s.buf[SBS_B_IMP_REST].p, rest.data(), rest.size() * 4, hipMemcpyHostToDevice, e->stream));
    }
    SB_HIP(e, hipStreamSynchronize(e->stream)); // (the host vectors go out of scope)
    s.imp_valid = true;
    s.imp_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SB_OK;
}

static sb_status sbs_write_beams(sb_engine *e, const void *beams, uint32_t fields)
{
    if (!e) return SB_ERR_INVALID;
    if (!beams) SB_FAIL(e, SB_ERR_INVALID, "sb_write_beams_device: null source");
    if ((uintptr_t)beams & 15u) SB_FAIL(e, SB_ERR_INVALID, "sb_write_beams_device: beam rows need a 16-byte aligned buffer");
    if (fields == 0u || (fields & ~(SB_BEAM_TARGET_LENGTH | SB_BEAM_LAST_LENGTH)))
        SB_FAIL(e, SB_ERR_INVALID, "sb_write_beams_device: fields 0x%x is not a mask of SB_BEAM_TARGET_LENGTH / SB_BEAM_LAST_LENGTH", fields);
    SB_TRY(sbs_check(e, "sb_write_beams_device"));
    const uint32_t nc = e->nbeam;
    if (!nc || !sb_user_beams(e)) return SB_OK;
    if (!e->sio->imp_valid) SB_TRY(sbs_build_import_tables(e));
    const SbStateIoState &s = *e->sio;
    const uint32_t blocks = (nc + SBS_BLOCK - 1) / SBS_BLOCK;
    if (e->bk.K) {
        const SbBlockedDev &k = e->bk;
        k_state_import_beams_blocked<<<blocks, SBS_BLOCK, 0, e->stream>>>(
            (const uint2 *)beams, e->beams.slot, s.buf[SBS_B_IMP_ROW].as<uint32_t>(), s.buf[SBS_B_IMP_REST].as<uint32_t>(), nc, e->B, e->opt.max_beams, fields,
            (uint32_t *)k.d_target[0], (uint32_t *)k.d_target[1], (uint32_t *)k.d_last[k.cur], k.d_plastic[0], k.d_plastic[1], k.d_tile_b0,
            k.ntiles);
    } else {
        // (SB_COLLIDE_GRID with a blocked plan beside the tiling: that plan borrows target / last from these arrays and recomputes its
        // plastic flags at the start of every run -- k_hybrid_to_blocked, sb_blocked.hip:676 -- so the tiled layout is all there is to write)
        k_state_import_beams<<<blocks, SBS_BLOCK, 0, e->stream>>>((const uint2 *)beams, e->beams.slot, s.buf[SBS_B_IMP_ROW].as<uint32_t>(), nc, e->B,
                                                                  e->opt.max_beams, fields, (uint32_t *)e->beams.target,
                                                                  (uint32_t *)e->beams.last);
    }
    SB_HIP(e, hipGetLastError());
    return SB_OK; // (beams do not move particles: the spatial hash and the hybrid's verdict stay as they are)
}

// ---- checkpoint / restore

// WHAT A RUN MUTATES -- the one list sb_checkpoint_device and sb_restore_device walk (DESIGN.md 4.2 has the same table).  A flag,
// mask or counter added to reset_run_state (sb_api.hip) belongs in one of these rows too:
//
//   state                                              written by                          checkpoint / restore
//   -------------------------------------------------  ----------------------------------  --------------------------------------------
//   part[cur] pos / vel / acc, e->cur                  every substep, particle import      restored (the current buffer and its number)
//   part[cur ^ 1]                                      every substep (scratch between)     not part (fully rewritten, but see next row)
//   d_acc_flag[cur]                                    every substep, particle import      restored
//   d_acc_flag[cur ^ 1]                                every substep                       reset: raised (0 would promise zeros in a
//                                                                                          buffer the checkpoint does not hold)
//   d_forces (atomic path)                             k_beams_atomic / k_particles        restored
//   beams.target / last / strain / stress              every substep, beam import          restored
//     blocked: bk.d_target[0..1], bk.d_last[bk.cur],                                       restored (both target halves, the current
//     bk.d_strain / d_stress, bk.cur, bk.d_plastic[0..1]                                   half of last, both plastic rows)
//   d_broken                                           every substep, delete pass          restored (flags pending mid-frame)
//   d_dead_gen, e->delete_gen                          delete pass                         restored
//   bk.d_ent_word | beams.pair | beams.ia              delete pass (dummies)               restored (from the checkpoint, not from
//                                                                                          d_ent_word0 / d_live0: it may be after a pass)
//   e->substeps_done                                   every substep                       restored
//   spatial hash (d_head, d_grid_ctl, lists, grid_*)   every substep                       reset (sb_grid_reset_hash): bits do not depend
//   hy.slow_chunk / slow_left                          hybrid_substeps                     reset to 0 (a fresh look)
//   hy.d_ent_word, hy.synced_delete_gen                k_hybrid_sync_dead                  reset: from hy.d_ent_word0, 0 (the next run
//                                                                                          reads d_dead_gen's beams again)
//   hy.d_target / d_last / d_plastic / d_broken ...    a hybrid run                        not part (borrowed anew by every run)
//   hy.rate, fail_streak, launch and grid statistics   host heuristics / counters          not part (no bit depends on them)
//   e->consts (physics constants, user input)          the caller                          not part (as the batch's reset)
//   *dev_err                                           peer exchange                       not part (no peers: sbs_check)
//   a hybrid plan pending on the side thread           upload                              not part (depends on the topology only)
struct SbRunItem {
    void *p;
    size_t bytes;
};
// `cur` / `bcur`: the particle buffer and the blocked beam-state half the list is about (the engine's now, or the checkpoint's)
static void sbs_walk_run_state(const sb_engine *e, uint32_t cur, uint32_t bcur, std::vector<SbRunItem> &out)
{
    out.clear();
    auto add = [&](const void *p, size_t bytes) {
        if (p && bytes) out.push_back(SbRunItem{const_cast<void *>(p), bytes});
    };
    const size_t P = e->P, nc = e->nbeam, B = e->B, T = e->ntiles;
    const SbParticleArrays &c = e->part[cur];
    add(c.pos, P * sizeof(float2));
    add(c.vel, P * sizeof(float2));
    add(c.acc, P * sizeof(float2));
    if (e->path == SB_PATH_TILED) add(e->d_acc_flag[cur], T * 4);
    if (e->path == SB_PATH_ATOMIC) add(e->d_forces, P * sizeof(int2));
    if (e->bk.K) {
        const SbBlockedDev &k = e->bk;
        add(k.d_target[0], nc * 4);
        add(k.d_target[1], nc * 4);
        add(k.d_last[bcur], nc * 4);
        add(k.d_strain, nc * 4);
        add(k.d_stress, nc * 4);
        add(k.d_plastic[0], (size_t)k.ntiles * 4);
        add(k.d_plastic[1], (size_t)k.ntiles * 4);
        add(k.d_ent_word, (size_t)k.entries * 4);
    } else {
        add(e->beams.target, nc * 4);
        add(e->beams.last, nc * 4);
        add(e->beams.strain, nc * 4);
        add(e->beams.stress, nc * 4);
        add(e->path == SB_PATH_TILED ? e->beams.pair : e->beams.ia, e->live_words * 4);
    }
    add(e->d_broken, (nc + 31) / 32 * 4);
    add(e->d_dead_gen, B * 4);
}
static inline size_t sbs_item_stride(size_t bytes) { return (bytes + 255u) & ~(size_t)255u; }

static sb_status sbs_checkpoint(sb_engine *e)
{
    if (!e) return SB_ERR_INVALID;
    SB_TRY(sbs_check(e, "sb_checkpoint_device"));
    SbStateIoState &s = *e->sio;
    SbDevBuf &ck = s.buf[SBS_B_CKPT];
    std::vector<SbRunItem> items;
    sbs_walk_run_state(e, e->cur, e->bk.cur, items);
    size_t total = 0;
    for (const SbRunItem &it : items) total += sbs_item_stride(it.bytes);
    total = std::max<size_t>(total, 256);
    if (!ck.p || ck.cap < total) { // (the first checkpoint after an upload: every later one finds the block)
        sbs_drop_checkpoint(e);
        void *blk = nullptr;
        if (hipMalloc(&blk, total) != hipSuccess) {
            (void)hipGetLastError();
            SB_FAIL(e, SB_ERR_OOM, "sb_checkpoint_device: no device memory for %zu bytes (the engine is unchanged; there is no checkpoint)", total);
        }
        ck.p = blk;
        ck.cap = total;
    }
    size_t off = 0;
    for (const SbRunItem &it : items) {
        SB_HIP(e, hipMemcpyAsync(ck.as<uint8_t>() + off, it.p, it.bytes, hipMemcpyDeviceToDevice, e->stream));
        off += sbs_item_stride(it.bytes);
    }
    s.ck_cur = e->cur;
    s.ck_bcur = e->bk.cur;
    s.ck_delete_gen = e->delete_gen;
    s.ck_substeps_done = e->substeps_done;
    s.ckpt_bytes = total;
    s.checkpoints++;
    return SB_OK;
}

static sb_status sbs_restore(sb_engine *e)
{
    if (!e) return SB_ERR_INVALID;
    SB_TRY(sbs_check(e, "sb_restore_device"));
    if (!e->sio->buf[SBS_B_CKPT].p || !e->sio->ckpt_bytes) SB_FAIL(e, SB_ERR_STATE, "sb_restore_device without a checkpoint (sb_checkpoint_device; every upload drops it)");
    SbStateIoState &s = *e->sio;
    std::vector<SbRunItem> items;
    sbs_walk_run_state(e, s.ck_cur, s.ck_bcur, items);
    size_t off = 0;
    for (const SbRunItem &it : items) {
        SB_HIP(e, hipMemcpyAsync(it.p, s.buf[SBS_B_CKPT].as<const uint8_t>() + off, it.bytes, hipMemcpyDeviceToDevice, e->stream));
        off += sbs_item_stride(it.bytes);
    }
    if (off > s.ckpt_bytes) SB_FAIL(e, SB_ERR_STATE, "sb_restore_device: the checkpoint holds %zu bytes, the scene's run state %zu", s.ckpt_bytes, off);
    // the host's words of the run state
    e->cur = s.ck_cur;
    e->delete_gen = s.ck_delete_gen;
    e->substeps_done = s.ck_substeps_done;
    if (e->bk.K) {
        e->bk.cur = s.ck_bcur;
        e->beams.target = e->bk.d_target[e->bk.cur];
        e->beams.last = e->bk.d_last[e->bk.cur];
    }
    // the other particle buffer is not part of the checkpoint: no promise about its accelerations
    if (e->path == SB_PATH_TILED && e->ntiles) SB_HIP(e, hipMemsetAsync(e->d_acc_flag[e->cur ^ 1u], 0x01, (size_t)e->ntiles * 4, e->stream));
    // what the engine promised itself about where the particles are: as the particle import (sbs_write)
    SB_TRY(sb_grid_reset_hash(e));
    e->hy.slow_chunk = e->hy.slow_left = 0;
    // the blocked plan beside the tiling: its entries as uploaded; its next run reads the removed beams from the tiled layout again
    if (e->hy.K && e->hy.synced_delete_gen && e->hy.entries)
        SB_HIP(e, hipMemcpyAsync(e->hy.d_ent_word, e->hy.d_ent_word0, (size_t)e->hy.entries * 4, hipMemcpyDeviceToDevice, e->stream));
    e->hy.synced_delete_gen = 0;
    s.restores++;
    return SB_OK;
}

bool sbs_info(sb_engine *e, const char *key, uint64_t *value)
{
    const std::string k(key);
    const SbStateIoState *s = e->sio;
    if (k == "checkpoint_bytes") *value = s ? s->ckpt_bytes : 0;
    else if (k == "checkpoints") *value = s ? s->checkpoints : 0;
    else if (k == "restores") *value = s ? s->restores : 0;
    else if (k == "beam_import_table_build_us") *value = s ? (uint64_t)(s->imp_build_ms * 1000.0 + 0.5) : 0;
    else return false;
    return true;
}

extern "C" {

sb_status sb_write_beams_device(sb_engine *e, const void *device_beams, uint32_t fields) { SB_GUARDED(e, sbs_write_beams(e, device_beams, fields)) }
sb_status sb_checkpoint_device(sb_engine *e) { SB_GUARDED(e, sbs_checkpoint(e)) }
sb_status sb_restore_device(sb_engine *e) { SB_GUARDED(e, sbs_restore(e)) }

sb_status sb_read_state_device(sb_engine *e, void *device_particles, void *device_beams, void *device_beam_alive)
{
    SB_GUARDED(e, sbs_read(e, device_particles, device_beams, device_beam_alive))
}
sb_status sb_write_particles_device(sb_engine *e, const void *device_particles) { SB_GUARDED(e, sbs_write(e, device_particles)) }

} // extern "C"
