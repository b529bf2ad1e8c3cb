// sb_batch_spawn.hip -- adding particles ("spawns") in every scene of a batch in ONE launch; a reset undoes them
// (sb_batch_add_particles_device of include/softbody.h; gfx950, wave64).
//
// One workgroup per scene.  All lanes build, in LDS, the bitmap of the FREE particle data indices ("holds a particle" == 0 in the
// constant blob) with its prefix (sb_batch_alloc.h).  A lane per row takes the row's verdict (sb_batch_spawn_math.h); with
// SB_BATCH_SPAWN_SKIP_TOUCHING all lanes then sweep the current positions of the particle slots against the candidate rows with
// sb_touch, the step's own contact test.  Wave 0 finishes: rows against earlier rows, the allocator's finish (rank, room, the r-th
// free index, result and counts), the mapping entry, the "holds a particle" byte and the record, the count.  Every store is a
// plain vector store of this workgroup into its own scene.
#include "sb_batch.h"
#include "sb_batch_spawn_math.h"

#define SBS_BLOCK 256u

static_assert(SBA_COUNT_WORDS == SB_BATCH_SPAWN_COUNT_WORDS, "the count words of sb_batch_add_particles_device: added, invalid, blocked, full");
static_assert(SB_BATCH_ADD_MAX == 64u, "a lane of wave 0 per row, one ballot for the ranks");
static_assert(sizeof(sb_batch_new_particle) == SBA_ROW_WORDS * 4u, "a row is 8 words");
static_assert(sba::EMPTY == SB_BATCH_SPAWN_EMPTY && sba::INVALID == SB_BATCH_SPAWN_INVALID && sbs::SBS_BLOCKED == SB_BATCH_SPAWN_BLOCKED &&
                  sba::FULL == SB_BATCH_SPAWN_FULL,
              "the row codes");
static_assert(sbs::SBS_DRY_RUN == SB_BATCH_SPAWN_DRY_RUN && sbs::SBS_SKIP_TOUCHING == SB_BATCH_SPAWN_SKIP_TOUCHING, "the flags");

#define SBS_MAX_BITMAP_WORDS ((SB_BATCH_MAX_PARTICLES + 31u) / 32u) // the capacity of a scene is at most SB_BATCH_MAX_PARTICLES
static_assert(SBS_MAX_BITMAP_WORDS <= SBA_MAX_WORDS, "the free bitmap of the particle data indices");

__global__ __launch_bounds__(SBS_BLOCK) void k_batch_add_particles(SbBatchView V, float radius, const uint32_t *__restrict__ rows, uint32_t k,
                                                                   uint32_t flags, int32_t *__restrict__ result, int32_t *__restrict__ counts)
{
    __shared__ uint32_t s_row[SB_BATCH_ADD_MAX * SBA_ROW_WORDS]; // [64][8]
    __shared__ int32_t s_verd[SB_BATCH_ADD_MAX];                 // [64] steps 1 and 2
    __shared__ uint32_t s_hit[2];                                // bit j: row j touches a particle slot < P ("E(j)")
    __shared__ uint32_t s_free[SBS_MAX_BITMAP_WORDS];            // bit d: particle data index d is free
    __shared__ uint32_t s_pref[SBS_MAX_BITMAP_WORDS + 1u];       // free indices in front of each word; [npw]: all
    const uint32_t scene = blockIdx.x, tid = threadIdx.x;
    if (scene >= V.n_scenes) return;
    const uint32_t maxP = V.maxP, npw = sba::bitmap_words(maxP);

    const SbbScene hd = sbb_scene(V, scene);
    const uint32_t P = hd.P;
    unsigned char *cst = V.cst + (size_t)scene * V.cst_bytes, *st = V.st + (size_t)scene * V.st_bytes;
    uint32_t *g_pmap = (uint32_t *)(cst + V.o_pmap);
    float2 *g_part = (float2 *)(st + V.o_part);
    const bool dry = (flags & SB_BATCH_SPAWN_DRY_RUN) != 0u, skip_touching = (flags & SB_BATCH_SPAWN_SKIP_TOUCHING) != 0u;

    // ---- rows, the free bitmap
    for (uint32_t i = tid; i < k * SBA_ROW_WORDS; i += SBS_BLOCK) s_row[i] = rows[(size_t)scene * k * SBA_ROW_WORDS + i];
    if (tid < 2u) s_hit[tid] = 0u;
    // (the "holds a particle" bytes: the row of them is padded to 16 bytes)
    sba::fill_free(s_free, s_pref, npw, (const uint32_t *)(cst + V.o_pex), nullptr, maxP, hd.loaded != 0u, tid, SBS_BLOCK);
    // ---- the verdict of each row, a lane per row
    if (tid < k) s_verd[tid] = sbs::row_verdict(s_row + tid * SBA_ROW_WORDS, hd.loaded != 0u);
    __syncthreads();

    // ---- touching a particle of the scene: every slot's current position against the candidate rows
    const SbTouchTest tt = sb_touch_test(radius);
    if (skip_touching) {
        for (uint32_t s = tid; s < P; s += SBS_BLOCK) {
            const uint32_t d = g_pmap[s];
            if (d >= maxP) continue; // (an upload is refused unless its particle data indices are inside the capacity)
            const float2 other = g_part[3u * d];
            for (uint32_t q = 0; q < k; q++) {
                const float2 me = make_float2(__uint_as_float(s_row[q * SBA_ROW_WORDS + 1u]), __uint_as_float(s_row[q * SBA_ROW_WORDS + 2u]));
                if (s_verd[q] == sba::CANDIDATE && sb_touch(me, other, tt.thr, tt.two_r)) atomicOr(&s_hit[q >> 5], 1u << (q & 31u));
            }
        }
        __syncthreads();
    }
    if (tid >= 64u) return; // wave 0 finishes (k <= 64: a lane per row)

    // ---- rows against earlier rows, room, the r-th free index
    const bool row = tid < k;
    const uint32_t *w = s_row + (row ? tid : 0u) * SBA_ROW_WORDS;
    int32_t verd = row ? s_verd[tid] : (int32_t)sba::EMPTY;
    if (skip_touching && verd == sba::CANDIDATE) {
        const float2 me = make_float2(__uint_as_float(w[1]), __uint_as_float(w[2]));
        const bool blocked = sbs::blocked(
            tid, ((s_hit[tid >> 5] >> (tid & 31u)) & 1u) != 0u, [&](uint32_t i) { return s_verd[i]; },
            [&](uint32_t i) { return ((s_hit[i >> 5] >> (i & 31u)) & 1u) != 0u; },
            [&](uint32_t i) {
                return sb_touch(me, make_float2(__uint_as_float(s_row[i * SBA_ROW_WORDS + 1u]), __uint_as_float(s_row[i * SBA_ROW_WORDS + 2u])), tt.thr, tt.two_r);
            });
        if (blocked) verd = sbs::SBS_BLOCKED;
    }
    const sba::Finish f = sba::finish(verd, tid, P, maxP, s_free, s_pref, npw);
    const uint32_t d = f.index, n_add = f.n_added;

    if (!dry && n_add != 0u) {
        if (f.add) { // (d < maxP and P + rank < maxP: the room test of the finish)
            g_pmap[P + f.rank] = d;
            (cst + V.o_pex)[d] = 1;
            g_part[3u * d] = make_float2(__uint_as_float(w[1]), __uint_as_float(w[2]));
            g_part[3u * d + 1u] = make_float2(__uint_as_float(w[3]), __uint_as_float(w[4]));
            g_part[3u * d + 2u] = make_float2(__uint_as_float(w[5]), __uint_as_float(w[6]));
        }
        // (the count: written at agent scope, as every kernel of the batch reads it)
        if (tid == 0u) SB_AGENT_STORE(&V.meta[(size_t)scene * SB_BM_WORDS + SB_BM_P], P + n_add);
    }
    sba::report(f, row, tid, scene, k, result, counts);
}

// ---------------------------------------------------------------- host
bool sbb_spawn_info(sb_batch *b, const char *key, uint64_t *value)
{
    return sbb_kernel_info(b, "add_particles", (const void *)k_batch_add_particles, b->spawn_res, key, value);
}

sb_status sb_batch_add_particles_device(sb_batch *b, uint32_t flags, const void *device_rows, uint32_t k, void *device_result_i32,
                                        void *device_counts_i32)
{
    SB_TRY(sbb_edit_entry(b, "sb_batch_add_particles_device", flags, SB_BATCH_SPAWN_DRY_RUN | SB_BATCH_SPAWN_SKIP_TOUCHING,
                          "SB_BATCH_SPAWN_DRY_RUN and _SKIP_TOUCHING are", k, SB_BATCH_ADD_MAX, "rows", device_rows,
                          {device_rows, device_result_i32, device_counts_i32}, "rows, result and counts"));
    k_batch_add_particles<<<b->opt.n_scenes, SBS_BLOCK, 0, b->stream>>>(b->V, b->prm.particle_radius, (const uint32_t *)device_rows, k, flags,
                                                                        (int32_t *)device_result_i32, (int32_t *)device_counts_i32);
    return check_launch(b, "sb_batch_add_particles_device");
}
