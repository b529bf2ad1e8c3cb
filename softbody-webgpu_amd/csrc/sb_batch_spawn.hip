// sb_batch_spawn.hip -- adding particles ("spawns") in every scene of a batch in ONE launch; a reset undoes them
// (sb_batch_add_particles_device of include/softbody.h; gfx950, wave64).
//
// One workgroup per scene.  All lanes build, in LDS, a bitmap of the FREE particle data indices ("holds a particle" == 0 in the
// constant blob) with a popcount prefix over its words.  A lane per row takes the row's verdict (sb_batch_spawn_math.h); with
// SB_BATCH_SPAWN_SKIP_TOUCHING all lanes then sweep the current positions of the particle slots against the candidate rows with
// sb_touch, the step's own contact test.  Wave 0 finishes: rows against earlier rows, ranks from one ballot, the r-th free index
// from the prefix, the mapping entry, the "holds a particle" byte and the record, the count.  Every store is a plain vector store
// of this workgroup into its own scene.
#include <string>

#include "sb_batch.h"
#include "sb_batch_spawn_math.h"

#define SBS_BLOCK 256u
enum { SBS_ADDED, SBS_N_INVALID, SBS_N_BLOCKED, SBS_N_FULL, SBS_NWORDS };

static_assert(SBS_NWORDS == SB_BATCH_SPAWN_COUNT_WORDS, "the count words of sb_batch_add_particles_device");
static_assert(SB_BATCH_ADD_MAX == 64u, "a lane of wave 0 per row, one ballot for the ranks");
static_assert(sizeof(sb_batch_new_particle) == SBS_ROW_WORDS * 4u, "a row is 8 words");
static_assert(sbs::SBS_EMPTY == SB_BATCH_SPAWN_EMPTY && sbs::SBS_INVALID == SB_BATCH_SPAWN_INVALID && sbs::SBS_BLOCKED == SB_BATCH_SPAWN_BLOCKED &&
                  sbs::SBS_FULL == SB_BATCH_SPAWN_FULL,
              "the row codes");
static_assert(sbs::SBS_DRY_RUN == SB_BATCH_SPAWN_DRY_RUN && sbs::SBS_SKIP_TOUCHING == SB_BATCH_SPAWN_SKIP_TOUCHING, "the flags");

#define SBS_MAX_BITMAP_WORDS ((SB_BATCH_MAX_PARTICLES + 31u) / 32u) // the capacity of a scene is at most SB_BATCH_MAX_PARTICLES

__global__ __launch_bounds__(SBS_BLOCK) void k_batch_add_particles(SbBatchView V, float radius, const uint32_t *__restrict__ rows, uint32_t k,
                                                                   uint32_t flags, int32_t *__restrict__ result, int32_t *__restrict__ counts)
{
    __shared__ uint32_t s_row[SB_BATCH_ADD_MAX * SBS_ROW_WORDS]; // [64][8]
    __shared__ int32_t s_verd[SB_BATCH_ADD_MAX];                 // [64] steps 1 and 2
    __shared__ uint32_t s_hit[2];                                // bit j: row j touches a particle slot < P ("E(j)")
    __shared__ uint32_t s_free[SBS_MAX_BITMAP_WORDS];            // bit d: particle data index d is free
    __shared__ uint32_t s_pref[SBS_MAX_BITMAP_WORDS + 1u];       // free indices in front of each word
    const uint32_t scene = blockIdx.x, tid = threadIdx.x;
    if (scene >= V.n_scenes) return;
    const uint32_t maxP = V.maxP, npw = (maxP + 31u) >> 5;

    const SbbScene hd = sbb_scene(V, scene);
    const uint32_t P = hd.P;
    unsigned char *cst = V.cst + (size_t)scene * V.cst_bytes, *st = V.st + (size_t)scene * V.st_bytes;
    uint32_t *g_pmap = (uint32_t *)(cst + V.o_pmap);
    float2 *g_part = (float2 *)(st + V.o_part);
    const bool dry = (flags & SB_BATCH_SPAWN_DRY_RUN) != 0u, skip_touching = (flags & SB_BATCH_SPAWN_SKIP_TOUCHING) != 0u;

    // ---- rows, the free bitmap
    for (uint32_t i = tid; i < k * SBS_ROW_WORDS; i += SBS_BLOCK) s_row[i] = rows[(size_t)scene * k * SBS_ROW_WORDS + i];
    if (tid < 2u) s_hit[tid] = 0u;
    {
        // (the "holds a particle" bytes, four to a load: the row of them is padded to 16 bytes; bytes at and past maxP are no indices)
        const uint32_t *pex4 = (const uint32_t *)(cst + V.o_pex);
        for (uint32_t w = tid; w < npw; w += SBS_BLOCK) {
            uint32_t bits = 0u;
            for (uint32_t q = 0; q < 8u; q++) {
                const uint32_t d0 = 32u * w + 4u * q;
                if (d0 >= maxP) break;
                const uint32_t held = pex4[d0 >> 2];
                for (uint32_t e = 0; e < 4u; e++)
                    if (d0 + e < maxP && ((held >> (8u * e)) & 0xffu) == 0u) bits |= 1u << (4u * q + e);
            }
            s_free[w] = hd.loaded ? bits : 0u;
        }
    }
    __syncthreads();
    if (tid <= npw) { // the prefix, a lane per entry (at most 33): the free indices in words 0 .. tid - 1; entry npw is the total
        uint32_t run = 0u;
        for (uint32_t w = 0; w < tid; w++) run += __popc(s_free[w]);
        s_pref[tid] = run;
    }
    // ---- the verdict of each row, a lane per row
    if (tid < k) s_verd[tid] = sbs::row_verdict(s_row + tid * SBS_ROW_WORDS, hd.loaded != 0u);
    __syncthreads();

    // ---- touching a particle of the scene: every slot's current position against the candidate rows
    float two_r;
    const float thr = sbs::touch_threshold(radius, &two_r);
    if (skip_touching) {
        for (uint32_t s = tid; s < P; s += SBS_BLOCK) {
            const uint32_t d = g_pmap[s];
            if (d >= maxP) continue; // (an upload is refused unless its particle data indices are inside the capacity)
            const float2 other = g_part[3u * d];
            for (uint32_t q = 0; q < k; q++) {
                const float2 me = make_float2(__uint_as_float(s_row[q * SBS_ROW_WORDS + 1u]), __uint_as_float(s_row[q * SBS_ROW_WORDS + 2u]));
                if (s_verd[q] == sbs::SBS_CANDIDATE && sb_touch(me, other, thr, two_r)) atomicOr(&s_hit[q >> 5], 1u << (q & 31u));
            }
        }
        __syncthreads();
    }
    if (tid >= 64u) return; // wave 0 finishes (k <= 64: a lane per row)

    // ---- rows against earlier rows, room, the r-th free index
    const bool row = tid < k;
    const uint32_t *w = s_row + (row ? tid : 0u) * SBS_ROW_WORDS;
    int32_t verd = row ? s_verd[tid] : (int32_t)sbs::SBS_EMPTY;
    if (skip_touching && verd == sbs::SBS_CANDIDATE) {
        const float2 me = make_float2(__uint_as_float(w[1]), __uint_as_float(w[2]));
        const bool blocked = sbs::blocked(
            tid, ((s_hit[tid >> 5] >> (tid & 31u)) & 1u) != 0u, [&](uint32_t i) { return s_verd[i]; },
            [&](uint32_t i) { return ((s_hit[i >> 5] >> (i & 31u)) & 1u) != 0u; },
            [&](uint32_t i) {
                return sb_touch(me, make_float2(__uint_as_float(s_row[i * SBS_ROW_WORDS + 1u]), __uint_as_float(s_row[i * SBS_ROW_WORDS + 2u])), thr, two_r);
            });
        if (blocked) verd = sbs::SBS_BLOCKED;
    }
    const unsigned long long m_cand = __ballot(verd == sbs::SBS_CANDIDATE);
    const uint32_t r = (uint32_t)__popcll(m_cand & ((1ull << tid) - 1ull)), n_free = s_pref[npw];
    uint32_t d = 0u;
    if (verd == sbs::SBS_CANDIDATE) {
        if (P + r < maxP && r < n_free) {
            uint32_t lo = 0u, hi = npw; // the word with s_pref[lo] <= r < s_pref[lo + 1]
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_pref[mid] <= r) lo = mid;
                else hi = mid;
            }
            uint32_t bits = s_free[lo];
            for (uint32_t t = r - s_pref[lo]; t != 0u; t--) bits &= bits - 1u;
            d = 32u * lo + (uint32_t)__builtin_ctz(bits);
        } else {
            verd = sbs::SBS_FULL;
        }
    }
    const bool add = verd == sbs::SBS_CANDIDATE;
    const unsigned long long m_add = __ballot(add), m_inv = __ballot(verd == sbs::SBS_INVALID), m_blk = __ballot(verd == sbs::SBS_BLOCKED),
                             m_full = __ballot(verd == sbs::SBS_FULL);
    const uint32_t n_add = (uint32_t)__popcll(m_add);

    if (!dry && n_add != 0u) {
        if (add) { // (d < maxP and P + r < maxP: the room test above)
            g_pmap[P + r] = d;
            (cst + V.o_pex)[d] = 1;
            g_part[3u * d] = make_float2(__uint_as_float(w[1]), __uint_as_float(w[2]));
            g_part[3u * d + 1u] = make_float2(__uint_as_float(w[3]), __uint_as_float(w[4]));
            g_part[3u * d + 2u] = make_float2(__uint_as_float(w[5]), __uint_as_float(w[6]));
        }
        // (the count: written at agent scope, as every kernel of the batch reads it)
        if (tid == 0u) SB_AGENT_STORE(&V.meta[(size_t)scene * SB_BM_WORDS + SB_BM_P], P + n_add);
    }
    if (result && row) result[(size_t)scene * k + tid] = add ? (int32_t)d : verd;
    if (counts && tid == 0u) {
        int32_t *c = counts + (size_t)scene * SBS_NWORDS;
        c[SBS_ADDED] = (int32_t)n_add;
        c[SBS_N_INVALID] = __popcll(m_inv);
        c[SBS_N_BLOCKED] = __popcll(m_blk);
        c[SBS_N_FULL] = __popcll(m_full);
    }
}

// ---------------------------------------------------------------- host
bool sbb_spawn_info(sb_batch *b, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "add_particles_kernel_vgprs" || k == "add_particles_kernel_scratch_bytes")
        *value = sbb_kernel_res(b, b->spawn_res, (const void *)k_batch_add_particles, k == "add_particles_kernel_vgprs");
    else return false;
    return true;
}

sb_status sb_batch_add_particles_device(sb_batch *b, uint32_t flags, const void *device_rows, uint32_t k, void *device_result_i32,
                                        void *device_counts_i32)
{
    if (!b) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_add_particles_device: null batch");
    if (flags & ~(SB_BATCH_SPAWN_DRY_RUN | SB_BATCH_SPAWN_SKIP_TOUCHING))
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_add_particles_device: flags 0x%x: only SB_BATCH_SPAWN_DRY_RUN and _SKIP_TOUCHING are known", flags);
    if (k > SB_BATCH_ADD_MAX) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_add_particles_device: %u rows per scene, at most %u", k, SB_BATCH_ADD_MAX);
    if (k && !device_rows) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_add_particles_device: null rows");
    if (sbb_misaligned4({device_rows, device_result_i32, device_counts_i32}))
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_add_particles_device: rows, result and counts must be 4-byte aligned");
    SB_HIP(b, hipSetDevice(b->device));
    k_batch_add_particles<<<b->opt.n_scenes, SBS_BLOCK, 0, b->stream>>>(b->V, b->prm.particle_radius, (const uint32_t *)device_rows, k, flags,
                                                                        (int32_t *)device_result_i32, (int32_t *)device_counts_i32);
    return check_launch(b, "sb_batch_add_particles_device");
}
