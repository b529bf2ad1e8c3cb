// sb_batch_raycast.hip -- range sensors: every scene of a batch casts its own k rays in ONE launch and gets, per ray, the nearest
// hit among its particles (discs), its live beams (segments) and the four walls (sb_batch_raycast_device of include/softbody.h;
// gfx950, wave64).  The arithmetic of a meeting and the key of the winner are sb_batch_ray_math.h's, the plan --
// stage, walk, combine, answer -- is sb_batch_query.h's.  This file holds what only a ray cast has: the two loops of the walk, with
// the division and the root behind the sign tests, and the t word of a row.
#include "sb_batch_query.h"
#include "sb_batch_ray_math.h"

static_assert(SB_BATCH_RAY_MAX == SBQ_BLOCK, "a thread per ray at the widest call");
static_assert(SB_BATCH_RAY_HIT_WORDS == SBR_HIT_WORDS && SB_BATCH_RAY_COUNT_WORDS == SBQ_COUNT_WORDS && sizeof(sb_batch_ray) == SBR_ROW_WORDS * 4u,
              "the row, the hit row and the counts of the header");
static_assert(SB_RAY_PARTICLES == sbr::MASK_PARTICLES && SB_RAY_BEAMS == sbr::MASK_BEAMS && SB_RAY_WALLS == sbr::MASK_WALLS, "the mask bits");

__global__ __launch_bounds__(SBQ_BLOCK) void k_batch_raycast(SbBatchView V, SbParams prm, const uint32_t *__restrict__ rays, uint32_t k,
                                                             const int32_t *__restrict__ labels, uint32_t *__restrict__ out_t,
                                                             int32_t *__restrict__ out_hit, int32_t *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sbrc_lds[];
    const uint32_t scene = blockIdx.x, tid = threadIdx.x;
    if (scene >= V.n_scenes) return;
    const SbqLds s = sbq_carve(sbrc_lds, V.maxP, V.maxB, 0u);
    const SbqScene sc = sbq_stage(V, scene, s, rays, k, labels);

    // ---- walk: my ray, my part
    const SbqSplit my = sbq_split(k);
    int verdict = sbr::EMPTY;
    uint64_t key = SBR_NO_KEY;
    if (my.row < k) {
        const uint32_t *w = s.row + my.row * SBR_ROW_WORDS;
        verdict = sbr::row_verdict(w, sc.lrow != nullptr);
        if (verdict == sbr::MISS) {
            const sbr::Ray r = sbr::ray_of(w);
            const float r2 = prm.particle_radius * prm.particle_radius;
            if (r.mask & sbr::MASK_PARTICLES)
                for (uint32_t p = my.part; p < sc.P; p += my.nparts) {
                    if (sbr::skipped(r, s.lab[p])) continue;
                    const float2 c = s.pos[p];
                    key = sbr::nearer(key, sbr::disc(r, c.x, c.y, r2, s.pidx[p]));
                }
            if (r.mask & sbr::MASK_BEAMS)
                for (uint32_t j = my.part; j < sc.nb; j += my.nparts) {
                    const uint32_t word = s.beam[j], a = sbq_beam_a(word);
                    if (sbr::skipped(r, s.lab[a])) continue;
                    const float2 pa = s.pos[a], pb = s.pos[sbq_beam_b(word)];
                    key = sbr::nearer(key, sbr::segment(r, pa.x, pa.y, pb.x, pb.y, sbq_beam_index(word)));
                }
            if ((r.mask & sbr::MASK_WALLS) && my.part == 0u) key = sbr::nearer(key, sbr::walls(r, prm.bounds_size));
        }
    }
    sbq_combine(s, my, key);
    __syncthreads();

    // ---- answer: a lane per ray (part 0 holds the row's verdict)
    int32_t kind = sbr::EMPTY;
    if (tid < k) { // (tid < k <= kk: my.row == tid, my.part == 0)
        key = s.key[tid];
        kind = sbr::out_kind(verdict, key);
        const int32_t index = sbr::out_index(verdict, key);
        const size_t at = (size_t)scene * k + tid;
        if (out_t) out_t[at] = sbr::out_t(verdict, key, s.row[tid * SBR_ROW_WORDS + 5u]);
        if (out_hit) sbq_store_hit(V, sc, s, out_hit, at, kind, index, sbq_hit_beam(V, sc, kind, index).x);
    }
    sbq_store_counts(s, counts, scene, k, kind);
}

// ---------------------------------------------------------------- host
bool sbb_raycast_info(sb_batch *b, const char *key, uint64_t *value)
{
    return sbq_info(b, "ray", "raycast", sbq_lds_bytes(b->V.maxP, b->V.maxB, 0u), (const void *)k_batch_raycast, b->raycast_res, key, value);
}

sb_status sb_batch_raycast_device(sb_batch *b, uint32_t flags, const void *device_rays, uint32_t k, const void *device_labels_i32,
                                  void *device_t_f32, void *device_hit_i32, void *device_counts_i32)
{
    bool launch;
    const sb_status st = sbq_entry(b, "sb_batch_raycast_device", flags, k, "rays", "t, hit and counts",
                                   {device_rays, device_labels_i32, device_t_f32, device_hit_i32, device_counts_i32}, &launch);
    if (!launch) return st; // (an error, or nothing is asked)
    const SbBatchView &V = b->V;
    k_batch_raycast<<<b->opt.n_scenes, SBQ_BLOCK, sbq_lds_bytes(V.maxP, V.maxB, 0u), b->stream>>>(
        V, b->prm, (const uint32_t *)device_rays, k, (const int32_t *)device_labels_i32, (uint32_t *)device_t_f32, (int32_t *)device_hit_i32,
        (int32_t *)device_counts_i32);
    return check_launch(b, "sb_batch_raycast_device");
}
