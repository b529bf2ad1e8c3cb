// sb_batch_nearest.hip -- proximity queries: every scene of a batch asks about its own k points in ONE launch and gets, per point,
// the nearest among its particles (centres), its live beams (segments) and the four walls, the closest point on it, and how many
// particles and beams lie within reach (sb_batch_nearest_device of include/softbody.h; gfx950, wave64).  The
// arithmetic of a distance and the key of the winner are sb_batch_near_math.h's, the plan -- stage, walk, combine, answer -- is
// sb_batch_query.h's.  This file holds what only a proximity query has: the two loops of the walk, with the division behind the two
// sign tests; the two `within` counts of a row, kept in registers over the walk and combined by at most two LDS atomicAdds per
// thread (plain stores where there is one part); and in the answer the distance -- the one root of a row -- and the closest point,
// recomputed from the winner.
#include "sb_batch_query.h"
#include "sb_batch_near_math.h"

#define SBNR_WITHIN_WORDS 2u // per point, in LDS: particles, beams within reach

static_assert(SB_BATCH_NEAR_MAX == SBQ_BLOCK, "a thread per point at the widest call");
static_assert(SB_BATCH_NEAR_HIT_WORDS == SBN_HIT_WORDS && SB_BATCH_NEAR_COUNT_WORDS == SBQ_COUNT_WORDS && sizeof(sb_batch_near_point) == SBN_ROW_WORDS * 4u,
              "the row, the hit row and the counts of the header");
static_assert(SB_NEAR_PARTICLES == sbn::MASK_PARTICLES && SB_NEAR_BEAMS == sbn::MASK_BEAMS && SB_NEAR_WALLS == sbn::MASK_WALLS, "the mask bits");
static_assert(SB_BATCH_NEAR_MISS == sbn::MISS && SB_BATCH_NEAR_PARTICLE == sbn::PARTICLE && SB_BATCH_NEAR_BEAM == sbn::BEAM &&
                  SB_BATCH_NEAR_WALL == sbn::WALL && SB_BATCH_NEAR_EMPTY == sbn::EMPTY && SB_BATCH_NEAR_INVALID == sbn::INVALID, "the kind words");

__global__ __launch_bounds__(SBQ_BLOCK) void k_batch_nearest(SbBatchView V, SbParams prm, const uint32_t *__restrict__ points, uint32_t k,
                                                             const int32_t *__restrict__ labels, uint32_t *__restrict__ out_d,
                                                             int32_t *__restrict__ out_hit, uint32_t *__restrict__ out_point,
                                                             int32_t *__restrict__ out_within, int32_t *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sbnr_lds[];
    const uint32_t scene = blockIdx.x, tid = threadIdx.x;
    if (scene >= V.n_scenes) return;
    const SbqLds s = sbq_carve(sbnr_lds, V.maxP, V.maxB, SBNR_WITHIN_WORDS);
    uint32_t *s_within = s.extra; // [256][2]
    const SbqScene sc = sbq_stage(V, scene, s, points, k, labels);

    // ---- walk: my point, my part
    const SbqSplit my = sbq_split(k);
    int verdict = sbn::EMPTY;
    uint64_t key = SBN_NO_KEY;
    uint32_t in_p = 0u, in_b = 0u;
    if (my.row < k) {
        const uint32_t *w = s.row + my.row * SBN_ROW_WORDS;
        verdict = sbn::row_verdict(w, sc.lrow != nullptr);
        if (verdict == sbn::MISS) {
            const sbn::Probe q = sbn::probe_of(w);
            if (q.mask & sbn::MASK_PARTICLES)
                for (uint32_t p = my.part; p < sc.P; p += my.nparts) {
                    if (sbn::skipped(q, s.lab[p])) continue;
                    const float2 c = s.pos[p];
                    const uint64_t cand = sbn::particle(q, c.x, c.y, s.pidx[p]);
                    in_p += cand != SBN_NO_KEY;
                    key = sbn::nearer(key, cand);
                }
            if (q.mask & sbn::MASK_BEAMS)
                for (uint32_t j = my.part; j < sc.nb; j += my.nparts) {
                    const uint32_t word = s.beam[j], a = sbq_beam_a(word);
                    if (sbn::skipped(q, s.lab[a])) continue;
                    const float2 pa = s.pos[a], pb = s.pos[sbq_beam_b(word)];
                    const uint64_t cand = sbn::segment(q, pa.x, pa.y, pb.x, pb.y, sbq_beam_index(word));
                    in_b += cand != SBN_NO_KEY;
                    key = sbn::nearer(key, cand);
                }
            if ((q.mask & sbn::MASK_WALLS) && my.part == 0u) key = sbn::nearer(key, sbn::walls(q, prm.bounds_size));
        }
    }
    // ---- combine the parts of a point (a padding lane holds nothing and stores nothing, or its own zeros)
    sbq_combine(s, my, key);
    if (my.nparts > 1u) {
        if (in_p) atomicAdd(&s_within[2u * my.row], in_p);
        if (in_b) atomicAdd(&s_within[2u * my.row + 1u], in_b);
    } else {
        s_within[2u * my.row] = in_p, s_within[2u * my.row + 1u] = in_b;
    }
    __syncthreads();

    // ---- answer: a lane per point (part 0 holds the row's verdict)
    int32_t kind = sbn::EMPTY;
    if (tid < k) { // (tid < k <= kk: my.row == tid, my.part == 0)
        key = s.key[tid];
        kind = sbn::out_kind(verdict, key);
        const int32_t index = sbn::out_index(verdict, key);
        const uint32_t *w = s.row + tid * SBN_ROW_WORDS;
        const size_t at = (size_t)scene * k + tid;
        if (out_d) out_d[at] = sbn::out_d(verdict, key, w[3]);
        const uint2 ends = sbq_hit_beam(V, sc, kind, index);
        if (out_hit) sbq_store_hit(V, sc, s, out_hit, at, kind, index, ends.x);
        if (out_point) {
            float qx = 0.0f, qy = 0.0f; // (an empty or invalid row)
            if (verdict == sbn::MISS) {
                const sbn::Probe q = sbn::probe_of(w);
                qx = q.px, qy = q.py; // (a miss: the query point's bits)
                if (kind == sbn::PARTICLE && (uint32_t)index < V.maxP) {
                    const float2 c = sc.g_part[3u * (uint32_t)index];
                    qx = c.x, qy = c.y;
                } else if (kind == sbn::BEAM && ends.x < sc.P && ends.y < sc.P) {
                    const float2 pa = s.pos[ends.x], pb = s.pos[ends.y];
                    sbn::segment_q(q, pa.x, pa.y, pb.x, pb.y, &qx, &qy);
                } else if (kind == sbn::WALL) {
                    sbn::wall_q(q, prm.bounds_size, (uint32_t)index, &qx, &qy);
                }
            }
            out_point[2u * at] = __float_as_uint(qx), out_point[2u * at + 1u] = __float_as_uint(qy);
        }
        if (out_within) out_within[2u * at] = (int32_t)s_within[2u * tid], out_within[2u * at + 1u] = (int32_t)s_within[2u * tid + 1u];
    }
    sbq_store_counts(s, counts, scene, k, kind);
}

// ---------------------------------------------------------------- host
bool sbb_nearest_info(sb_batch *b, const char *key, uint64_t *value)
{
    return sbq_info(b, "near", "nearest", sbq_lds_bytes(b->V.maxP, b->V.maxB, SBNR_WITHIN_WORDS), (const void *)k_batch_nearest, b->nearest_res, key, value);
}

sb_status sb_batch_nearest_device(sb_batch *b, uint32_t flags, const void *device_points, uint32_t k, const void *device_labels_i32,
                                  void *device_d_f32, void *device_hit_i32, void *device_point_f32, void *device_within_i32,
                                  void *device_counts_i32)
{
    bool launch;
    const sb_status st = sbq_entry(b, "sb_batch_nearest_device", flags, k, "points", "d, hit, point, within and counts",
                                   {device_points, device_labels_i32, device_d_f32, device_hit_i32, device_point_f32, device_within_i32,
                                    device_counts_i32}, &launch);
    if (!launch) return st; // (an error, or nothing is asked)
    const SbBatchView &V = b->V;
    k_batch_nearest<<<b->opt.n_scenes, SBQ_BLOCK, sbq_lds_bytes(V.maxP, V.maxB, SBNR_WITHIN_WORDS), b->stream>>>(
        V, b->prm, (const uint32_t *)device_points, k, (const int32_t *)device_labels_i32, (uint32_t *)device_d_f32, (int32_t *)device_hit_i32,
        (uint32_t *)device_point_f32, (int32_t *)device_within_i32, (int32_t *)device_counts_i32);
    return check_launch(b, "sb_batch_nearest_device");
}
