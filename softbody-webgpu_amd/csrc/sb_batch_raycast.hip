// sb_batch_raycast.hip -- range sensors: every scene of a batch casts its own k rays in ONE launch and gets, per ray, the nearest
// hit among its particles (discs), its live beams (segments) and the four walls (sb_batch_raycast_device of include/softbody.h;
// gfx950, wave64).  The arithmetic of a meeting and the key of the winner are sb_batch_ray_math.h's.
//
// One workgroup of 256 per scene.
//   stage    into LDS: the positions, data indices and (with labels) labels of the particle SLOTS; the live beam slots as ONE word
//            each -- slot of endpoint A, slot of endpoint B, beam data index: 10 + 10 + 12 bits --; the k rows; k keys of SBR_NO_KEY
//   walk     thread tid owns ray tid % kk (kk: k rounded up to a power of two) and part tid / kk of the 256 / kk interleaved parts
//            of both primitive lists.  It keeps its smallest key in registers.  The lanes of a wave that share a part read the same
//            primitive (an LDS broadcast), those of different parts neighbouring words (different banks).  No atomic, no
//            cross-lane step, no barrier inside the loops; the division and the root sit behind the sign tests.  Part 0 also
//            meets the walls.
//   combine  one LDS atomicMin of the 64-bit key per thread that found something; with k > 128 there is one part and a plain store
//   answer   one lane per ray decodes the key and stores t and the hit row (the label is read from the caller's row at the hit's
//            data index, which is inside the row); wave 0 counts the row codes by ballots
// Nothing of the batch is written; every store goes to the workgroup's own rows.  The key is an integer minimum: the outputs are
// the same bits whatever the schedule.
#include <string>

#include "sb_batch.h"
#include "sb_batch_ray_math.h"

#define SBRC_BLOCK 256u
#define SBRC_SLOT_BITS 10u
#define SBRC_SLOT_MASK ((1u << SBRC_SLOT_BITS) - 1u)

static_assert(SB_BATCH_MAX_PARTICLES <= (1u << SBRC_SLOT_BITS) && SB_BATCH_MAX_BEAMS <= (1u << (32u - 2u * SBRC_SLOT_BITS)),
              "two particle slots and a beam data index share one staged word");
static_assert(SB_BATCH_MAX_PARTICLES <= 0x10000 && SB_BATCH_MAX_BEAMS <= 0x10000, "the index field of a key is 16 bits");
static_assert(SB_BATCH_RAY_MAX == SBRC_BLOCK, "a thread per ray at the widest call");
static_assert(SB_BATCH_RAY_HIT_WORDS == SBR_HIT_WORDS && sizeof(sb_batch_ray) == SBR_ROW_WORDS * 4u, "the row and the hit row of the header");
static_assert(SB_RAY_PARTICLES == sbr::MASK_PARTICLES && SB_RAY_BEAMS == sbr::MASK_BEAMS && SB_RAY_WALLS == sbr::MASK_WALLS, "the mask bits");
static_assert(SB_BATCH_WALL_LEFT == sbr::WALL_LEFT && SB_BATCH_WALL_RIGHT == sbr::WALL_RIGHT && SB_BATCH_WALL_LOW == sbr::WALL_LOW &&
                  SB_BATCH_WALL_HIGH == sbr::WALL_HIGH, "the wall words");

// LDS of a workgroup: key[SB_BATCH_RAY_MAX] (8 bytes each, first: aligned), pos[maxP] (2 words each), pidx[maxP], label[maxP],
// beam[maxB], rows[SB_BATCH_RAY_MAX][8]
static inline uint32_t sbrc_lds_bytes(uint32_t maxP, uint32_t maxB) { return (2u * SB_BATCH_RAY_MAX + 4u * maxP + maxB + SBR_ROW_WORDS * SB_BATCH_RAY_MAX) * 4u; }

__global__ __launch_bounds__(SBRC_BLOCK) void k_batch_raycast(SbBatchView V, SbParams prm, const uint32_t *__restrict__ rays, uint32_t k,
                                                              const int32_t *__restrict__ labels, uint32_t *__restrict__ out_t,
                                                              int32_t *__restrict__ out_hit, int32_t *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sbrc_lds[];
    const uint32_t scene = blockIdx.x, tid = threadIdx.x;
    if (scene >= V.n_scenes) return;
    const uint32_t maxP = V.maxP, maxB = V.maxB;
    unsigned long long *s_key = (unsigned long long *)sbrc_lds; // [SB_BATCH_RAY_MAX] per ray: the smallest key; then its row's kind
    float2 *s_pos = (float2 *)(sbrc_lds + 2u * SB_BATCH_RAY_MAX); // [maxP] per particle SLOT: position
    uint32_t *s_pidx = (uint32_t *)(s_pos + maxP);                // [maxP] per SLOT: data index
    int32_t *s_lab = (int32_t *)(s_pidx + maxP);                  // [maxP] per SLOT: the caller's label (-1 without labels)
    uint32_t *s_beam = (uint32_t *)(s_lab + maxP);                // [maxB] per live beam SLOT: slot A | slot B << 10 | data index << 20
    uint32_t *s_row = s_beam + maxB;                              // [k][8] the rows

    const SbbScene hd = sbb_scene(V, scene);
    const uint32_t P = hd.P, Bc = P ? hd.Bc : 0u; // (a beam needs two particles: an upload is refused unless its endpoints are slots < P)
    const uint32_t *g_pmap = (const uint32_t *)(hd.cst + V.o_pmap), *g_bword = (const uint32_t *)(hd.cst + V.o_bword);
    const uint32_t *g_bmap = (const uint32_t *)(hd.st + V.o_bmap);
    const float2 *g_part = (const float2 *)(hd.st + V.o_part);
    const int32_t *lrow = labels ? labels + (size_t)scene * maxP : nullptr;
    const uint32_t *rrow = rays + (size_t)scene * k * SBR_ROW_WORDS;

    // ---- stage (data indices outside the capacity cannot be uploaded; were one met, its particle is nowhere and its beam degenerate)
    for (uint32_t s = tid; s < P; s += SBRC_BLOCK) {
        const uint32_t d = g_pmap[s];
        const bool in = d < maxP;
        s_pos[s] = in ? g_part[3u * d] : make_float2(__uint_as_float(SBB_QNAN), __uint_as_float(SBB_QNAN));
        s_pidx[s] = d;
        s_lab[s] = (lrow && in) ? lrow[d] : -1;
    }
    for (uint32_t j = tid; j < Bc; j += SBRC_BLOCK) {
        const uint32_t d = g_bmap[j];
        uint32_t word = 0u; // (slots 0 and 0: a degenerate segment, which nothing meets)
        if (d < maxB) {
            const uint32_t w = g_bword[d], a = w & 0xffffu, b = w >> 16;
            if (a < P && b < P) word = a | (b << SBRC_SLOT_BITS) | (d << (2u * SBRC_SLOT_BITS));
        }
        s_beam[j] = word;
    }
    for (uint32_t i = tid; i < k * SBR_ROW_WORDS; i += SBRC_BLOCK) s_row[i] = rrow[i];
    s_key[tid] = SBR_NO_KEY;
    __syncthreads();

    // ---- walk: my ray, my part
    uint32_t kk = 1u;
    while (kk < k) kk <<= 1; // (uniform; k <= 256)
    const uint32_t ray = tid & (kk - 1u), part = tid / kk, nparts = SBRC_BLOCK / kk;
    int verdict = sbr::EMPTY;
    uint64_t key = SBR_NO_KEY;
    if (ray < k) {
        const uint32_t *w = s_row + ray * SBR_ROW_WORDS;
        verdict = sbr::row_verdict(w, lrow != nullptr);
        if (verdict == sbr::MISS) {
            const sbr::Ray r = sbr::ray_of(w);
            const float r2 = prm.particle_radius * prm.particle_radius;
            if (r.mask & sbr::MASK_PARTICLES)
                for (uint32_t s = part; s < P; s += nparts) {
                    if (sbr::skipped(r, s_lab[s])) continue;
                    const float2 c = s_pos[s];
                    key = sbr::nearer(key, sbr::disc(r, c.x, c.y, r2, s_pidx[s]));
                }
            if (r.mask & sbr::MASK_BEAMS)
                for (uint32_t j = part; j < Bc; j += nparts) {
                    const uint32_t word = s_beam[j], a = word & SBRC_SLOT_MASK, b = (word >> SBRC_SLOT_BITS) & SBRC_SLOT_MASK;
                    if (sbr::skipped(r, s_lab[a])) continue;
                    const float2 pa = s_pos[a], pb = s_pos[b];
                    key = sbr::nearer(key, sbr::segment(r, pa.x, pa.y, pb.x, pb.y, word >> (2u * SBRC_SLOT_BITS)));
                }
            if ((r.mask & sbr::MASK_WALLS) && part == 0u) key = sbr::nearer(key, sbr::walls(r, prm.bounds_size));
        }
    }
    // ---- combine the parts of a ray
    if (nparts > 1u) {
        if (key != SBR_NO_KEY) atomicMin(&s_key[ray], (unsigned long long)key);
    } else {
        s_key[ray] = key;
    }
    __syncthreads();

    // ---- answer: a lane per ray (part 0 holds the row's verdict)
    int32_t kind = sbr::EMPTY;
    if (tid < k) { // (tid < k <= kk: ray == tid, part == 0)
        key = s_key[tid];
        kind = sbr::out_kind(verdict, key);
        const size_t at = (size_t)scene * k + tid;
        if (out_t) out_t[at] = sbr::out_t(verdict, key, s_row[tid * SBR_ROW_WORDS + 5u]);
        if (out_hit) {
            const int32_t index = sbr::out_index(verdict, key);
            int32_t label = -1;
            if (lrow && (kind == sbr::PARTICLE || kind == sbr::BEAM)) {
                uint32_t p = (uint32_t)index; // the particle whose label it is: the hit one, or the hit beam's endpoint A
                if (kind == sbr::BEAM) {
                    const uint32_t a = p < maxB ? g_bword[p] & 0xffffu : P;
                    p = a < P ? s_pidx[a] : maxP;
                }
                if (p < maxP) label = lrow[p];
            }
            int32_t *h = out_hit + at * SBR_HIT_WORDS;
            h[0] = kind, h[1] = index, h[2] = label;
        }
    }
    if (!counts) return; // (uniform)
    s_key[tid] = (unsigned long long)(uint32_t)kind; // (my own word: the ray's key was read by this thread alone)
    __syncthreads();
    if (tid >= 64u) return;
    uint32_t n_valid = 0u, n_part = 0u, n_beam = 0u, n_wall = 0u;
    for (uint32_t base = 0u; base < k; base += 64u) { // (uniform trip count)
        const int32_t c = base + tid < k ? (int32_t)(uint32_t)s_key[base + tid] : (int32_t)sbr::EMPTY;
        n_valid += __popcll(__ballot(c >= 0));
        n_part += __popcll(__ballot(c == sbr::PARTICLE));
        n_beam += __popcll(__ballot(c == sbr::BEAM));
        n_wall += __popcll(__ballot(c == sbr::WALL));
    }
    if (tid < SB_BATCH_RAY_COUNT_WORDS)
        counts[(size_t)scene * SB_BATCH_RAY_COUNT_WORDS + tid] = (int32_t)(tid == 0u ? n_valid : tid == 1u ? n_part : tid == 2u ? n_beam : n_wall);
}

// ---------------------------------------------------------------- host
bool sbb_raycast_info(sb_batch *b, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "ray_max") *value = SB_BATCH_RAY_MAX;
    else if (k == "ray_hit_words") *value = SB_BATCH_RAY_HIT_WORDS;
    else if (k == "ray_count_words") *value = SB_BATCH_RAY_COUNT_WORDS;
    else if (k == "raycast_lds_bytes") *value = sbrc_lds_bytes(b->V.maxP, b->V.maxB);
    else return sbb_kernel_info(b, "raycast", (const void *)k_batch_raycast, b->raycast_res, key, value);
    return true;
}

sb_status sb_batch_raycast_device(sb_batch *b, uint32_t flags, const void *device_rays, uint32_t k, const void *device_labels_i32,
                                  void *device_t_f32, void *device_hit_i32, void *device_counts_i32)
{
    if (!b) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_raycast_device: null batch");
    if (!device_t_f32 && !device_hit_i32 && !device_counts_i32)
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_raycast_device: t, hit and counts are all null: nothing to write");
    const sb_status st = sbb_edit_entry(b, "sb_batch_raycast_device", flags, 0u, "no flag is", k, SB_BATCH_RAY_MAX, "rays", device_rays,
                                        {device_rays, device_labels_i32, device_t_f32, device_hit_i32, device_counts_i32},
                                        "rays, labels, t, hit and counts");
    if (st != SB_OK) return st;
    if (k == 0u) return SB_OK; // nothing is asked
    const SbBatchView &V = b->V;
    k_batch_raycast<<<b->opt.n_scenes, SBRC_BLOCK, sbrc_lds_bytes(V.maxP, V.maxB), b->stream>>>(
        V, b->prm, (const uint32_t *)device_rays, k, (const int32_t *)device_labels_i32, (uint32_t *)device_t_f32, (int32_t *)device_hit_i32,
        (int32_t *)device_counts_i32);
    return check_launch(b, "sb_batch_raycast_device");
}
