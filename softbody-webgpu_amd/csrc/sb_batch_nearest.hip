// sb_batch_nearest.hip -- proximity queries: every scene of a batch asks about its own k points in ONE launch and gets, per point,
// the nearest among its particles (centres), its live beams (segments) and the four walls, the closest point on it, and how many
// particles and beams lie within reach (sb_batch_nearest_device of include/softbody.h; gfx950, wave64).  The
// arithmetic of a distance and the key of the winner are sb_batch_near_math.h's.  The plan is sb_batch_raycast.hip's.
//
// One workgroup of 256 per scene.
//   stage    into LDS: the positions, data indices and (with labels) labels of the particle SLOTS; the live beams as ONE word each
//            -- slot of endpoint A, slot of endpoint B, beam data index: 10 + 10 + 12 bits --; the k rows; k keys of SBN_NO_KEY; 2k
//            `within` words of zero.  A beam entry that names nothing (none can be uploaded) is left out: the list is compacted wave
//            by wave, so its order depends on the schedule -- which no output does: minima and counts of integers.
//   walk     thread tid owns point tid % kk (kk: k rounded up to a power of two) and part tid / kk of the 256 / kk interleaved parts
//            of both lists.  It keeps its smallest key and its two counts in registers.  The lanes of a wave that share a part read
//            the same primitive (an LDS broadcast), those of different parts neighbouring words (different banks).  No atomic, no
//            cross-lane step, no barrier inside the loops; the division sits behind the two sign tests.  Part 0 also asks the walls.
//   combine  one LDS atomicMin of the 64-bit key and at most two LDS atomicAdds per thread; with k > 128 there is one part and plain
//            stores
//   answer   one lane per point decodes the key, recomputes the closest point from the winner, takes the root and stores (the label
//            is read from the caller's row at the hit's data index, which is inside the row); wave 0 counts the row codes by ballots
// Nothing of the batch is written; every store goes to the workgroup's own rows.
#include <string>

#include "sb_batch.h"
#include "sb_batch_near_math.h"

#define SBNR_BLOCK 256u
#define SBNR_SLOT_BITS 10u
#define SBNR_SLOT_MASK ((1u << SBNR_SLOT_BITS) - 1u)
#define SBNR_TAIL_WORDS 4u // the length of the compacted beam list, padded to 16 bytes

static_assert(SB_BATCH_MAX_PARTICLES <= (1u << SBNR_SLOT_BITS) && SB_BATCH_MAX_BEAMS <= (1u << (32u - 2u * SBNR_SLOT_BITS)),
              "two particle slots and a beam data index share one staged word");
static_assert(SB_BATCH_MAX_PARTICLES <= 0x10000 && SB_BATCH_MAX_BEAMS <= 0x10000, "the index field of a key is 16 bits");
static_assert(SB_BATCH_NEAR_MAX == SBNR_BLOCK, "a thread per point at the widest call");
static_assert(SB_BATCH_NEAR_HIT_WORDS == SBN_HIT_WORDS && sizeof(sb_batch_near_point) == SBN_ROW_WORDS * 4u, "the row and the hit row of the header");
static_assert(SB_NEAR_PARTICLES == sbn::MASK_PARTICLES && SB_NEAR_BEAMS == sbn::MASK_BEAMS && SB_NEAR_WALLS == sbn::MASK_WALLS, "the mask bits");
static_assert(SB_BATCH_WALL_LEFT == sbn::WALL_LEFT && SB_BATCH_WALL_RIGHT == sbn::WALL_RIGHT && SB_BATCH_WALL_LOW == sbn::WALL_LOW &&
                  SB_BATCH_WALL_HIGH == sbn::WALL_HIGH, "the wall words");
static_assert(SB_BATCH_NEAR_MISS == sbn::MISS && SB_BATCH_NEAR_PARTICLE == sbn::PARTICLE && SB_BATCH_NEAR_BEAM == sbn::BEAM &&
                  SB_BATCH_NEAR_WALL == sbn::WALL && SB_BATCH_NEAR_EMPTY == sbn::EMPTY && SB_BATCH_NEAR_INVALID == sbn::INVALID, "the kind words");

// LDS of a workgroup: key[SB_BATCH_NEAR_MAX] (8 bytes each, first: aligned), pos[maxP] (2 words each), pidx[maxP], label[maxP],
// beam[maxB], rows[SB_BATCH_NEAR_MAX][8], within[SB_BATCH_NEAR_MAX][2], the tail
static inline uint32_t sbnr_lds_bytes(uint32_t maxP, uint32_t maxB)
{
    return (2u * SB_BATCH_NEAR_MAX + 4u * maxP + maxB + SBN_ROW_WORDS * SB_BATCH_NEAR_MAX + 2u * SB_BATCH_NEAR_MAX + SBNR_TAIL_WORDS) * 4u;
}

__global__ __launch_bounds__(SBNR_BLOCK) void k_batch_nearest(SbBatchView V, SbParams prm, const uint32_t *__restrict__ points, uint32_t k,
                                                              const int32_t *__restrict__ labels, uint32_t *__restrict__ out_d,
                                                              int32_t *__restrict__ out_hit, uint32_t *__restrict__ out_point,
                                                              int32_t *__restrict__ out_within, int32_t *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sbnr_lds[];
    const uint32_t scene = blockIdx.x, tid = threadIdx.x;
    if (scene >= V.n_scenes) return;
    const uint32_t maxP = V.maxP, maxB = V.maxB;
    unsigned long long *s_key = (unsigned long long *)sbnr_lds; // [SB_BATCH_NEAR_MAX] per point: the smallest key; then its row's kind
    float2 *s_pos = (float2 *)(sbnr_lds + 2u * SB_BATCH_NEAR_MAX); // [maxP] per particle SLOT: position
    uint32_t *s_pidx = (uint32_t *)(s_pos + maxP);                 // [maxP] per SLOT: data index
    int32_t *s_lab = (int32_t *)(s_pidx + maxP);                   // [maxP] per SLOT: the caller's label (-1 without labels)
    uint32_t *s_beam = (uint32_t *)(s_lab + maxP);                 // [maxB] per live beam: slot A | slot B << 10 | data index << 20
    uint32_t *s_row = s_beam + maxB;                               // [k][8] the rows
    uint32_t *s_within = s_row + SBN_ROW_WORDS * SB_BATCH_NEAR_MAX; // [SB_BATCH_NEAR_MAX][2] per point: particles, beams within reach
    uint32_t *s_nb = s_within + 2u * SB_BATCH_NEAR_MAX;            // [1] beams staged

    const SbbScene hd = sbb_scene(V, scene);
    const uint32_t P = hd.P, Bc = P ? hd.Bc : 0u; // (a beam needs two particles: an upload is refused unless its endpoints are slots < P)
    const uint32_t *g_pmap = (const uint32_t *)(hd.cst + V.o_pmap), *g_bword = (const uint32_t *)(hd.cst + V.o_bword);
    const uint32_t *g_bmap = (const uint32_t *)(hd.st + V.o_bmap);
    const float2 *g_part = (const float2 *)(hd.st + V.o_part);
    const int32_t *lrow = labels ? labels + (size_t)scene * maxP : nullptr;
    const uint32_t *rrow = points + (size_t)scene * k * SBN_ROW_WORDS;

    // ---- stage (data indices outside the capacity cannot be uploaded; were one met, its particle is nowhere and its beam left out)
    if (tid == 0u) *s_nb = 0u;
    for (uint32_t s = tid; s < P; s += SBNR_BLOCK) {
        const uint32_t d = g_pmap[s];
        const bool in = d < maxP;
        s_pos[s] = in ? g_part[3u * d] : make_float2(__uint_as_float(SBB_QNAN), __uint_as_float(SBB_QNAN));
        s_pidx[s] = d;
        s_lab[s] = (lrow && in) ? lrow[d] : -1;
    }
    for (uint32_t i = tid; i < k * SBN_ROW_WORDS; i += SBNR_BLOCK) s_row[i] = rrow[i];
    s_key[tid] = SBN_NO_KEY;
    s_within[2u * tid] = 0u, s_within[2u * tid + 1u] = 0u;
    __syncthreads();
    const uint32_t lane = tid & 63u;
    for (uint32_t j0 = 0u; j0 < Bc; j0 += SBNR_BLOCK) { // (uniform trip count: every lane reaches the ballot)
        const uint32_t j = j0 + tid;
        uint32_t word = 0u;
        bool names = false;
        if (j < Bc) {
            const uint32_t d = g_bmap[j];
            if (d < maxB) {
                const uint32_t w = g_bword[d], a = w & 0xffffu, b = w >> 16;
                names = a < P && b < P;
                word = a | (b << SBNR_SLOT_BITS) | (d << (2u * SBNR_SLOT_BITS));
            }
        }
        const unsigned long long m = __ballot(names);
        uint32_t base = 0u;
        if (lane == 0u && m) base = atomicAdd(s_nb, (uint32_t)__popcll(m)); // (at most Bc <= maxB in all: every store below is inside s_beam)
        base = sbb_uniform(base);
        if (names) s_beam[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = word;
    }
    __syncthreads();
    const uint32_t nb = *s_nb;

    // ---- walk: my point, my part
    uint32_t kk = 1u;
    while (kk < k) kk <<= 1; // (uniform; k <= 256)
    const uint32_t pt = tid & (kk - 1u), part = tid / kk, nparts = SBNR_BLOCK / kk;
    int verdict = sbn::EMPTY;
    uint64_t key = SBN_NO_KEY;
    uint32_t in_p = 0u, in_b = 0u;
    if (pt < k) {
        const uint32_t *w = s_row + pt * SBN_ROW_WORDS;
        verdict = sbn::row_verdict(w, lrow != nullptr);
        if (verdict == sbn::MISS) {
            const sbn::Probe q = sbn::probe_of(w);
            if (q.mask & sbn::MASK_PARTICLES)
                for (uint32_t s = part; s < P; s += nparts) {
                    if (sbn::skipped(q, s_lab[s])) continue;
                    const float2 c = s_pos[s];
                    const uint64_t cand = sbn::particle(q, c.x, c.y, s_pidx[s]);
                    in_p += cand != SBN_NO_KEY;
                    key = sbn::nearer(key, cand);
                }
            if (q.mask & sbn::MASK_BEAMS)
                for (uint32_t j = part; j < nb; j += nparts) {
                    const uint32_t word = s_beam[j], a = word & SBNR_SLOT_MASK, b = (word >> SBNR_SLOT_BITS) & SBNR_SLOT_MASK;
                    if (sbn::skipped(q, s_lab[a])) continue;
                    const float2 pa = s_pos[a], pb = s_pos[b];
                    const uint64_t cand = sbn::segment(q, pa.x, pa.y, pb.x, pb.y, word >> (2u * SBNR_SLOT_BITS));
                    in_b += cand != SBN_NO_KEY;
                    key = sbn::nearer(key, cand);
                }
            if ((q.mask & sbn::MASK_WALLS) && part == 0u) key = sbn::nearer(key, sbn::walls(q, prm.bounds_size));
        }
    }
    // ---- combine the parts of a point (pt < 256 always: a padding lane holds nothing and stores nothing, or its own zeros)
    if (nparts > 1u) {
        if (key != SBN_NO_KEY) atomicMin(&s_key[pt], (unsigned long long)key);
        if (in_p) atomicAdd(&s_within[2u * pt], in_p);
        if (in_b) atomicAdd(&s_within[2u * pt + 1u], in_b);
    } else {
        s_key[pt] = key;
        s_within[2u * pt] = in_p, s_within[2u * pt + 1u] = in_b;
    }
    __syncthreads();

    // ---- answer: a lane per point (part 0 holds the row's verdict)
    int32_t kind = sbn::EMPTY;
    if (tid < k) { // (tid < k <= kk: pt == tid, part == 0)
        key = s_key[tid];
        kind = sbn::out_kind(verdict, key);
        const int32_t index = sbn::out_index(verdict, key);
        const uint32_t *w = s_row + tid * SBN_ROW_WORDS;
        const size_t at = (size_t)scene * k + tid;
        if (out_d) out_d[at] = sbn::out_d(verdict, key, w[3]);
        uint32_t a_slot = P; // the hit beam's endpoints, as slots
        uint32_t b_slot = P;
        if (kind == sbn::BEAM && (uint32_t)index < maxB) {
            const uint32_t bw = g_bword[index];
            a_slot = bw & 0xffffu, b_slot = bw >> 16;
        }
        if (out_hit) {
            int32_t label = -1;
            if (lrow && (kind == sbn::PARTICLE || kind == sbn::BEAM)) {
                uint32_t p = (uint32_t)index; // the particle whose label it is: the nearest one, or the nearest beam's endpoint A
                if (kind == sbn::BEAM) p = a_slot < P ? s_pidx[a_slot] : maxP;
                if (p < maxP) label = lrow[p];
            }
            int32_t *h = out_hit + at * SBN_HIT_WORDS;
            h[0] = kind, h[1] = index, h[2] = label;
        }
        if (out_point) {
            float qx = 0.0f, qy = 0.0f; // (an empty or invalid row)
            if (verdict == sbn::MISS) {
                const sbn::Probe q = sbn::probe_of(w);
                qx = q.px, qy = q.py; // (a miss: the query point's bits)
                if (kind == sbn::PARTICLE && (uint32_t)index < maxP) {
                    const float2 c = g_part[3u * (uint32_t)index];
                    qx = c.x, qy = c.y;
                } else if (kind == sbn::BEAM && a_slot < P && b_slot < P) {
                    const float2 pa = s_pos[a_slot], pb = s_pos[b_slot];
                    sbn::segment_q(q, pa.x, pa.y, pb.x, pb.y, &qx, &qy);
                } else if (kind == sbn::WALL) {
                    sbn::wall_q(q, prm.bounds_size, (uint32_t)index, &qx, &qy);
                }
            }
            out_point[2u * at] = __float_as_uint(qx), out_point[2u * at + 1u] = __float_as_uint(qy);
        }
        if (out_within) out_within[2u * at] = (int32_t)s_within[2u * tid], out_within[2u * at + 1u] = (int32_t)s_within[2u * tid + 1u];
    }
    if (!counts) return; // (uniform)
    s_key[tid] = (unsigned long long)(uint32_t)kind; // (my own word: the point's key was read by this thread alone)
    __syncthreads();
    if (tid >= 64u) return;
    uint32_t n_valid = 0u, n_part = 0u, n_beam = 0u, n_wall = 0u;
    for (uint32_t base = 0u; base < k; base += 64u) { // (uniform trip count)
        const int32_t c = base + tid < k ? (int32_t)(uint32_t)s_key[base + tid] : (int32_t)sbn::EMPTY;
        n_valid += __popcll(__ballot(c >= 0));
        n_part += __popcll(__ballot(c == sbn::PARTICLE));
        n_beam += __popcll(__ballot(c == sbn::BEAM));
        n_wall += __popcll(__ballot(c == sbn::WALL));
    }
    if (tid < SB_BATCH_NEAR_COUNT_WORDS)
        counts[(size_t)scene * SB_BATCH_NEAR_COUNT_WORDS + tid] = (int32_t)(tid == 0u ? n_valid : tid == 1u ? n_part : tid == 2u ? n_beam : n_wall);
}

// ---------------------------------------------------------------- host
bool sbb_nearest_info(sb_batch *b, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "near_max") *value = SB_BATCH_NEAR_MAX;
    else if (k == "near_hit_words") *value = SB_BATCH_NEAR_HIT_WORDS;
    else if (k == "near_count_words") *value = SB_BATCH_NEAR_COUNT_WORDS;
    else if (k == "nearest_lds_bytes") *value = sbnr_lds_bytes(b->V.maxP, b->V.maxB);
    else return sbb_kernel_info(b, "nearest", (const void *)k_batch_nearest, b->nearest_res, key, value);
    return true;
}

sb_status sb_batch_nearest_device(sb_batch *b, uint32_t flags, const void *device_points, uint32_t k, const void *device_labels_i32,
                                  void *device_d_f32, void *device_hit_i32, void *device_point_f32, void *device_within_i32,
                                  void *device_counts_i32)
{
    if (!b) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_nearest_device: null batch");
    if (!device_d_f32 && !device_hit_i32 && !device_point_f32 && !device_within_i32 && !device_counts_i32)
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_nearest_device: d, hit, point, within and counts are all null: nothing to write");
    const sb_status st = sbb_edit_entry(b, "sb_batch_nearest_device", flags, 0u, "no flag is", k, SB_BATCH_NEAR_MAX, "points", device_points,
                                        {device_points, device_labels_i32, device_d_f32, device_hit_i32, device_point_f32, device_within_i32,
                                         device_counts_i32},
                                        "points, labels, d, hit, point, within and counts");
    if (st != SB_OK) return st;
    if (k == 0u) return SB_OK; // nothing is asked
    const SbBatchView &V = b->V;
    k_batch_nearest<<<b->opt.n_scenes, SBNR_BLOCK, sbnr_lds_bytes(V.maxP, V.maxB), b->stream>>>(
        V, b->prm, (const uint32_t *)device_points, k, (const int32_t *)device_labels_i32, (uint32_t *)device_d_f32, (int32_t *)device_hit_i32,
        (uint32_t *)device_point_f32, (int32_t *)device_within_i32, (int32_t *)device_counts_i32);
    return check_launch(b, "sb_batch_nearest_device");
}
