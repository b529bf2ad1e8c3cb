// sb_batch_graph.hip -- the beam graph of every scene of a batch in ONE launch: edge list, materials and a sorted adjacency in the
// caller's index space (sb_batch_graph_device of include/softbody.h; gfx950, wave64).
//
// One workgroup per scene.  The particle mapping (slot -> data index) is copied into LDS once: the constant blob's endpoint words
// hold SLOTS, so nothing is inverted.  A lane per live beam slot takes the slot's data index through the state blob's beam mapping
// and its pending break bit, raises the beam's bit in an LDS bitmap of the LISTED data indices and, where an adjacency is wanted,
// writes the two half-edge keys of sb_graph_math.h to words 2 j and 2 j + 1 of the key array (SBG_NO_KEY for a slot that is not
// listed).  `ends` and `material` are then written once per data index from that bitmap, zero rows included.  The keys are sorted
// by ONE bitonic network in LDS whose width depends on the number of live slots alone: a star of 4095 beams on one particle costs
// what a lattice of as many beams costs.  Sorted, position i IS row i of `nbr`; row_ptr[p] is the lower bound of particle p's
// smallest possible key; the degrees are differences of row_ptr.  A call that wants counts but no adjacency skips the sort: the
// degrees are then an LDS histogram.  Integers only; LDS atomics and plain vector stores of this
// workgroup into its own scene's rows; nothing of the batch is written.
#include <string>

#include "sb_batch.h"
#include "sb_graph_math.h"

#define SBH_BLOCK 512u
enum { SBH_NODES, SBH_BEST, SBH_LISTED, SBH_NWORDS }; // LDS words behind the arrays

static_assert(SB_BATCH_MAX_PARTICLES <= (1u << SBG_PARTICLE_BITS) && SB_BATCH_MAX_BEAMS <= (1u << SBG_BEAM_BITS), "the fields of a half-edge key");
static_assert(SB_BATCH_GRAPH_MATERIAL_WORDS < SB_BATCH_MAT_ROW, "a material row of the report is the head of the constant blob's");
// the largest-degree key: the degree above SBG_PARTICLE_BITS bits of (SBH_PMASK - data index), so that the maximum names the smallest index
#define SBH_PMASK ((1u << SBG_PARTICLE_BITS) - 1u)
static_assert(SB_BATCH_MAX_PARTICLES - 1u <= SBH_PMASK && 2u * SB_BATCH_MAX_BEAMS < (1u << (32u - SBG_PARTICLE_BITS)),
              "a degree (at most 2 * SB_BATCH_MAX_BEAMS) and a particle data index share one 32-bit key");

static __host__ __device__ inline uint32_t sbh_listed_words(uint32_t maxB) { return (maxB + 31u) >> 5; }
// LDS of a workgroup: key[smallest power of two >= 2 maxB], row_ptr[maxP + 1], pmap[maxP], listed[maxB / 32], SBH_NWORDS words
static inline uint32_t sbh_lds_bytes(uint32_t maxP, uint32_t maxB)
{
    return (sbg::sort_width(2u * maxB) + 2u * maxP + 1u + sbh_listed_words(maxB) + SBH_NWORDS) * 4u;
}

__global__ __launch_bounds__(SBH_BLOCK) void k_batch_graph(SbBatchView V, uint32_t skip_pending, int32_t *__restrict__ ends,
                                                           uint32_t *__restrict__ material, int32_t *__restrict__ row_ptr,
                                                           int32_t *__restrict__ nbr, int32_t *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sbh_lds[];
    const uint32_t scene = blockIdx.x, tid = threadIdx.x;
    if (scene >= V.n_scenes) return;
    const uint32_t maxP = V.maxP, maxB = V.maxB, nlw = sbh_listed_words(maxB);
    uint32_t *s_key = sbh_lds;                              // [sort_width(2 maxB)] half-edge keys; sorted: nbr's rows
    uint32_t *s_rp = s_key + sbg::sort_width(2u * maxB);    // [maxP + 1] row_ptr
    uint32_t *s_pmap = s_rp + maxP + 1u;                    // [maxP] particle SLOT -> data index
    uint32_t *s_listed = s_pmap + maxP;                     // [nlw] bit d: beam DATA index d is listed
    uint32_t *s_red = s_listed + nlw;                       // [SBH_NWORDS]

    const SbbScene hd = sbb_scene(V, scene);
    const uint32_t P = hd.P, Bc = hd.Bc;
    const uint32_t *g_pmap = (const uint32_t *)(hd.cst + V.o_pmap), *g_bword = (const uint32_t *)(hd.cst + V.o_bword);
    const uint32_t *g_bmat = (const uint32_t *)(hd.cst + V.o_bmat); // (verbatim bits: copied as words)
    const uint32_t *g_bmap = (const uint32_t *)(hd.st + V.o_bmap), *g_bflags = (const uint32_t *)(hd.st + V.o_bflags);
    // (uniform: kernel arguments.)  An adjacency needs the sorted keys; counts alone only the degrees, which are sums of ones: an
    // LDS histogram in row_ptr's place, filled with integer atomics whose order is nothing
    const bool adjacency = row_ptr || nbr, histogram = counts && !adjacency;
    const uint32_t n_keys = adjacency ? sbg::sort_width(2u * Bc) : 0u; // (uniform: Bc is; <= sort_width(2 maxB))

    // ---- stage: the mapping, an empty bitmap, the sort's padding
    for (uint32_t s = tid; s < P; s += SBH_BLOCK) s_pmap[s] = g_pmap[s];
    for (uint32_t w = tid; w < nlw; w += SBH_BLOCK) s_listed[w] = 0u;
    for (uint32_t i = 2u * Bc + tid; i < n_keys; i += SBH_BLOCK) s_key[i] = SBG_NO_KEY;
    if (histogram)
        for (uint32_t p = tid; p < maxP; p += SBH_BLOCK) s_rp[p] = 0u;
    if (tid < SBH_NWORDS) s_red[tid] = 0u;
    __syncthreads();

    // ---- the live beam slots (an upload is refused unless its data indices are inside the capacity and its endpoints are slots < P)
    for (uint32_t j = tid; j < Bc; j += SBH_BLOCK) {
        const uint32_t d = g_bmap[j];
        const bool pending = ((g_bflags[j >> 5] >> (j & 31u)) & 1u) != 0u;
        const bool listed = d < maxB && !(skip_pending && pending);
        uint32_t k0 = SBG_NO_KEY, k1 = SBG_NO_KEY;
        if (listed) {
            atomicOr(&s_listed[d >> 5], 1u << (d & 31u));
            if (adjacency || histogram) {
                const uint32_t w = g_bword[d], a = s_pmap[w & 0xffffu], b = s_pmap[w >> 16];
                k0 = sbg::key(a, d, 0u), k1 = sbg::key(b, d, 1u);
                if (histogram && a < maxP && b < maxP) {
                    atomicAdd(&s_rp[a], 1u), atomicAdd(&s_rp[b], 1u);
                    atomicAdd(&s_red[SBH_LISTED], 1u);
                }
            }
        }
        if (adjacency) s_key[2u * j] = k0, s_key[2u * j + 1u] = k1;
    }
    __syncthreads();

    // ---- ends and material, every word once: a lane per WORD of the scene's rows (4-byte alignment is all that is asked for)
    if (ends) {
        int32_t *row = ends + (size_t)scene * maxB * 2u;
        for (uint32_t i = tid; i < 2u * maxB; i += SBH_BLOCK) {
            const uint32_t d = i >> 1;
            int32_t v = -1;
            if ((s_listed[d >> 5] >> (d & 31u)) & 1u) {
                const uint32_t w = g_bword[d];
                v = (int32_t)s_pmap[(i & 1u) ? w >> 16 : w & 0xffffu];
            }
            row[i] = v;
        }
    }
    if (material) {
        uint32_t *row = material + (size_t)scene * maxB * SB_BATCH_GRAPH_MATERIAL_WORDS;
        for (uint32_t i = tid; i < maxB * SB_BATCH_GRAPH_MATERIAL_WORDS; i += SBH_BLOCK) {
            const uint32_t d = i / SB_BATCH_GRAPH_MATERIAL_WORDS, q = i - d * SB_BATCH_GRAPH_MATERIAL_WORDS;
            row[i] = ((s_listed[d >> 5] >> (d & 31u)) & 1u) ? g_bmat[(size_t)SB_BATCH_MAT_ROW * d + q] : 0u;
        }
    }
    if (!adjacency && !histogram) return; // (uniform)

    // ---- one bitonic network over the n_keys keys; every pass ends in one barrier (the trip counts are workgroup-uniform)
    for (uint32_t k = 2u; k <= n_keys; k <<= 1)
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            for (uint32_t t = tid; t < (n_keys >> 1); t += SBH_BLOCK) {
                const uint32_t i = sbg::bitonic_low(t, j), l = i | j, x = s_key[i], y = s_key[l];
                if ((x > y) == ((i & k) == 0u)) s_key[i] = y, s_key[l] = x;
            }
            __syncthreads();
        }

    // ---- row_ptr: the keys below particle p's smallest; [maxP] is the number of half-edges (SBG_NO_KEY lies above every bound)
    // (with the histogram no key was sorted -- n_keys is 0 -- and s_rp holds the degrees themselves: it stays)
    int32_t *rrow = row_ptr ? row_ptr + (size_t)scene * (maxP + 1u) : nullptr;
    if (adjacency) {
        for (uint32_t p = tid; p <= maxP; p += SBH_BLOCK) {
            const uint32_t r = sbg::lower_bound(s_key, n_keys, sbg::first_key_of(p));
            s_rp[p] = r;
            if (rrow) rrow[p] = (int32_t)r;
        }
        __syncthreads();
    }
    const uint32_t n_half = adjacency ? s_rp[maxP] : 2u * s_red[SBH_LISTED]; // (<= 2 Bc <= 2 maxB)

    // ---- nbr: sorted position i is row i; {-1, -1} behind the last half-edge
    if (nbr) {
        int32_t *row = nbr + (size_t)scene * maxB * 4u;
        for (uint32_t i = tid; i < 2u * maxB; i += SBH_BLOCK) {
            int32_t other = -1, beam = -1;
            if (i < n_half) {
                const uint32_t k = s_key[i], d = sbg::key_beam(k), w = g_bword[d];
                other = (int32_t)s_pmap[sbg::key_side(k) ? w & 0xffffu : w >> 16];
                beam = (int32_t)d;
            }
            row[2u * i] = other, row[2u * i + 1u] = beam;
        }
    }
    if (!counts) return; // (uniform)

    // ---- the count words: a sum and a maximum of (degree, smallest data index first), order-free
    uint32_t nodes = 0u, best = 0u;
    for (uint32_t p = tid; p < maxP; p += SBH_BLOCK) {
        const uint32_t deg = adjacency ? s_rp[p + 1u] - s_rp[p] : s_rp[p];
        if (deg) {
            nodes++;
            best = max(best, (deg << SBG_PARTICLE_BITS) | (SBH_PMASK - p));
        }
    }
    if (nodes) {
        atomicAdd(&s_red[SBH_NODES], nodes);
        atomicMax(&s_red[SBH_BEST], best);
    }
    __syncthreads();
    if (tid != 0u) return;
    int32_t *c = counts + (size_t)scene * SB_BATCH_GRAPH_COUNT_WORDS;
    const uint32_t key = s_red[SBH_BEST];
    c[0] = (int32_t)(n_half >> 1);
    c[1] = (int32_t)s_red[SBH_NODES];
    c[2] = (int32_t)(key >> SBG_PARTICLE_BITS);
    c[3] = key ? (int32_t)(SBH_PMASK - (key & SBH_PMASK)) : -1;
}

// ---------------------------------------------------------------- host
bool sbb_graph_info(sb_batch *b, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "graph_count_words") *value = SB_BATCH_GRAPH_COUNT_WORDS;
    else if (k == "graph_material_words") *value = SB_BATCH_GRAPH_MATERIAL_WORDS;
    else if (k == "graph_lds_bytes") *value = sbh_lds_bytes(b->V.maxP, b->V.maxB);
    else return sbb_kernel_info(b, "graph", (const void *)k_batch_graph, b->graph_res, key, value);
    return true;
}

sb_status sb_batch_graph_device(sb_batch *b, uint32_t flags, void *device_ends_i32, void *device_material_f32, void *device_row_ptr_i32,
                                void *device_nbr_i32, void *device_counts_i32)
{
    if (!b) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_graph_device: null batch");
    if (flags & ~SB_GRAPH_SKIP_PENDING) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_graph_device: flags 0x%x: only SB_GRAPH_SKIP_PENDING is known", flags);
    if (sbb_misaligned4({device_ends_i32, device_material_f32, device_row_ptr_i32, device_nbr_i32, device_counts_i32}))
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_graph_device: the device buffers must be 4-byte aligned");
    if (device_nbr_i32 && !device_row_ptr_i32) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_graph_device: nbr without row_ptr: its rows could not be found");
    if (!device_ends_i32 && !device_material_f32 && !device_row_ptr_i32 && !device_counts_i32) return SB_OK; // nothing is wanted
    SB_HIP(b, hipSetDevice(b->device));
    const SbBatchView &V = b->V;
    k_batch_graph<<<b->opt.n_scenes, SBH_BLOCK, sbh_lds_bytes(V.maxP, V.maxB), b->stream>>>(
        V, (flags & SB_GRAPH_SKIP_PENDING) ? 1u : 0u, (int32_t *)device_ends_i32, (uint32_t *)device_material_f32, (int32_t *)device_row_ptr_i32,
        (int32_t *)device_nbr_i32, (int32_t *)device_counts_i32);
    return check_launch(b, "sb_batch_graph_device");
}
