// sb_batch_cut.hip -- cutting beams in every scene of a batch in ONE launch (sb_batch_cut_device of include/softbody.h; gfx950,
// wave64).
//
// One workgroup per scene, a lane per live beam slot: the slot's data index through the state blob's beam mapping, its endpoint
// slots through the constant blob, their positions from the particle records at their data indices, the scene's k shapes from LDS,
// the predicate of sb_cut_math.h -- sb_cut_device's definition word for word.  A hit raises the slot's bit in the scene's pending
// break flags (one bit per beam SLOT: what k_batch_frame's delete pass reads), with a vector atomic.  The hit bytes are staged in
// LDS so that the row is zero-filled and written once.  A scene that is hit nowhere is not written at all.
#include "sb_batch.h"
#include "sb_cut_math.h"

#define SBU_BLOCK 256u
enum { SBU_TESTED, SBU_HIT, SBU_FLAGGED, SBU_ALREADY, SBU_NWORDS };

static_assert(SBU_NWORDS == SB_CUT_COUNT_WORDS, "the count words of sb_cut_device");
static_assert(SB_BATCH_MAX_BEAMS % 4u == 0u, "the staged hit bytes are followed by words");

// LDS of a workgroup: hit[maxB rounded up to 4] bytes, the shapes, the count words
static inline uint32_t sbu_lds_bytes(uint32_t maxB) { return ((maxB + 3u) & ~3u) + (SB_CUT_MAX_SHAPES * SBX_SHAPE_WORDS + SBU_NWORDS) * 4u; }

__global__ __launch_bounds__(SBU_BLOCK) void k_batch_cut(SbBatchView V, const uint32_t *__restrict__ shapes, uint32_t k, uint32_t dry,
                                                         uint8_t *__restrict__ hit, int32_t *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sbu_lds[];
    const uint32_t scene = blockIdx.x, tid = threadIdx.x;
    if (scene >= V.n_scenes) return;
    const uint32_t maxB = V.maxB, hit_words = (maxB + 3u) >> 2;
    uint8_t *s_hit = (uint8_t *)sbu_lds;                        // [maxB] per beam DATA index
    uint32_t *s_shape = sbu_lds + hit_words;                    // [k][8]
    uint32_t *s_cnt = s_shape + SB_CUT_MAX_SHAPES * SBX_SHAPE_WORDS; // [SBU_NWORDS]

    const SbbScene hd = sbb_scene(V, scene);
    const uint32_t Bc = hd.Bc;
    const uint32_t *g_pmap = (const uint32_t *)(hd.cst + V.o_pmap), *g_bword = (const uint32_t *)(hd.cst + V.o_bword);
    const uint32_t *g_bmap = (const uint32_t *)(hd.st + V.o_bmap);
    const float2 *g_part = (const float2 *)(hd.st + V.o_part);
    uint32_t *g_bflags = (uint32_t *)(V.st + (size_t)scene * V.st_bytes + V.o_bflags);

    for (uint32_t w = tid; w < hit_words; w += SBU_BLOCK) sbu_lds[w] = 0u;
    for (uint32_t i = tid; i < k * SBX_SHAPE_WORDS; i += SBU_BLOCK) s_shape[i] = shapes[(size_t)scene * k * SBX_SHAPE_WORDS + i];
    if (tid < SBU_NWORDS) s_cnt[tid] = 0u;
    __syncthreads();

    // (the trip count is workgroup-uniform: every lane of a wave reaches the ballots)
    for (uint32_t j0 = 0; j0 < Bc; j0 += SBU_BLOCK) {
        const uint32_t j = j0 + tid;
        bool live = j < Bc, h = false, already = false;
        if (live) {
            const uint32_t d = g_bmap[j], w = g_bword[d];
            // (an upload is refused unless its data indices are inside the capacity and its endpoints are slots < P)
            const float2 a = g_part[3u * g_pmap[w & 0xffffu]], b = g_part[3u * g_pmap[w >> 16]];
            const sbx::P2 A{a.x, a.y}, B{b.x, b.y};
            for (uint32_t q = 0; q < k && !h; q++) h = sbx::shape_hits(sbx::shape_of(s_shape + q * SBX_SHAPE_WORDS), A, B);
            if (h) {
                const uint32_t bit = 1u << (j & 31u);
                already = (g_bflags[j >> 5] & bit) != 0u;
                if (d < maxB) s_hit[d] = 1u;
                if (!dry && !already) atomicOr(&g_bflags[j >> 5], bit);
            }
        }
        const unsigned long long m_live = __ballot(live), m_hit = __ballot(h), m_already = __ballot(already);
        if (__lane_id() == 0u) {
            if (m_live) atomicAdd(&s_cnt[SBU_TESTED], (uint32_t)__popcll(m_live));
            if (m_hit) atomicAdd(&s_cnt[SBU_HIT], (uint32_t)__popcll(m_hit));
            if (!dry && (m_hit & ~m_already)) atomicAdd(&s_cnt[SBU_FLAGGED], (uint32_t)__popcll(m_hit & ~m_already));
            if (m_already) atomicAdd(&s_cnt[SBU_ALREADY], (uint32_t)__popcll(m_already));
        }
    }
    __syncthreads();
    if (hit) {
        uint8_t *row = hit + (size_t)scene * maxB; // (no alignment is asked for: bytes)
        for (uint32_t d = tid; d < maxB; d += SBU_BLOCK) row[d] = s_hit[d];
    }
    if (counts && tid < SBU_NWORDS) counts[(size_t)scene * SBU_NWORDS + tid] = (int32_t)s_cnt[tid];
}

// ---------------------------------------------------------------- host
bool sbb_cut_info(sb_batch *b, const char *key, uint64_t *value)
{
    return sbb_kernel_info(b, "cut", (const void *)k_batch_cut, b->cut_res, key, value);
}

sb_status sb_batch_cut_device(sb_batch *b, uint32_t flags, const void *device_shapes, uint32_t k, void *device_hit_u8, void *device_counts_i32)
{
    SB_TRY(sbb_edit_entry(b, "sb_batch_cut_device", flags, SB_CUT_DRY_RUN, "SB_CUT_DRY_RUN is", k, SB_CUT_MAX_SHAPES, "shapes", device_shapes,
                          {device_shapes, device_counts_i32}, "shapes and counts"));
    k_batch_cut<<<b->opt.n_scenes, SBU_BLOCK, sbu_lds_bytes(b->V.maxB), b->stream>>>(b->V, (const uint32_t *)device_shapes, k,
                                                                                   (flags & SB_CUT_DRY_RUN) ? 1u : 0u, (uint8_t *)device_hit_u8,
                                                                                   (int32_t *)device_counts_i32);
    return check_launch(b, "sb_batch_cut_device");
}
