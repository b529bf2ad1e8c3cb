// sb_batch_add.hip -- adding beams ("welds") in every scene of a batch in ONE launch, the inverse of a cut
// (sb_batch_add_beams_device of include/softbody.h; gfx950, wave64).
//
// One workgroup per scene.  All lanes build, in LDS, the data -> slot inverse of the particle mapping and the bitmap of the FREE beam
// data indices (balive == 0 in the current AND in the reset state blob) with its prefix (sb_batch_alloc.h).  A lane per row
// takes the row's verdict (sb_batch_add_math.h) and its endpoint slots; with SB_BATCH_ADD_SKIP_JOINED all lanes then sweep the live
// beam slots against the rows' unordered slot pairs.  Wave 0 finishes: in-call duplicates, the allocator's finish (rank, room, the
// r-th free index, result and counts), the rows of the constant and the state blob, the pending bits of the new slots, the count.
// Everything behind the float length is integers; every store is a plain vector store of this workgroup into its own scene.
#include "sb_batch.h"
#include "sb_batch_add_math.h"

#define SBW_BLOCK 256u

static_assert(SBA_COUNT_WORDS == SB_BATCH_ADD_COUNT_WORDS, "the count words of sb_batch_add_beams_device: added, invalid, joined, full");
static_assert(SB_BATCH_ADD_MAX == 64u, "a lane of wave 0 per row, one ballot for the ranks");
static_assert(sizeof(sb_batch_new_beam) == SBA_ROW_WORDS * 4u, "a row is 8 words");
static_assert(sba::EMPTY == SB_BATCH_ADD_EMPTY && sba::INVALID == SB_BATCH_ADD_INVALID && sbw::SBW_JOINED == SB_BATCH_ADD_JOINED &&
                  sba::FULL == SB_BATCH_ADD_FULL,
              "the row codes");
static_assert(sbw::SBW_DRY_RUN == SB_BATCH_ADD_DRY_RUN && sbw::SBW_LENGTH_CURRENT == SB_BATCH_ADD_LENGTH_CURRENT &&
                  sbw::SBW_SKIP_JOINED == SB_BATCH_ADD_SKIP_JOINED,
              "the flags");
static_assert(SB_BATCH_MAX_PARTICLES <= 0xFFFFu, "the inverse holds slots in 16 bits, 0xFFFF: no slot");
static_assert(SB_BATCH_MAX_BEAMS <= 32u * SBA_MAX_WORDS, "the free bitmap of the beam data indices");

#define SBW_NO_SLOT 0xFFFFu
// words of the fixed part of a workgroup's LDS: rows, per row {verdict, length, current distance, endpoint slots, unordered key},
// the rows a live beam joins (two words)
#define SBW_FIXED_WORDS (SB_BATCH_ADD_MAX * SBA_ROW_WORDS + 5u * SB_BATCH_ADD_MAX + 2u)
// LDS of a workgroup: the fixed part, the bitmap and its prefix (one word more), the inverse (16 bits per particle data index)
static inline uint32_t sbw_lds_bytes(uint32_t maxP, uint32_t maxB) { return (SBW_FIXED_WORDS + 2u * sba::bitmap_words(maxB) + 1u + ((maxP + 1u) >> 1)) * 4u; }

__global__ __launch_bounds__(SBW_BLOCK) void k_batch_add_beams(SbBatchView V, const uint32_t *__restrict__ rows, uint32_t k, uint32_t flags,
                                                               int32_t *__restrict__ result, int32_t *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sbw_lds[];
    const uint32_t scene = blockIdx.x, tid = threadIdx.x;
    if (scene >= V.n_scenes) return;
    const uint32_t maxP = V.maxP, maxB = V.maxB, nbw = sba::bitmap_words(maxB), inv_words = (maxP + 1u) >> 1;
    uint32_t *s_row = sbw_lds;                                    // [64][8]
    int32_t *s_verd = (int32_t *)(s_row + SB_BATCH_ADD_MAX * SBA_ROW_WORDS); // [64]
    float *s_len = (float *)(s_verd + SB_BATCH_ADD_MAX);          // [64] resolved length
    float *s_cur = s_len + SB_BATCH_ADD_MAX;                      // [64] current distance
    uint32_t *s_ends = (uint32_t *)(s_cur + SB_BATCH_ADD_MAX);    // [64] slot(a) | slot(b) << 16
    uint32_t *s_key = s_ends + SB_BATCH_ADD_MAX;                  // [64] min slot | max slot << 16
    uint32_t *s_joined = s_key + SB_BATCH_ADD_MAX;                // [2] rows a live beam joins
    uint32_t *s_free = s_joined + 2u;                             // [nbw] bit d: beam data index d is free
    uint32_t *s_pref = s_free + nbw;                              // [nbw + 1] free indices in front of each word; [nbw]: all
    uint16_t *s_inv = (uint16_t *)(s_pref + nbw + 1u);            // [maxP] data index -> slot

    const SbbScene hd = sbb_scene(V, scene);
    const uint32_t P = hd.P, Bc = hd.Bc;
    unsigned char *cst = V.cst + (size_t)scene * V.cst_bytes, *st = V.st + (size_t)scene * V.st_bytes;
    const unsigned char *rst = V.rst + (size_t)scene * V.st_bytes;
    const uint32_t *g_pmap = (const uint32_t *)(cst + V.o_pmap);
    const float2 *g_part = (const float2 *)(st + V.o_part);
    uint32_t *g_bword = (uint32_t *)(cst + V.o_bword), *g_bmap = (uint32_t *)(st + V.o_bmap), *g_bflags = (uint32_t *)(st + V.o_bflags);
    const bool dry = (flags & SB_BATCH_ADD_DRY_RUN) != 0u, skip_joined = (flags & SB_BATCH_ADD_SKIP_JOINED) != 0u;

    // ---- rows, the inverse (empty), the free bitmap
    for (uint32_t i = tid; i < k * SBA_ROW_WORDS; i += SBW_BLOCK) s_row[i] = rows[(size_t)scene * k * SBA_ROW_WORDS + i];
    for (uint32_t i = tid; i < inv_words; i += SBW_BLOCK) ((uint32_t *)s_inv)[i] = 0xFFFFFFFFu;
    if (tid < 2u) s_joined[tid] = 0u;
    // (the alive bytes of the current and of the reset state: a state blob's row of them is padded to 16 bytes)
    sba::fill_free(s_free, s_pref, nbw, (const uint32_t *)(st + V.o_balive), (const uint32_t *)(rst + V.o_balive), maxB, hd.loaded != 0u, tid, SBW_BLOCK);
    for (uint32_t s = tid; s < P; s += SBW_BLOCK) {
        const uint32_t d = g_pmap[s];
        if (d < maxP) s_inv[d] = (uint16_t)s; // (an upload is refused unless its particle data indices are inside the capacity, each once)
    }
    __syncthreads();

    // ---- the verdict of each row, a lane per row
    if (tid < k) {
        const uint32_t *w = s_row + tid * SBA_ROW_WORDS;
        const int32_t a = (int32_t)w[0], b = (int32_t)w[1];
        uint32_t sa = SBW_NO_SLOT, sb = SBW_NO_SLOT;
        float cur = 0.0f, len = 0.0f;
        if (hd.loaded && sbw::ends_in_range(a, b, maxP)) {
            sa = s_inv[a], sb = s_inv[b];
            if (sa != SBW_NO_SLOT && sb != SBW_NO_SLOT) {
                const float2 pa = g_part[3u * (uint32_t)a], pb = g_part[3u * (uint32_t)b];
                cur = sb_length(pb.x - pa.x, pb.y - pa.y);
            }
        }
        s_verd[tid] = sbw::row_verdict(w, flags, maxP, hd.loaded != 0u, sa != SBW_NO_SLOT, sb != SBW_NO_SLOT, cur, &len);
        s_len[tid] = len;
        s_cur[tid] = cur;
        s_ends[tid] = sa | (sb << 16);
        s_key[tid] = sa < sb ? sa | (sb << 16) : sb | (sa << 16);
    }
    __syncthreads();

    // ---- joined by a live beam: every live slot against the candidate rows (slots, not data indices: the mapping is one to one)
    if (skip_joined) {
        for (uint32_t j = tid; j < Bc; j += SBW_BLOCK) {
            const uint32_t d = g_bmap[j];
            if (d >= maxB) continue; // (an upload is refused unless its beam data indices are inside the capacity)
            const uint32_t w = g_bword[d], x = w & 0xffffu, y = w >> 16, key = x < y ? x | (y << 16) : y | (x << 16);
            for (uint32_t q = 0; q < k; q++)
                if (s_verd[q] == sba::CANDIDATE && s_key[q] == key) atomicOr(&s_joined[q >> 5], 1u << (q & 31u));
        }
        __syncthreads();
    }
    if (tid >= 64u) return; // wave 0 finishes (k <= 64: a lane per row)

    // ---- duplicates inside the call, room, the r-th free index
    const bool row = tid < k;
    int32_t verd = row ? s_verd[tid] : (int32_t)sba::EMPTY;
    if (skip_joined && verd == sba::CANDIDATE) {
        bool joined = ((s_joined[tid >> 5] >> (tid & 31u)) & 1u) != 0u;
        // (an earlier candidate row of the same pair: were it joined itself, by a beam or by a row before it, so would this one be)
        for (uint32_t i = 0; i < tid && !joined; i++) joined = s_verd[i] == sba::CANDIDATE && s_key[i] == s_key[tid];
        if (joined) verd = sbw::SBW_JOINED;
    }
    const sba::Finish f = sba::finish(verd, tid, Bc, maxB, s_free, s_pref, nbw);
    const uint32_t d = f.index, n_add = f.n_added;

    if (!dry && n_add != 0u) {
        if (f.add && d < maxB) {
            const uint32_t slot = Bc + f.rank;
            const uint32_t *w = s_row + tid * SBA_ROW_WORDS;
            const float len = s_len[tid];
            float *m = (float *)(cst + V.o_bmat) + (size_t)SB_BATCH_MAT_ROW * d;
            g_bword[d] = s_ends[tid];
            m[0] = len, m[1] = sbw::word_as_float(w[3]), m[2] = sbw::word_as_float(w[4]), m[3] = sbw::word_as_float(w[5]);
            m[4] = sbw::word_as_float(w[6]);
            m[5] = sb_div(1.0f, len); // one IEEE divide per beam, as at upload
            (cst + V.o_bex)[d] = 1;
            ((float4 *)(st + V.o_bstate))[d] = make_float4(len, s_cur[tid], 0.0f, 0.0f);
            g_bmap[slot] = d;
            (st + V.o_balive)[d] = 1;
        }
        // the pending bits of the new slots Bc .. Bc + n_add - 1 (at most three flag words): a lane per word
        const uint32_t w0 = Bc >> 5, w1 = (Bc + n_add - 1u) >> 5, fw = w0 + tid;
        if (fw <= w1 && fw < V.nflagw) {
            const uint32_t lo = fw == w0 ? (Bc & 31u) : 0u, hi = fw == w1 ? ((Bc + n_add - 1u) & 31u) : 31u; // bits lo .. hi
            const uint32_t mask = (hi == 31u ? 0xFFFFFFFFu : (1u << (hi + 1u)) - 1u) & ~((1u << lo) - 1u);
            g_bflags[fw] &= ~mask;
        }
        if (tid == 0u) V.meta[(size_t)scene * SB_BM_WORDS + SB_BM_B] = Bc + n_add;
    }
    sba::report(f, row, tid, scene, k, result, counts);
}

// ---------------------------------------------------------------- host
bool sbb_add_info(sb_batch *b, const char *key, uint64_t *value)
{
    return sbb_kernel_info(b, "add_beams", (const void *)k_batch_add_beams, b->add_res, key, value);
}

sb_status sb_batch_add_beams_device(sb_batch *b, uint32_t flags, const void *device_rows, uint32_t k, void *device_result_i32, void *device_counts_i32)
{
    SB_TRY(sbb_edit_entry(b, "sb_batch_add_beams_device", flags, SB_BATCH_ADD_DRY_RUN | SB_BATCH_ADD_LENGTH_CURRENT | SB_BATCH_ADD_SKIP_JOINED,
                          "SB_BATCH_ADD_DRY_RUN, _LENGTH_CURRENT and _SKIP_JOINED are", k, SB_BATCH_ADD_MAX, "rows", device_rows,
                          {device_rows, device_result_i32, device_counts_i32}, "rows, result and counts"));
    k_batch_add_beams<<<b->opt.n_scenes, SBW_BLOCK, sbw_lds_bytes(b->V.maxP, b->V.maxB), b->stream>>>(
        b->V, (const uint32_t *)device_rows, k, flags, (int32_t *)device_result_i32, (int32_t *)device_counts_i32);
    return check_launch(b, "sb_batch_add_beams_device");
}
