// sb_cut.hip -- cutting beams on the device (sb_cut_device / sb_cut of include/softbody.h; gfx950, wave64).
//
// A cut raises the pending break flag of every live beam a knife stroke crosses or an eraser disc covers: the bit the substep
// would have raised had the beam broken.  Everything downstream -- the delete pass of either layout, the reports, the checkpoint,
// the hybrid's k_hybrid_to_tiled -- already handles a pending flag, so nothing there changes.  Two launches:
//   k_cut_decide  a lane per caller beam slot of the latest upload: its endpoints through the shared scene tables (sb_report.h:
//                 data index -> internal particle, the current particle buffer), the call's shapes from LDS, the predicate of
//                 sb_cut_math.h; writes `hit` at the beam's data index and a mark per ENGINE slot; counts with ballots, the waves'
//                 counts combined in LDS, one 64-bit add per workgroup and count word (integers: any order gives the same bits)
//   k_cut_apply   a lane per beam COPY (tiled / atomic layouts: a beam cut by a tile boundary has one in each tile; blocked layout:
//                 one per blocked beam): the copy's engine slot from the per-copy slot word, its bit ORed into the mask the delete
//                 pass of the engine's layout reads (e->d_broken on every path)
// The engine's positions are read where they are; no host copy of them exists or is made.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "sb_report.h"
#include "sb_cut_math.h"

#define SBX_BLOCK 256u
enum { SBX_TESTED, SBX_HIT, SBX_FLAGGED, SBX_ALREADY }; // the count words (SB_CUT_COUNT_WORDS)

static_assert(sizeof(sb_cut_shape) == SBX_SHAPE_WORDS * 4u, "a shape is 8 words");
static_assert(SB_CUT_SEGMENT == 1u && SB_CUT_DISC == 2u, "sb_cut_math.h spells the kinds as numbers");

// tab: [4][n] = data index of A, data index of B, engine slot, the copy read back, per caller beam slot; row: its beam data index
__global__ __launch_bounds__(SBX_BLOCK) void k_cut_decide(const uint32_t *__restrict__ tab, uint32_t n, const uint32_t *__restrict__ row,
                                                          const uint32_t *__restrict__ pinv, const float2 *__restrict__ pos,
                                                          const uint32_t *__restrict__ dead, const uint32_t *__restrict__ broken,
                                                          const uint32_t *__restrict__ shapes, uint32_t n_shapes, uint32_t dry,
                                                          uint8_t *hit, uint8_t *mark, unsigned long long *counts)
{
    __shared__ uint32_t s_shape[SB_CUT_MAX_SHAPES * SBX_SHAPE_WORDS];
    __shared__ uint32_t s_cnt[SB_CUT_COUNT_WORDS];
    for (uint32_t i = threadIdx.x; i < n_shapes * SBX_SHAPE_WORDS; i += SBX_BLOCK) s_shape[i] = shapes[i];
    if (threadIdx.x < SB_CUT_COUNT_WORDS) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t u = blockIdx.x * SBX_BLOCK + threadIdx.x;
    bool live = false, h = false, already = false;
    if (u < n) {
        const uint32_t slot = tab[2u * (size_t)n + u];
        live = !(dead && dead[slot] != 0u);
        if (live) {
            const float2 a = pos[pinv[tab[u]]], b = pos[pinv[tab[(size_t)n + u]]];
            const sbx::P2 A{a.x, a.y}, B{b.x, b.y};
            for (uint32_t k = 0; k < n_shapes && !h; k++) h = sbx::shape_hits(sbx::shape_of(s_shape + k * SBX_SHAPE_WORDS), A, B);
            if (h) {
                // ONE copy's bit speaks for the beam, the copy sb_load_buffers and sb_summary read: every copy of a beam carries
                // the same pending bit at a launch boundary (each copy evaluates the same strain on the same bits, and
                // k_cut_apply marks all of them)
                const uint32_t c = tab[3u * (size_t)n + u];
                already = ((broken[c >> 5] >> (c & 31u)) & 1u) != 0u;
                if (!dry) mark[slot] = 1u;
            }
        }
        if (hit) hit[row[u]] = h ? 1u : 0u;
    }
    const unsigned long long m_live = __ballot(live), m_hit = __ballot(h), m_already = __ballot(already);
    if (!counts) return; // (uniform)
    // the wave's counts into LDS, then one 64-bit add per workgroup and count word that is not zero (a workgroup counts at most 256)
    if (__lane_id() == 0u) {
        if (m_live) atomicAdd(&s_cnt[SBX_TESTED], (uint32_t)__popcll(m_live));
        if (m_hit) atomicAdd(&s_cnt[SBX_HIT], (uint32_t)__popcll(m_hit));
        if (!dry && (m_hit & ~m_already)) atomicAdd(&s_cnt[SBX_FLAGGED], (uint32_t)__popcll(m_hit & ~m_already));
        if (m_already) atomicAdd(&s_cnt[SBX_ALREADY], (uint32_t)__popcll(m_already));
    }
    __syncthreads();
    if (threadIdx.x < SB_CUT_COUNT_WORDS && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// slot: per copy its engine slot (0xFFFFFFFF: a padding copy); mark: per engine slot "this call hit it"
__global__ __launch_bounds__(SBX_BLOCK) void k_cut_apply(const uint32_t *__restrict__ slot, uint32_t ncopies, uint32_t nslots,
                                                         const uint8_t *__restrict__ mark, uint32_t *broken)
{
    const uint32_t c = blockIdx.x * SBX_BLOCK + threadIdx.x;
    if (c >= ncopies) return;
    const uint32_t s = slot[c];
    const uint32_t bit = 1u << (c & 31u);
    if (s < nslots && mark[s] && !(broken[c >> 5] & bit)) atomicOr(&broken[c >> 5], bit); // (a bit already pending: nothing to write)
}

// ---------------------------------------------------------------- host side

// per caller beam slot of the latest upload the data index of its record (sb_load_buffers' beam loop)
sb_status sbx_build_rows(sb_engine *e, const char *what) // (sb_report.h: sb_graph.hip reads the same rows)
{
    const auto t0 = std::chrono::steady_clock::now();
    SbStateIoState &s = *e->sio;
    std::vector<uint2> slots;
    SB_TRY(sbq_user_slots(e, what, slots));
    std::vector<uint32_t> row(slots.size());
    for (size_t u = 0; u < slots.size(); u++) row[u] = slots[u].y;
    s.cut_nd = 0;
    for (uint32_t u = 0; u < sb_user_beams(e); u++) s.cut_nd = std::max(s.cut_nd, row[u] + 1u);
    SB_TRY(s.buf[SBX_B_ROW].grow(e, row.size() * 4));
    SB_HIP(e, hipMemcpyAsync(s.buf[SBX_B_ROW].p, row.data(), row.size() * 4, hipMemcpyHostToDevice, e->stream));
    SB_HIP(e, hipStreamSynchronize(e->stream)); // (the host vector goes out of scope)
    s.cut_valid = true;
    s.cut_row_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SB_OK;
}

static sb_status sbx_enqueue(sb_engine *e, const sb_cut_options *o, const void *shapes, uint32_t n_shapes, void *hit, void *counts, bool host)
{
    if (!e) return SB_ERR_INVALID;
    const char *what = host ? "sb_cut" : "sb_cut_device";
    if (n_shapes > SB_CUT_MAX_SHAPES) SB_FAIL(e, SB_ERR_INVALID, "%s: %u shapes, at most %u in a call", what, n_shapes, SB_CUT_MAX_SHAPES);
    if (n_shapes && !shapes) SB_FAIL(e, SB_ERR_INVALID, "%s: null shapes", what);
    if ((uintptr_t)shapes & 3u) SB_FAIL(e, SB_ERR_INVALID, "%s: shapes must be 4-byte aligned", what);
    if ((uintptr_t)counts & 7u) SB_FAIL(e, SB_ERR_INVALID, "%s: counts must be 8-byte aligned", what);
    uint32_t flags = 0u;
    if (o && o->struct_size == sizeof(sb_cut_options)) {
        flags = o->flags;
        if (flags & ~SB_CUT_DRY_RUN) SB_FAIL(e, SB_ERR_INVALID, "%s: flags 0x%x: only SB_CUT_DRY_RUN is known", what, flags);
    }
    if (host)
        for (uint32_t k = 0; k < n_shapes; k++) {
            const sb_cut_shape &sh = ((const sb_cut_shape *)shapes)[k];
            if (sh.kind > SB_CUT_DISC) SB_FAIL(e, SB_ERR_INVALID, "%s: shape %u has kind %u", what, k, sh.kind);
            if (sh.kind == SB_CUT_DISC && !(sh.y1 == 0.0f)) SB_FAIL(e, SB_ERR_INVALID, "%s: shape %u is a disc whose y1 is not 0", what, k);
        }
    SB_TRY(sbq_preflight(e, what, o, "cut", "cuts across ranks are not handled"));
    SB_TRY(sbq_need(e, what, SBQ_PARTICLES | SBQ_BEAMS | SBQ_COPIES));
    SbStateIoState &s = *e->sio;
    if (!s.cut_valid) SB_TRY(sbx_build_rows(e, what));
    s.cut_build_ms = s.part_ms + s.beam_ms + s.copy_ms + s.cut_row_ms;
    s.cuts++;

    const uint32_t n = s.nslots, maxB = e->opt.max_beams;
    const bool dry = (flags & SB_CUT_DRY_RUN) != 0u;
    SbqMirror mir(e, host); // (sb_cut: the same launches on the engine's own copies of the caller's memory)
    const uint32_t *d_shapes = mir.in<uint32_t>(SBX_B_SHAPES, n_shapes ? shapes : nullptr, (size_t)n_shapes * sizeof(sb_cut_shape),
                                                (size_t)SB_CUT_MAX_SHAPES * sizeof(sb_cut_shape));
    uint8_t *d_hit = mir.inout<uint8_t>(SBX_B_HIT, hit, maxB); // (bytes at indices that hold no beam stay the caller's: they travel there and back)
    unsigned long long *d_counts = mir.out<unsigned long long>(SBX_B_ACC, counts, SB_CUT_COUNT_WORDS * sizeof(unsigned long long));
    SB_TRY(mir.st);
    if (d_counts) SB_HIP(e, hipMemsetAsync(d_counts, 0, SB_CUT_COUNT_WORDS * sizeof(unsigned long long), e->stream));
    if (n) {
        uint8_t *d_mark = nullptr;
        if (!dry) {
            SB_TRY(s.buf[SBX_B_MARK].grow(e, e->B));
            d_mark = s.buf[SBX_B_MARK].as<uint8_t>();
            SB_HIP(e, hipMemsetAsync(d_mark, 0, e->B, e->stream));
        }
        auto blocks = [](uint32_t k) { return (k + SBX_BLOCK - 1u) / SBX_BLOCK; };
        k_cut_decide<<<blocks(n), SBX_BLOCK, 0, e->stream>>>(s.buf[SBQ_B_TAB].as<uint32_t>(), n, s.buf[SBX_B_ROW].as<uint32_t>(),
                                                             s.buf[SBQ_B_PINV].as<uint32_t>(), e->part[e->cur].pos, sbq_dead(e), e->d_broken, d_shapes,
                                                             n_shapes, dry ? 1u : 0u, d_hit, d_mark, d_counts);
        if (!dry && n_shapes && e->nbeam)
            k_cut_apply<<<blocks(e->nbeam), SBX_BLOCK, 0, e->stream>>>(e->beams.slot, e->nbeam, e->B, d_mark, e->d_broken);
        SB_HIP(e, hipGetLastError());
    }
    return mir.finish();
}

// what sb_get_info reads ("cuts", "cut_table_build_us", "cut_kernel_vgprs")
bool sbx_info(sb_engine *e, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "cuts") *value = e->sio ? e->sio->cuts : 0u;
    else if (k == "cut_table_build_us") *value = e->sio ? (uint64_t)(e->sio->cut_build_ms * 1000.0 + 0.5) : 0u;
    else if (k == "cut_kernel_vgprs") return sbq_kernel_most(e, {(const void *)k_cut_decide, (const void *)k_cut_apply}, true, value);
    else return false;
    return true;
}

extern "C" {

sb_status sb_cut_device(sb_engine *e, const sb_cut_options *opts, const void *device_shapes, uint32_t n_shapes, void *device_hit_u8,
                        void *device_counts_i64)
{
    SB_GUARDED(e, sbx_enqueue(e, opts, device_shapes, n_shapes, device_hit_u8, device_counts_i64, false))
}

sb_status sb_cut(sb_engine *e, const sb_cut_options *opts, const sb_cut_shape *shapes, uint32_t n_shapes, uint8_t *hit, int64_t *counts)
{
    SB_GUARDED(e, sbx_enqueue(e, opts, shapes, n_shapes, hit, counts, true))
}

} // extern "C"
