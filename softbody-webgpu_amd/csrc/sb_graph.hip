// sb_graph.hip -- the beam graph of the whole scene on the device: edge list and CSR adjacency at the caller's data indices
// (sb_graph_device / sb_graph of include/softbody.h; gfx950, wave64).
//
// The tables are the reports' shared ones (sb_report.h: per caller beam slot the data indices of both endpoints, the engine slot,
// the copy read back) and sb_cut.hip's rows (per caller slot its beam data index).  Stages, all enqueued on the engine's stream:
//   k_graph_edges   a lane per caller beam slot: live as sb_bodies has it, listed unless SKIP_PENDING and the copy's pending bit;
//                   writes ends at the beam's data index, adds one to the degree of both endpoints (integer atomics: sums of
//                   ones do not depend on order) and, where nbr is wanted, writes the beam's two half-edge keys
//                   (particle << 32 | 2 d + side) and their neighbours at positions 2 d and 2 d + 1
//   sbq_scan        the degrees into the 64-bit row_ptr (the reports' three-launch exclusive scan)
//   sbq_sort        the stable radix sort of sb_report.hip by the keys' particle halves; the keys stand in (beam, side) order, so the
//                   result is in (particle, beam, side) order: the one order the definition names
//   k_graph_nbr     a lane per row of nbr
//   k_graph_degrees / k_graph_counts   a 64-bit sum and a 64-bit maximum of (degree, smallest data index first), then the four words
// Integers only.  Nothing of the engine is written; nothing is read back.
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "sb_report.h"

#define SBG_BLOCK 256u
enum { SBG_A_LISTED, SBG_A_NODES, SBG_A_BEST, SBG_NACC }; // the accumulators (64-bit words)

// tab: [4][n] = data index of A, data index of B, engine slot, the copy read back, per caller beam slot; row: its beam data index
__global__ __launch_bounds__(SBG_BLOCK) void k_graph_edges(const uint32_t *__restrict__ tab, uint32_t n, const uint32_t *__restrict__ row,
                                                           const uint32_t *__restrict__ dead, const uint32_t *__restrict__ broken, uint32_t skip_pending,
                                                           uint32_t max_beams, uint32_t max_particles, int32_t *ends, uint32_t *deg,
                                                           unsigned long long *keys, uint32_t *other, uint32_t nd, unsigned long long *acc)
{
    const uint32_t u = blockIdx.x * SBG_BLOCK + threadIdx.x;
    bool listed = false;
    if (u < n) {
        const uint32_t slot = tab[2u * (size_t)n + u];
        listed = !(dead && dead[slot] != 0u);
        if (listed && skip_pending) {
            const uint32_t c = tab[3u * (size_t)n + u]; // (one copy's bit speaks for the beam: sb_cut.hip)
            listed = ((broken[c >> 5] >> (c & 31u)) & 1u) == 0u;
        }
        const uint32_t d = row[u], a = tab[u], b = tab[(size_t)n + u];
        // (the table builders refuse a scene whose indices leave the capacity; the tests keep every store inside its buffer)
        if (listed && d < max_beams && a < max_particles && b < max_particles) {
            if (ends) ends[2u * (size_t)d] = (int32_t)a, ends[2u * (size_t)d + 1u] = (int32_t)b;
            if (deg) atomicAdd(&deg[a], 1u), atomicAdd(&deg[b], 1u);
            if (keys && d < nd) {
                const size_t at = 2u * (size_t)d;
                keys[at] = ((unsigned long long)a << 32) | (unsigned long long)at;
                keys[at + 1u] = ((unsigned long long)b << 32) | (unsigned long long)(at + 1u);
                other[at] = b, other[at + 1u] = a;
            }
        } else {
            listed = false;
        }
    }
    const unsigned long long m = __ballot(listed);
    if (acc && m && __lane_id() == 0u) atomicAdd(&acc[SBG_A_LISTED], (unsigned long long)__popcll(m));
}

// the keys of positions that hold no listed half-edge: the particle half `none` is above every particle, the low half keeps the order
__global__ __launch_bounds__(SBG_BLOCK) void k_graph_fill(unsigned long long *keys, uint32_t n2, uint32_t none)
{
    const uint32_t i = blockIdx.x * SBG_BLOCK + threadIdx.x;
    if (i < n2) keys[i] = ((unsigned long long)none << 32) | i;
}

// a lane per row i < H of nbr; sorted: n2 keys, the listed half-edges first
__global__ __launch_bounds__(SBG_BLOCK) void k_graph_nbr(const unsigned long long *__restrict__ sorted, uint32_t n2, uint32_t none,
                                                         const uint32_t *__restrict__ other, unsigned long long H, int32_t *nbr)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * SBG_BLOCK + threadIdx.x;
    if (i >= H) return;
    int32_t o = -1, d = -1;
    if (i < n2) {
        const unsigned long long k = sorted[i];
        if ((uint32_t)(k >> 32) != none) {
            const uint32_t at = (uint32_t)k;
            o = (int32_t)other[at];
            d = (int32_t)(at >> 1);
        }
    }
    nbr[2u * i] = o, nbr[2u * i + 1u] = d;
}

__global__ __launch_bounds__(SBG_BLOCK) void k_graph_degrees(const uint32_t *__restrict__ deg, uint32_t max_particles, unsigned long long *acc)
{
    const uint32_t p = blockIdx.x * SBG_BLOCK + threadIdx.x;
    const uint32_t g = p < max_particles ? deg[p] : 0u;
    const unsigned long long m = __ballot(g != 0u);
    if (m && __lane_id() == 0u) atomicAdd(&acc[SBG_A_NODES], (unsigned long long)__popcll(m));
    if (g) atomicMax(&acc[SBG_A_BEST], ((unsigned long long)g << 32) | (unsigned long long)(0xFFFFFFFFu - p));
}

__global__ void k_graph_counts(const unsigned long long *__restrict__ acc, long long *counts)
{
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    const unsigned long long best = acc[SBG_A_BEST];
    counts[0] = (long long)acc[SBG_A_LISTED];
    counts[1] = (long long)acc[SBG_A_NODES];
    counts[2] = (long long)(best >> 32);
    counts[3] = best ? (long long)(0xFFFFFFFFu - (uint32_t)best) : -1ll;
}

// ---------------------------------------------------------------- host side

static uint32_t sbg_bits(uint64_t most) // bits that hold every value 0 .. most
{
    uint32_t b = 1u;
    while (b < 64u && (most >> b) != 0u) b++;
    return b;
}

static size_t sbg_up(size_t bytes) { return (bytes + 255u) & ~(size_t)255u; }

static sb_status sbg_enqueue(sb_engine *e, const sb_graph_options *o, void *ends, void *row_ptr, void *nbr, void *counts, bool host)
{
    if (!e) return SB_ERR_INVALID;
    const char *what = host ? "sb_graph" : "sb_graph_device";
    uint32_t flags = 0u;
    uint64_t H = 0u;
    if (o && o->struct_size == sizeof(sb_graph_options)) {
        flags = o->flags, H = o->max_half_edges;
        if (flags & ~SB_GRAPH_SKIP_PENDING) SB_FAIL(e, SB_ERR_INVALID, "%s: flags 0x%x: only SB_GRAPH_SKIP_PENDING is known", what, flags);
    }
    if (((uintptr_t)ends | (uintptr_t)nbr) & 3u) SB_FAIL(e, SB_ERR_INVALID, "%s: ends and nbr must be 4-byte aligned", what);
    if (((uintptr_t)row_ptr | (uintptr_t)counts) & 7u) SB_FAIL(e, SB_ERR_INVALID, "%s: row_ptr and counts must be 8-byte aligned", what);
    if (nbr && !row_ptr) SB_FAIL(e, SB_ERR_INVALID, "%s: nbr without row_ptr: its rows could not be found", what);
    if (nbr && H == 0u) SB_FAIL(e, SB_ERR_INVALID, "%s: nbr with max_half_edges == 0", what);
    SB_TRY(sbq_preflight(e, what, o, "reported", "the graph across ranks is not handled"));
    if (!ends && !row_ptr && !counts) return SB_OK; // nothing is wanted
    SB_TRY(sbq_need(e, what, SBQ_PARTICLES | SBQ_BEAMS | SBQ_COPIES));
    SbStateIoState &s = *e->sio;
    if (!s.cut_valid) SB_TRY(sbx_build_rows(e, what));
    s.graph_build_ms = s.part_ms + s.beam_ms + s.copy_ms + s.cut_row_ms;
    const uint32_t n = s.nslots, maxP = e->opt.max_particles, maxB = e->opt.max_beams, nd = s.cut_nd, none = s.np;
    if (nd >= 0x80000000u) SB_FAIL(e, SB_ERR_INVALID, "%s: beam data indices reach 2^31", what);
    const uint32_t n2 = nbr ? 2u * nd : 0u;
    if (!nbr) H = 0u;

    // the call's scratch, one block: degrees [maxP + 1], the scan's block sums, the accumulators, and for nbr two key buffers, the
    // neighbours, the sort's histogram and its scan's block sums
    const bool want_deg = row_ptr || counts;
    const uint64_t nscan = (uint64_t)maxP + 1u, nb_scan = (nscan + SBQ_SCAN - 1u) / SBQ_SCAN;
    const uint64_t nb_sort = ((uint64_t)n2 + SBQ_SORT - 1u) / SBQ_SORT, hist_words = (uint64_t)SBQ_RADIX * nb_sort;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t o0 = at; at += sbg_up(bytes); return o0; };
    const size_t o_acc = take(SBG_NACC * 8), o_deg = take(want_deg ? nscan * 4 : 0), o_bsum = take(row_ptr ? nb_scan * 8 : 0),
                 o_ka = take((size_t)n2 * 8), o_kb = take((size_t)n2 * 8), o_other = take((size_t)n2 * 4),
                 o_hist = take(hist_words * 4), o_hsum = take(((hist_words + SBQ_SCAN - 1u) / SBQ_SCAN) * 4);
    SB_TRY(s.buf[SBG_B_SCRATCH].grow(e, at));
    unsigned char *base = s.buf[SBG_B_SCRATCH].as<unsigned char>();
    unsigned long long *acc = (unsigned long long *)(base + o_acc), *bsum = (unsigned long long *)(base + o_bsum);
    uint32_t *deg = want_deg ? (uint32_t *)(base + o_deg) : nullptr;
    unsigned long long *ka = n2 ? (unsigned long long *)(base + o_ka) : nullptr, *kb = (unsigned long long *)(base + o_kb);
    uint32_t *other = (uint32_t *)(base + o_other), *hist = (uint32_t *)(base + o_hist), *hsum = (uint32_t *)(base + o_hsum);

    SbqMirror mir(e, host);
    int32_t *d_ends = mir.out<int32_t>(SBG_B_ENDS, ends, (size_t)maxB * 8), *d_nbr = mir.out<int32_t>(SBG_B_NBR, nbr, (size_t)H * 8);
    unsigned long long *d_rp = mir.out<unsigned long long>(SBG_B_ROWPTR, row_ptr, (size_t)nscan * 8);
    long long *d_counts = mir.out<long long>(SBG_B_COUNTS, counts, SB_GRAPH_COUNT_WORDS * 8);
    SB_TRY(mir.st);
    auto blocks = [](uint64_t k) { return (uint32_t)((k + SBG_BLOCK - 1u) / SBG_BLOCK); };
    SB_HIP(e, hipMemsetAsync(acc, 0, SBG_NACC * 8, e->stream));
    if (d_ends && maxB) SB_HIP(e, hipMemsetAsync(d_ends, 0xFF, (size_t)maxB * 8, e->stream)); // {-1, -1}
    if (deg) SB_HIP(e, hipMemsetAsync(deg, 0, nscan * 4, e->stream));
    if (n2) k_graph_fill<<<blocks(n2), SBG_BLOCK, 0, e->stream>>>(ka, n2, none);
    if (n) {
        k_graph_edges<<<blocks(n), SBG_BLOCK, 0, e->stream>>>(s.buf[SBQ_B_TAB].as<uint32_t>(), n, s.buf[SBX_B_ROW].as<uint32_t>(), sbq_dead(e), e->d_broken,
                                                              (flags & SB_GRAPH_SKIP_PENDING) ? 1u : 0u, maxB, maxP, d_ends, deg, ka, other, nd, acc);
    }
    if (d_rp) sbq_scan<unsigned long long>(e, deg, nscan, bsum, d_rp, nullptr);
    if (d_nbr) {
        const unsigned long long *sorted = n2 ? sbq_sort(e, ka, kb, n2, nullptr, sbg_bits(none), hist, hsum) : nullptr;
        k_graph_nbr<<<blocks(H), SBG_BLOCK, 0, e->stream>>>(sorted, n2, none, other, H, d_nbr);
    }
    if (d_counts) {
        if (maxP) k_graph_degrees<<<blocks(maxP), SBG_BLOCK, 0, e->stream>>>(deg, maxP, acc);
        k_graph_counts<<<1, 64, 0, e->stream>>>(acc, d_counts);
    }
    SB_HIP(e, hipGetLastError());
    return mir.finish();
}

// what sb_get_info reads ("graph_kernel_vgprs", "graph_kernel_scratch_bytes", "graph_table_build_us")
bool sbg_info(sb_engine *e, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "graph_table_build_us") *value = e->sio ? (uint64_t)(e->sio->graph_build_ms * 1000.0 + 0.5) : 0u;
    else if (k == "graph_kernel_vgprs" || k == "graph_kernel_scratch_bytes") {
        std::vector<const void *> ks = {(const void *)k_graph_edges, (const void *)k_graph_fill, (const void *)k_graph_nbr, (const void *)k_graph_degrees,
                                        (const void *)k_graph_counts};
        for (const void *f : sbq_sort_kernels()) ks.push_back(f);
        for (const void *f : sbq_scan_kernels(true)) ks.push_back(f);
        return sbq_kernel_most(e, ks, k == "graph_kernel_vgprs", value);
    }
    else return false;
    return true;
}

extern "C" {

sb_status sb_graph_device(sb_engine *e, const sb_graph_options *opts, void *device_ends_i32, void *device_row_ptr_i64, void *device_nbr_i32,
                          void *device_counts_i64)
{
    SB_GUARDED(e, sbg_enqueue(e, opts, device_ends_i32, device_row_ptr_i64, device_nbr_i32, device_counts_i64, false))
}

sb_status sb_graph(sb_engine *e, const sb_graph_options *opts, int32_t *ends, int64_t *row_ptr, int32_t *nbr, int64_t *counts)
{
    SB_GUARDED(e, sbg_enqueue(e, opts, ends, row_ptr, nbr, counts, true))
}

} // extern "C"
