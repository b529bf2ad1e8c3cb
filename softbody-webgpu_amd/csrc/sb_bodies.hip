// sb_bodies.hip -- the connected bodies of the whole scene of an sb_engine, labelled on the device (sb_bodies / sb_bodies_device of
// include/softbody.h; gfx950, wave64).
//
// The definition is sb_batch_bodies_device's: nodes = the scene's particles, edges = its LIVE beams (the caller's beam slots of
// the latest upload whose engine slot no delete pass and no plan-keeping upload removed; a pending break flag still connects),
// everything indexed by particle DATA index, a body's label its smallest data index.  k_batch_bodies holds a scene in the LDS of
// one workgroup; here the graph lies in HBM and no workgroup sees it whole, and the call may only enqueue, so nothing may loop
// on a host read-back, and no workgroup may wait for another.  The search is the lock-free union-find with the minimum as root:
//   k_bodies_init     parent[d] = d where a particle lives, -1 elsewhere; sizes and the accumulators zeroed
//   k_bodies_union    a thread per caller beam slot: find both roots (path halving), hook the larger root under the smaller with
//                     ONE compare-and-swap on the larger root's own word; a failed swap means another thread's swap on that word
//                     succeeded, and at most particles - 1 swaps succeed in a launch: every thread ends, none waits
//   k_bodies_flatten  labels[d] = find(d) -- the root IS the smallest data index, by construction -- and the particles per label
//   k_bodies_beams    the live beams per label (at the label of endpoint A)
//   k_bodies_roots    per root: bodies, single-particle bodies, the largest as ONE 64-bit key  size << 32 | ~label  (atomicMax)
//   k_bodies_counts   one thread: the key back into the four count words
// `parent` IS the caller's `labels` when that is given (a scratch array up to the highest data index in use when not): flatten
// works in place, since whatever another thread reads on its way through word d -- the old parent or the root -- is an ancestor.
// Invariants of the parent words while k_bodies_union runs: parent[x] <= x, and parent[x] is an ancestor of x in the forest the
// successful swaps have built (a root only ever gets a smaller root as its parent; halving replaces a parent by an ancestor).
// A halving store may overwrite a later, smaller halving store: the word goes back UP to an older ancestor, never to a
// non-ancestor, and a non-root never becomes a root again (only the swap writes a root's word).  So a stale value costs a step,
// never a bit.  What a stale value may NOT do is survive for ever in this CU's L1 (a find that keeps reading "x is a root" from
// its own L1 after another CU hooked x would retry its swap without end): every access to a parent word in the union launch is
// an agent-scope relaxed atomic, which goes past the L1.
// Counting: a body of a million particles would send a million adds to one address, so lanes of a wave that hold the same label
// as their left neighbour are added by the first lane of their run (sbd_add_runs): neighbouring data indices mostly share a body.
// Integers only: the outputs do not depend on the order in which anything above happens.
#include <algorithm>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "sb_report.h"

#define SBD_BLOCK 256u
#define SBD_NONE 0xFFFFFFFFu

enum { SBD_BODIES, SBD_SINGLES, SBD_KEY, SBD_NACC, SBD_COUNTS = 4 }; // accumulator words; sb_bodies' four count words behind them

// the root of x's tree, every second node on the way pointed at its grandparent
SB_DEV int32_t sbd_find_halving(int32_t *parent, int32_t x)
{
    for (;;) {
        const int32_t p = SB_AGENT_LOAD(&parent[x]);
        if (p == x) return x;
        const int32_t g = SB_AGENT_LOAD(&parent[p]);
        if (g == p) return p;
        SB_AGENT_STORE(&parent[x], g);
        x = g;
    }
}

// Add each maximal run of lanes with the same label l >= 0 to sizes[l][col] with one atomic of its first lane.  Every lane of
// the wave calls it (l = -1: nothing to add).
SB_DEV void sbd_add_runs(int32_t *sizes, int32_t l, uint32_t col)
{
    const uint32_t run = sbq_run_length((uint32_t)l, l >= 0);
    if (run) atomicAdd(&sizes[2u * (size_t)l + col], (int)run);
}

// grid over max(n_parent, n_sizes): parent over n_parent words (a particle lives at d: pinv[d] != none, d < np), sizes over
// n_sizes rows (4-byte aligned only: two stores)
__global__ __launch_bounds__(SBD_BLOCK) void k_bodies_init(const uint32_t *__restrict__ pinv, uint32_t np, int32_t *parent,
                                                           uint32_t n_parent, int32_t *sizes, uint32_t n_sizes,
                                                           unsigned long long *acc)
{
    const uint32_t d = blockIdx.x * SBD_BLOCK + threadIdx.x;
    if (d < n_parent) parent[d] = d < np && pinv[d] != SBD_NONE ? (int32_t)d : -1;
    if (sizes && d < n_sizes) sizes[2u * (size_t)d] = 0, sizes[2u * (size_t)d + 1u] = 0;
    if (acc && d < SBD_NACC) acc[d] = 0ull;
}

// tab: [3][n] = data index of A, data index of B, engine slot, per caller beam slot
__global__ __launch_bounds__(SBD_BLOCK) void k_bodies_union(const uint32_t *__restrict__ tab, uint32_t n,
                                                            const uint32_t *__restrict__ dead, int32_t *parent)
{
    const uint32_t u = blockIdx.x * SBD_BLOCK + threadIdx.x;
    if (u >= n) return;
    if (dead && dead[tab[2u * (size_t)n + u]] != 0u) return;
    int32_t ra = sbd_find_halving(parent, (int32_t)tab[u]), rb = sbd_find_halving(parent, (int32_t)tab[(size_t)n + u]);
    while (ra != rb) {
        const int32_t hi = max(ra, rb), lo = min(ra, rb);
        const int32_t was = atomicCAS(&parent[hi], hi, lo);
        if (was == hi) break;
        ra = sbd_find_halving(parent, was); // (hi got this parent meanwhile)
        rb = sbd_find_halving(parent, lo);
    }
}

// the roots are final (the union launch has ended): walk up, store; COUNT: the particles per label
template <bool COUNT>
__global__ __launch_bounds__(SBD_BLOCK) void k_bodies_flatten(int32_t *parent, uint32_t np, int32_t *sizes)
{
    const uint32_t d = blockIdx.x * SBD_BLOCK + threadIdx.x;
    int32_t l = -1;
    if (d < np) {
        const int32_t p = SB_AGENT_LOAD(&parent[d]);
        l = p;
        if (p >= 0) {
            for (int32_t up; (up = SB_AGENT_LOAD(&parent[l])) != l;) l = up;
            if (l != p) SB_AGENT_STORE(&parent[d], l);
        }
    }
    if constexpr (COUNT) sbd_add_runs(sizes, l, 0u);
}

__global__ __launch_bounds__(SBD_BLOCK) void k_bodies_beams(const uint32_t *__restrict__ tab, uint32_t n,
                                                            const uint32_t *__restrict__ dead, const int32_t *__restrict__ labels,
                                                            int32_t *sizes)
{
    const uint32_t u = blockIdx.x * SBD_BLOCK + threadIdx.x;
    int32_t l = -1;
    if (u < n && !(dead && dead[tab[2u * (size_t)n + u]] != 0u)) l = labels[tab[u]];
    sbd_add_runs(sizes, l, 1u);
}

__global__ __launch_bounds__(SBD_BLOCK) void k_bodies_roots(const int32_t *__restrict__ labels, const int32_t *__restrict__ sizes,
                                                            uint32_t np, unsigned long long *acc)
{
    __shared__ unsigned long long s_acc[SBD_NACC];
    const uint32_t tid = threadIdx.x, d = blockIdx.x * SBD_BLOCK + tid;
    if (tid < SBD_NACC) s_acc[tid] = 0ull;
    __syncthreads();
    const bool root = d < np && labels[d] == (int32_t)d;
    const uint32_t size = root ? (uint32_t)sizes[2u * (size_t)d] : 0u;
    const unsigned long long roots = __ballot(root), singles = __ballot(root && size == 1u);
    if (root) atomicMax(&s_acc[SBD_KEY], ((unsigned long long)size << 32) | (unsigned long long)(0xFFFFFFFFu - d));
    if (__lane_id() == 0u && roots) {
        atomicAdd(&s_acc[SBD_BODIES], (unsigned long long)__popcll(roots));
        if (singles) atomicAdd(&s_acc[SBD_SINGLES], (unsigned long long)__popcll(singles));
    }
    __syncthreads();
    if (tid < SBD_NACC && s_acc[tid]) {
        if (tid == SBD_KEY) atomicMax(&acc[tid], s_acc[tid]);
        else atomicAdd(&acc[tid], s_acc[tid]);
    }
}

__global__ __launch_bounds__(64) void k_bodies_counts(const unsigned long long *__restrict__ acc, long long *counts)
{
    if (threadIdx.x != 0u) return;
    const unsigned long long bodies = acc[SBD_BODIES], key = acc[SBD_KEY];
    counts[0] = (long long)bodies;
    counts[1] = bodies ? (long long)(key >> 32) : 0ll;
    counts[2] = (long long)acc[SBD_SINGLES];
    counts[3] = bodies ? (long long)(0xFFFFFFFFu - (uint32_t)key) : -1ll;
}

// ---------------------------------------------------------------- host side

static sb_status sbd_enqueue(sb_engine *e, const sb_bodies_options *o, void *labels, void *sizes, void *counts, bool host)
{
    if (!e) return SB_ERR_INVALID;
    const char *what = host ? "sb_bodies" : "sb_bodies_device";
    if (!labels && !sizes && !counts) SB_FAIL(e, SB_ERR_INVALID, "%s: no output asked for", what);
    if (((uintptr_t)labels & 3u) || ((uintptr_t)sizes & 3u)) SB_FAIL(e, SB_ERR_INVALID, "%s: labels and sizes must be 4-byte aligned", what);
    if ((uintptr_t)counts & 7u) SB_FAIL(e, SB_ERR_INVALID, "%s: counts must be 8-byte aligned", what);
    SB_TRY(sbq_preflight(e, what, o, "labelled", "bodies across ranks are not handled"));
    SB_TRY(sbq_need(e, "sb_bodies", SBQ_PARTICLES | SBQ_BEAMS));
    SbStateIoState &s = *e->sio;
    s.bod_build_ms = s.part_ms + s.beam_ms;

    // where the launches write: the caller's device memory, or the engine's own (what the caller did not ask for but a later
    // stage needs: up to the highest data index in use; sb_bodies: whole outputs, copied to the host by the mirror)
    const uint32_t maxP = e->opt.max_particles, np = s.np, n = s.nslots;
    const bool want_sizes = sizes || counts;
    const uint32_t n_parent = labels ? maxP : np, n_sizes = !want_sizes ? 0u : sizes ? maxP : np;
    SbqMirror mir(e, host);
    int32_t *d_parent = mir.out<int32_t>(SBD_B_PARENT, labels, (size_t)maxP * sizeof(int32_t));
    int32_t *d_sizes = mir.out<int32_t>(SBD_B_SIZES, sizes, (size_t)2 * maxP * sizeof(int32_t));
    if (!labels) {
        SB_TRY(s.buf[SBD_B_PARENT].grow(e, (size_t)n_parent * sizeof(int32_t)));
        d_parent = s.buf[SBD_B_PARENT].as<int32_t>();
    }
    if (want_sizes && !sizes) {
        SB_TRY(s.buf[SBD_B_SIZES].grow(e, (size_t)2 * n_sizes * sizeof(int32_t)));
        d_sizes = s.buf[SBD_B_SIZES].as<int32_t>();
    }
    unsigned long long *d_acc = nullptr;
    long long *d_counts = nullptr;
    if (counts) {
        SB_TRY(s.buf[SBD_B_ACC].grow(e, ((size_t)SBD_COUNTS + SB_BODY_WORDS) * sizeof(unsigned long long)));
        d_acc = s.buf[SBD_B_ACC].as<unsigned long long>();
        d_counts = mir.out_at<long long>(counts, d_acc, SBD_COUNTS * sizeof(unsigned long long), SB_BODY_WORDS * sizeof(int64_t));
    }
    SB_TRY(mir.st);
    const uint32_t *d_pinv = s.buf[SBQ_B_PINV].as<uint32_t>(), *d_tab = s.buf[SBQ_B_TAB].as<uint32_t>(); // (three planes of the four are read)
    const uint32_t *dead = sbq_dead(e);
    auto blocks = [](uint32_t k) { return (k + SBD_BLOCK - 1u) / SBD_BLOCK; };

    k_bodies_init<<<std::max(blocks(std::max(n_parent, n_sizes)), 1u), SBD_BLOCK, 0, e->stream>>>(d_pinv, np, d_parent, n_parent,
                                                                                                  want_sizes ? d_sizes : nullptr, n_sizes, d_acc);
    if (n) k_bodies_union<<<blocks(n), SBD_BLOCK, 0, e->stream>>>(d_tab, n, dead, d_parent);
    if (np) {
        if (want_sizes) k_bodies_flatten<true><<<blocks(np), SBD_BLOCK, 0, e->stream>>>(d_parent, np, d_sizes);
        else k_bodies_flatten<false><<<blocks(np), SBD_BLOCK, 0, e->stream>>>(d_parent, np, nullptr);
    }
    if (want_sizes && n) k_bodies_beams<<<blocks(n), SBD_BLOCK, 0, e->stream>>>(d_tab, n, dead, d_parent, d_sizes);
    if (counts) {
        if (np) k_bodies_roots<<<blocks(np), SBD_BLOCK, 0, e->stream>>>(d_parent, d_sizes, np, d_acc);
        k_bodies_counts<<<1, 64, 0, e->stream>>>(d_acc, d_counts);
    }
    SB_HIP(e, hipGetLastError());
    return mir.finish();
}

// what sb_get_info reads ("bodies_table_build_us", "bodies_kernel_vgprs", "bodies_kernel_scratch_bytes")
bool sbd_info(sb_engine *e, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "bodies_table_build_us") *value = e->sio ? (uint64_t)(e->sio->bod_build_ms * 1000.0 + 0.5) : 0u;
    else if (k == "bodies_kernel_vgprs" || k == "bodies_kernel_scratch_bytes") { // the most over every kernel a call may launch
        const std::vector<const void *> ks = {(const void *)k_bodies_init, (const void *)k_bodies_union, (const void *)k_bodies_flatten<true>,
                            (const void *)k_bodies_flatten<false>, (const void *)k_bodies_beams, (const void *)k_bodies_roots,
                            (const void *)k_bodies_counts};
        return sbq_kernel_most(e, ks, k == "bodies_kernel_vgprs", value);
    }
    else return false;
    return true;
}

extern "C" {

sb_status sb_bodies_device(sb_engine *e, const sb_bodies_options *opts, void *device_labels_i32, void *device_sizes_i32,
                           void *device_counts_i64)
{
    SB_GUARDED(e, sbd_enqueue(e, opts, device_labels_i32, device_sizes_i32, device_counts_i64, false))
}

sb_status sb_bodies(sb_engine *e, const sb_bodies_options *opts, int32_t *labels, int32_t *sizes, int64_t *counts)
{
    SB_GUARDED(e, sbd_enqueue(e, opts, labels, sizes, counts, true))
}

} // extern "C"
