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
#include <atomic>
#include <chrono>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "sb_engine.h"

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
    const uint32_t lane = __lane_id();
    const int32_t left = __shfl_up(l, 1);
    const bool head = lane == 0u || left != l;
    const unsigned long long heads = __ballot(head);
    if (head && l >= 0) {
        const unsigned long long rest = lane == 63u ? 0ull : heads >> (lane + 1u);
        const uint32_t run = rest ? (uint32_t)__ffsll(rest) : 64u - lane; // up to the next head, or to the end of the wave
        atomicAdd(&sizes[2u * (size_t)l + col], (int)run);
    }
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

template <class T>
static sb_status sbd_grow(sb_engine *e, T **p, size_t &cap, size_t n)
{
    n = std::max<size_t>(n, 1);
    if (*p && cap >= n) return SB_OK;
    if (*p) {
        SB_HIP(e, hipStreamSynchronize(e->stream)); // a call in flight may still use it
        SB_HIP(e, hipFree(*p));
        *p = nullptr;
        cap = 0;
    }
    SB_HIP(e, hipMalloc((void **)p, n * sizeof(T)));
    cap = n;
    return SB_OK;
}

// data index -> internal particle (e->h_pidx inverted) up to the highest data index in use, and per caller beam slot of the latest
// upload {data index of A, data index of B, engine slot} as three planes.  Every endpoint is checked here to name a data index
// at which a particle lives: the kernels index parent[] with it.
static sb_status sbd_build_tables(sb_engine *e)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (!e->sio) e->sio = new SbStateIoState();
    SbStateIoState &s = *e->sio;
    const uint32_t P = e->P, maxP = e->opt.max_particles, Bu = sb_user_beams(e);
    if (e->h_pidx.size() != P || e->h_beams.size() != e->B) SB_FAIL(e, SB_ERR_STATE, "sb_bodies: host shadows of the scene are inconsistent");
    uint32_t np = 0;
    for (uint32_t i = 0; i < P; i++) np = std::max(np, e->h_pidx[i] + 1u);
    if (np > maxP) SB_FAIL(e, SB_ERR_STATE, "sb_bodies: particle data index outside the scene");
    std::vector<uint32_t> inv(std::max<uint32_t>(np, 1), SBD_NONE);
    for (uint32_t i = 0; i < P; i++) inv[e->h_pidx[i]] = i;
    const size_t n = std::max<uint32_t>(Bu, 1);
    std::vector<uint32_t> tab(3 * n, 0u);
    std::atomic<uint32_t> bad{0u};
    const uint32_t B = e->B;
    sbt::parallel_ranges(Bu, 1 << 16, [&](size_t u0, size_t u1) {
        for (size_t u = u0; u < u1; u++) {
            const uint32_t slot = sb_user_slot(e, u);
            if (slot >= B) {
                bad.store(1u, std::memory_order_relaxed);
                continue;
            }
            const SbHostBeam &h = e->h_beams[slot];
            if (h.da >= np || h.db >= np || inv[h.da] == SBD_NONE || inv[h.db] == SBD_NONE) {
                bad.store(1u, std::memory_order_relaxed);
                continue;
            }
            tab[u] = h.da, tab[n + u] = h.db, tab[2 * n + u] = slot;
        }
    });
    if (bad.load()) SB_FAIL(e, SB_ERR_STATE, "sb_bodies: beam slot or endpoint outside the scene");
    SB_TRY(sbd_grow(e, &s.d_bod_pinv, s.cap_bod_pinv, inv.size()));
    SB_TRY(sbd_grow(e, &s.d_bod_tab, s.cap_bod_tab, tab.size()));
    SB_HIP(e, hipMemcpyAsync(s.d_bod_pinv, inv.data(), inv.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    SB_HIP(e, hipMemcpyAsync(s.d_bod_tab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    SB_HIP(e, hipStreamSynchronize(e->stream)); // (the host vectors go out of scope)
    s.bod_np = np;
    s.bod_nslots = Bu;
    s.bod_valid = true;
    s.bod_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SB_OK;
}

static sb_status sbd_enqueue(sb_engine *e, const sb_bodies_options *o, void *labels, void *sizes, void *counts, bool host)
{
    if (!e) return SB_ERR_INVALID;
    const char *what = host ? "sb_bodies" : "sb_bodies_device";
    if (!labels && !sizes && !counts) SB_FAIL(e, SB_ERR_INVALID, "%s: no output asked for", what);
    if (((uintptr_t)labels & 3u) || ((uintptr_t)sizes & 3u)) SB_FAIL(e, SB_ERR_INVALID, "%s: labels and sizes must be 4-byte aligned", what);
    if ((uintptr_t)counts & 7u) SB_FAIL(e, SB_ERR_INVALID, "%s: counts must be 8-byte aligned", what);
    if (o && o->struct_size != 0 && o->struct_size != sizeof(sb_bodies_options))
        SB_FAIL(e, SB_ERR_INVALID, "%s: sb_bodies_options.struct_size %u != %zu", what, o->struct_size, sizeof(sb_bodies_options));
    if (o && o->struct_size)
        for (uint32_t r : o->reserved)
            if (r) SB_FAIL(e, SB_ERR_INVALID, "%s: reserved option words must be zero", what);
    if (e->opt.max_particles > 0x80000000u || e->opt.max_beams > 0x80000000u)
        SB_FAIL(e, SB_ERR_INVALID, "%s: capacities above 2^31 are not labelled", what);
    if (!e->loaded) SB_FAIL(e, SB_ERR_STATE, "%s before sb_write_buffers", what);
    if (e->halo_configured || e->n_ghost_p || e->n_send_p || e->n_ghost_b || e->n_send_b || e->n_peers || e->mailbox)
        SB_FAIL(e, SB_ERR_UNSUPPORTED, "%s: the engine has ghost zones or peers configured (bodies across ranks are not handled)", what);
    SB_HIP(e, hipSetDevice(e->device));
    if (!e->sio || !e->sio->bod_valid) SB_TRY(sbd_build_tables(e));
    SbStateIoState &s = *e->sio;

    // where the launches write: the caller's device memory, or the engine's own (what the caller did not ask for but a later
    // stage needs: up to the highest data index in use; sb_bodies: whole outputs, copied to the host below)
    const uint32_t maxP = e->opt.max_particles, np = s.bod_np, n = s.bod_nslots;
    const bool want_sizes = sizes || counts;
    const uint32_t n_parent = labels ? maxP : np, n_sizes = !want_sizes ? 0u : sizes ? maxP : np;
    int32_t *d_parent = (int32_t *)labels, *d_sizes = (int32_t *)sizes;
    long long *d_counts = (long long *)counts;
    if (host || !labels) {
        SB_TRY(sbd_grow(e, &s.d_bod_parent, s.cap_bod_parent, (size_t)n_parent));
        d_parent = s.d_bod_parent;
    }
    if (want_sizes && (host || !sizes)) {
        SB_TRY(sbd_grow(e, &s.d_bod_sizes, s.cap_bod_sizes, (size_t)2 * n_sizes));
        d_sizes = s.d_bod_sizes;
    }
    if (counts) {
        SB_TRY(sbd_grow(e, &s.d_bod_acc, s.cap_bod_acc, (size_t)SBD_COUNTS + SB_BODY_WORDS));
        if (host) d_counts = (long long *)(s.d_bod_acc + SBD_COUNTS);
    }
    unsigned long long *d_acc = counts ? s.d_bod_acc : nullptr;
    const uint32_t *dead = e->B && e->delete_gen ? e->d_dead_gen : nullptr; // as sb_load_buffers (fetch_dead) sees it
    auto blocks = [](uint32_t k) { return (k + SBD_BLOCK - 1u) / SBD_BLOCK; };

    k_bodies_init<<<std::max(blocks(std::max(n_parent, n_sizes)), 1u), SBD_BLOCK, 0, e->stream>>>(s.d_bod_pinv, np, d_parent, n_parent,
                                                                                                  want_sizes ? d_sizes : nullptr, n_sizes, d_acc);
    if (n) k_bodies_union<<<blocks(n), SBD_BLOCK, 0, e->stream>>>(s.d_bod_tab, n, dead, d_parent);
    if (np) {
        if (want_sizes) k_bodies_flatten<true><<<blocks(np), SBD_BLOCK, 0, e->stream>>>(d_parent, np, d_sizes);
        else k_bodies_flatten<false><<<blocks(np), SBD_BLOCK, 0, e->stream>>>(d_parent, np, nullptr);
    }
    if (want_sizes && n) k_bodies_beams<<<blocks(n), SBD_BLOCK, 0, e->stream>>>(s.d_bod_tab, n, dead, d_parent, d_sizes);
    if (counts) {
        if (np) k_bodies_roots<<<blocks(np), SBD_BLOCK, 0, e->stream>>>(d_parent, d_sizes, np, d_acc);
        k_bodies_counts<<<1, 64, 0, e->stream>>>(d_acc, d_counts);
    }
    SB_HIP(e, hipGetLastError());
    if (host) {
        if (labels) SB_HIP(e, hipMemcpyAsync(labels, d_parent, (size_t)maxP * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        if (sizes) SB_HIP(e, hipMemcpyAsync(sizes, d_sizes, (size_t)maxP * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        if (counts) SB_HIP(e, hipMemcpyAsync(counts, d_counts, SB_BODY_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
        SB_HIP(e, hipStreamSynchronize(e->stream));
    }
    return SB_OK;
}

// what sb_get_info reads ("bodies_table_build_us", "bodies_kernel_vgprs", "bodies_kernel_scratch_bytes")
bool sbd_info(sb_engine *e, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "bodies_table_build_us") *value = e->sio ? (uint64_t)(e->sio->bod_build_ms * 1000.0 + 0.5) : 0u;
    else if (k == "bodies_kernel_vgprs" || k == "bodies_kernel_scratch_bytes") { // the most over every kernel a call may launch
        const void *ks[] = {(const void *)k_bodies_init, (const void *)k_bodies_union, (const void *)k_bodies_flatten<true>,
                            (const void *)k_bodies_flatten<false>, (const void *)k_bodies_beams, (const void *)k_bodies_roots,
                            (const void *)k_bodies_counts};
        uint64_t most = 0;
        for (const void *f : ks) {
            hipFuncAttributes fa{};
            if (hipSetDevice(e->device) != hipSuccess || hipFuncGetAttributes(&fa, f) != hipSuccess) {
                (void)hipGetLastError();
                return false;
            }
            most = std::max<uint64_t>(most, k == "bodies_kernel_vgprs" ? (uint64_t)fa.numRegs : (uint64_t)fa.localSizeBytes);
        }
        *value = most;
    }
    else return false;
    return true;
}

#define SBD_GUARDED(e, call)                                                   \
    try {                                                                      \
        return (call);                                                         \
    } catch (const std::bad_alloc &) {                                         \
        if (e) (e)->err = "out of host memory";                                \
        return SB_ERR_OOM;                                                     \
    } catch (const std::exception &ex) {                                       \
        if (e) (e)->err = std::string("internal error: ") + ex.what();         \
        return SB_ERR_INVALID;                                                 \
    }

extern "C" {

sb_status sb_bodies_device(sb_engine *e, const sb_bodies_options *opts, void *device_labels_i32, void *device_sizes_i32,
                           void *device_counts_i64)
{
    SBD_GUARDED(e, sbd_enqueue(e, opts, device_labels_i32, device_sizes_i32, device_counts_i64, false))
}

sb_status sb_bodies(sb_engine *e, const sb_bodies_options *opts, int32_t *labels, int32_t *sizes, int64_t *counts)
{
    SBD_GUARDED(e, sbd_enqueue(e, opts, labels, sizes, counts, true))
}

} // extern "C"
