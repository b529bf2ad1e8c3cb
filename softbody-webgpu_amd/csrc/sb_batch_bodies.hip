// sb_batch_bodies.hip -- the connected bodies of every scene of a batch in ONE launch (gfx950, wave64).
//
// A body is a connected component of the graph whose nodes are the scene's particle slots 0 .. P-1 and whose edges are its live
// beam slots 0 .. B-1 (state blob: beam slot -> data index; constant blob: data index -> endpoint slots).  Its label is the
// smallest particle DATA index in it.  One workgroup per scene; the search never leaves LDS, uses integers only, and nothing is
// written but the three outputs.
//
// The search keeps a forest over the particles: lab[slot] is the data index of the slot's parent, initially its own, and only
// ever DEcreases, so a parent's data index is never above its child's and the forest has no cycle but the roots' self loops.
//   hook      every live edge whose endpoints carry different labels lowers the label of the ROOT of the larger one to the
//             smaller one (an LDS integer minimum); such an edge also raises the workgroup's "changed" word
//   compress  pointer jumping through the data index -> slot table, up to SBO_HOPS parents per pass, passes until every slot
//             points at a root
// and stops at the first hook pass that finds no such edge: every slot then points at a root, both ends of every edge at the same
// one, and the smallest data index of a component can only be its own root.  The result is defined by the graph alone, so the
// races inside a pass (a label read while another thread lowers it) change the number of passes, never the bits.
// Every pass ends in ONE barrier (sbo_any); its verdict is the same word for every thread, so the loops are workgroup-uniform.
#include <algorithm>
#include <string>

#include "sb_batch.h"

#define SBO_BLOCK 256u
#define SBO_HOPS 4u
#define SBO_NONE 0xFFFFFFFFu
enum { SBO_BODIES, SBO_SINGLES, SBO_BEST, SBO_FLAGS, SBO_NWORDS = SBO_FLAGS + 3 }; // LDS words behind the arrays

static_assert(SB_BATCH_MAX_PARTICLES <= 1024 && SB_BATCH_MAX_PARTICLES <= 0x10000, "the largest-body key holds 10 bits of label, an endpoint word 16 bits of slot");

// LDS of a workgroup: lab[maxP], slot[maxP], particles[maxP], beams[maxP], edge[maxB], SBO_NWORDS words
static inline uint32_t sbo_lds_bytes(uint32_t maxP, uint32_t maxB) { return (4u * maxP + maxB + SBO_NWORDS) * 4u; }

// "does `pred` hold for any thread?", with the one barrier of pass number `pass`.  Three flag words take turns: pass n raises word
// n % 3 in front of its barrier and reads it behind; thread 0 clears word (n + 1) % 3 in front of the same barrier -- its readers
// (pass n - 2) are all past barrier n - 1, its writers (pass n + 1) all behind barrier n.
SB_DEV bool sbo_any(uint32_t *s_flag, uint32_t &pass, bool pred)
{
    const uint32_t k = pass % 3u;
    if (threadIdx.x == 0u) s_flag[(pass + 1u) % 3u] = 0u;
    if (pred) s_flag[k] = 1u;
    __syncthreads();
    pass++;
    return sbb_uniform(s_flag[k]) != 0u;
}

__global__ __launch_bounds__(SBO_BLOCK) void k_batch_bodies(SbBatchView V, int32_t *__restrict__ labels, int32_t *__restrict__ sizes,
                                                            int32_t *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sbo_lds[];
    const uint32_t scene = blockIdx.x, tid = threadIdx.x;
    if (scene >= V.n_scenes) return;
    const uint32_t maxP = V.maxP, maxB = V.maxB;
    uint32_t *s_lab = sbo_lds;         // [maxP] per particle SLOT: data index of its parent
    uint32_t *s_slot = s_lab + maxP;   // [maxP] per particle DATA index: its slot, SBO_NONE where no particle lives
    uint32_t *s_np = s_slot + maxP;    // [maxP] per DATA index: particles of the body it labels
    uint32_t *s_nb = s_np + maxP;      // [maxP] per DATA index: live beams of the body it labels
    uint32_t *s_edge = s_nb + maxP;    // [maxB] per live beam SLOT: (slot of endpoint A) | (slot of endpoint B) << 16
    uint32_t *s_red = s_edge + maxB;   // [SBO_NWORDS]

    const SbbScene hd = sbb_scene(V, scene);
    const uint32_t P = hd.P, Bc = hd.Bc;
    const unsigned char *cst = hd.cst, *st = hd.st;
    const uint32_t *g_pmap = (const uint32_t *)(cst + V.o_pmap), *g_bword = (const uint32_t *)(cst + V.o_bword);
    const uint32_t *g_bmap = (const uint32_t *)(st + V.o_bmap);

    // ---- stage (an upload is refused unless its data indices are distinct and inside the capacity, its endpoints slots < P)
    for (uint32_t d = tid; d < maxP; d += SBO_BLOCK) s_slot[d] = SBO_NONE, s_np[d] = 0u, s_nb[d] = 0u;
    if (tid < SBO_NWORDS) s_red[tid] = 0u;
    __syncthreads();
    for (uint32_t s = tid; s < P; s += SBO_BLOCK) {
        const uint32_t d = g_pmap[s];
        s_lab[s] = d;
        s_slot[d] = s;
    }
    for (uint32_t j = tid; j < Bc; j += SBO_BLOCK) s_edge[j] = g_bword[g_bmap[j]];
    __syncthreads();

    // ---- hook and compress until a hook pass finds every edge inside one tree
    uint32_t *s_flag = s_red + SBO_FLAGS;
    uint32_t pass = 0u;
    for (;;) {
        bool differ = false;
        for (uint32_t j = tid; j < Bc; j += SBO_BLOCK) {
            const uint32_t w = s_edge[j], la = s_lab[w & 0xffffu], lb = s_lab[w >> 16];
            if (la != lb) { // (behind a compress both are roots; a stale read only costs a pass)
                differ = true;
                atomicMin(&s_lab[s_slot[max(la, lb)]], min(la, lb));
            }
        }
        if (!sbo_any(s_flag, pass, differ)) break;
        bool deeper;
        do {
            deeper = false;
            for (uint32_t s = tid; s < P; s += SBO_BLOCK) {
                const uint32_t was = s_lab[s];
                uint32_t l = was;
                bool root = false; // "l names a root": no pass of this loop changes a root's label
                for (uint32_t h = 0; h < SBO_HOPS; h++) {
                    const uint32_t up = s_lab[s_slot[l]];
                    if (up == l) {
                        root = true;
                        break;
                    }
                    l = up;
                }
                if (l != was) s_lab[s] = l;
                deeper |= !root;
            }
        } while (sbo_any(s_flag, pass, deeper));
    }

    // ---- particles and live beams per label (a beam belongs to the body of its endpoints: A's will do)
    for (uint32_t s = tid; s < P; s += SBO_BLOCK) atomicAdd(&s_np[s_lab[s]], 1u);
    for (uint32_t j = tid; j < Bc; j += SBO_BLOCK) atomicAdd(&s_nb[s_lab[s_edge[j] & 0xffffu]], 1u);
    __syncthreads();

    // ---- the rows, at data indices; the count words are order-free: two sums and a maximum of (particles, smallest label first)
    int32_t *lrow = labels ? labels + (size_t)scene * maxP : nullptr;
    int32_t *srow = sizes ? sizes + (size_t)scene * maxP * 2u : nullptr;
    uint32_t bodies = 0u, singles = 0u, best = 0u;
    for (uint32_t d = tid; d < maxP; d += SBO_BLOCK) {
        const uint32_t s = s_slot[d], np = s_np[d];
        if (lrow) lrow[d] = s == SBO_NONE ? -1 : (int32_t)s_lab[s];
        if (srow) srow[2u * d] = (int32_t)np, srow[2u * d + 1u] = (int32_t)s_nb[d]; // (4-byte alignment is all that is asked for)
        if (np) {
            bodies++;
            singles += np == 1u ? 1u : 0u;
            best = max(best, (np << 10) | (1023u - d));
        }
    }
    if (!counts) return; // (uniform)
    if (bodies) {
        atomicAdd(&s_red[SBO_BODIES], bodies);
        atomicMax(&s_red[SBO_BEST], best);
        if (singles) atomicAdd(&s_red[SBO_SINGLES], singles);
    }
    __syncthreads();
    if (tid != 0u) return;
    int32_t *c = counts + (size_t)scene * SB_BATCH_BODY_WORDS;
    const uint32_t key = s_red[SBO_BEST];
    c[0] = (int32_t)s_red[SBO_BODIES];
    c[1] = (int32_t)(key >> 10);
    c[2] = (int32_t)s_red[SBO_SINGLES];
    c[3] = key ? (int32_t)(1023u - (key & 1023u)) : -1;
}

// ---------------------------------------------------------------- host
bool sbb_bodies_info(sb_batch *b, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "body_words") *value = SB_BATCH_BODY_WORDS;
    else if (k == "bodies_lds_bytes") *value = sbo_lds_bytes(b->V.maxP, b->V.maxB);
    else return sbb_kernel_info(b, "bodies", (const void *)k_batch_bodies, b->bodies_res, key, value);
    return true;
}

sb_status sb_batch_bodies_device(sb_batch *b, void *device_labels_i32, void *device_sizes_i32, void *device_counts_i32)
{
    if (!b) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_bodies_device: null batch");
    if (!device_labels_i32 && !device_sizes_i32 && !device_counts_i32)
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_bodies_device: labels, sizes and counts are all null: nothing to write");
    if (sbb_misaligned4({device_labels_i32, device_sizes_i32, device_counts_i32}))
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_bodies_device: the device buffers must be 4-byte aligned");
    SB_HIP(b, hipSetDevice(b->device));
    const SbBatchView &V = b->V;
    k_batch_bodies<<<b->opt.n_scenes, SBO_BLOCK, sbo_lds_bytes(V.maxP, V.maxB), b->stream>>>(V, (int32_t *)device_labels_i32, (int32_t *)device_sizes_i32,
                                                                                         (int32_t *)device_counts_i32);
    return check_launch(b, "sb_batch_bodies_device");
}
