// sb_batch.hip -- N independent SMALL scenes, one workgroup per scene, one launch per frame (gfx950, wave64).
//
// sb_engine spreads ONE scene over the chip and pays a launch per substep (or per few): a scene of the reference's own size
// (119 particles / 299 beams by default, 2 500 at most in its box) uses a fraction of one CU and its frame costs what 64
// dependent launches cost.  Here a scene lives in the LDS and registers of ONE workgroup for a whole frame:
//
//   load    particles in SLOT order (internal index == slot, as on the atomic path), the data index per slot (the tie-break of
//           compute.wgsl:153 compares DATA indices), beams in beam-slot order, material rows
//   substep beam phase: every live beam slot from the READ positions through sb_beam_eval, ds_add of the i32 forces, break
//           flags as bits per beam slot; barrier; particle phase: the reference's loop over slots 0 .. P-1 in ascending order
//           against the frozen positions / velocities (every lane reads the same LDS word: a broadcast), sb_collide_pair_at,
//           sb_particle_finish with the consumed and cleared sum, new state into the WRITE half of the ping-pong; barrier
//   cells   (COLLIDE = SB_BATCH_CELLS, scenes of at least cell_min_p particles) beside the beam phase every particle's thread
//           puts its slot into the cell of its READ position: G x G fixed-capacity buckets in LDS, placed by ds_add on the cell's
//           count.  The particle phase then visits the 3 x 3 cells around its own and applies the contacts it finds in ascending
//           slot order (SB_SELECT_INSERT, the selection of sb_collide_grid): the walk's bits.  A full bucket sets a word that
//           sends the WHOLE workgroup through the walk for that substep.
//   delete  flagged beams leave the slot list by forward stable compaction (sbo_delete / SURVEY A7), counts updated, flags cleared
//   store   once per launch
//
// The arithmetic is sb_physics.h's, called, not restated: the bits are those of k_beams_atomic + k_particles<ALLPAIRS>.
// Forces are integer sums (order-free), so nothing here depends on how beams are dealt to lanes.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sb_batch.h"
#include "sb_scene_codec.h"

// ---------------------------------------------------------------- the frame kernel
// One thread per particle slot (blockDim.x >= max_particles: chosen at create), beams dealt round-robin.
// COLLIDE: SB_BATCH_NO_CONTACTS, SB_BATCH_WALK (the collision loop) or SB_BATCH_CELLS (the cell grid and the loop).
// MAT_LDS: the material rows fit the LDS beside the rest (else they are read from the constant blob every substep: L2 hits).
template <int COLLIDE, bool MAT_LDS>
__global__ __launch_bounds__(1024) void k_batch_frame(SbBatchView V, SbParams prm, uint32_t n_sub, uint32_t do_delete)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sbb_lds[];
    const uint32_t scene = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    uint32_t *meta = V.meta + (size_t)scene * SB_BM_WORDS;
    // (metadata words are rewritten between launches by other kernels: read at agent scope, never through the scalar cache)
    const uint32_t P = sbb_uniform(SB_AGENT_LOAD(&meta[SB_BM_P])), Bc = sbb_uniform(SB_AGENT_LOAD(&meta[SB_BM_B]));
    if (P == 0u || P > V.maxP || Bc > V.maxB) return; // an empty (or never uploaded) scene; counts are validated at upload
    const uint32_t maxP = V.maxP, maxB = V.maxB;

    // LDS map (sb_batch_lds_bytes mirrors it)
    float2 *s_pos = (float2 *)sbb_lds;       // [2][maxP] ping-pong
    float2 *s_vel = s_pos + 2u * maxP;       // [2][maxP]
    float2 *s_tl = s_vel + 2u * maxP;        // [maxB] {target_length, last_length} per beam slot
    int *s_f = (int *)(s_tl + maxB);         // [maxP][2] fixed-point force sums (compute.wgsl:68-69)
    uint32_t *s_pidx = (uint32_t *)(s_f + 2u * maxP); // [maxP] data index per slot
    uint32_t *s_w = s_pidx + maxP;           // [maxB] endpoint slots
    uint32_t *s_bd = s_w + maxB;             // [maxB] data index per beam slot
    uint32_t *s_flags = s_bd + maxB;         // [nflagw] break flags
    uint32_t *s_off = s_flags + V.nflagw;    // [nflagw + 1] delete pass: live beams in front of each flag word
    float *s_mat = (float *)(s_off + V.nflagw + 1u); // [maxB][6] (MAT_LDS)
    // contact cells (sb_batch_cell_lds_bytes mirrors them): the counts are double buffered by substep parity, so a substep
    // fills one buffer while every thread empties the word it filled in the other: no pass over G^2 words, no barrier of its own
    const bool cells = COLLIDE == SB_BATCH_CELLS && P >= V.cell_min_p; // workgroup-uniform
    const uint32_t G = V.cell_g, cntw = sb_bucket_count_words(G);
    uint16_t *s_cent = (uint16_t *)(sbb_lds + V.cell_off);               // [G * G][SB_BATCH_CELL_K] slots
    uint32_t *s_ccnt = (uint32_t *)(s_cent + G * G * SB_BATCH_CELL_K);   // [2][cntw] two 16-bit counts to a word
    uint32_t *s_covf = s_ccnt + 2u * cntw;                               // [2] "a cell was full"

    const unsigned char *cst = V.cst + (size_t)scene * V.cst_bytes;
    unsigned char *st = V.st + (size_t)scene * V.st_bytes;
    const uint32_t *g_pmap = (const uint32_t *)(cst + V.o_pmap);
    const uint32_t *g_bword = (const uint32_t *)(cst + V.o_bword);
    const float *g_bmat = (const float *)(cst + V.o_bmat);
    float2 *g_part = (float2 *)(st + V.o_part);
    float4 *g_bstate = (float4 *)(st + V.o_bstate);
    uint32_t *g_bmap = (uint32_t *)(st + V.o_bmap);
    uint32_t *g_bflags = (uint32_t *)(st + V.o_bflags);
    unsigned char *g_balive = st + V.o_balive;

    // the scene's constants: uniform, kept in scalar registers
    SbConsts c;
    {
        uint32_t w[16];
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = sbb_uniform(SB_AGENT_LOAD(&meta[SB_BM_CONSTS + k]));
        memcpy(&c, w, sizeof c);
    }
    const bool plain = c.drag_exp == 2.0f && c.mouse_active == 0u; // sb_particle_finish<PLAIN>: same bits, fewer branches

    // ---- load
    const bool active = tid < P;
    SbParticle q;
    q.p = q.v = q.a = make_float2(0.f, 0.f);
    uint32_t my_idx = 0u;
    if (active) {
        my_idx = g_pmap[tid];
        q.p = g_part[3u * my_idx];
        q.v = g_part[3u * my_idx + 1u];
        q.a = g_part[3u * my_idx + 2u];
        s_pos[tid] = q.p;
        s_vel[tid] = q.v;
        s_f[2u * tid] = 0;
        s_f[2u * tid + 1u] = 0;
        s_pidx[tid] = my_idx;
    }
    for (uint32_t j = tid; j < Bc; j += T) {
        const uint32_t d = g_bmap[j];
        const float4 bs = g_bstate[d];
        s_bd[j] = d;
        s_w[j] = g_bword[d];
        s_tl[j] = make_float2(bs.x, bs.y);
        if (MAT_LDS) {
#pragma unroll
            for (uint32_t k = 0; k < SB_BATCH_MAT_ROW; k++) s_mat[SB_BATCH_MAT_ROW * j + k] = g_bmat[SB_BATCH_MAT_ROW * d + k];
        }
    }
    for (uint32_t w = tid; w < V.nflagw; w += T) s_flags[w] = g_bflags[w];
    if (COLLIDE == SB_BATCH_CELLS && cells)
        for (uint32_t w = tid; w < 2u * cntw + 2u; w += T) s_ccnt[w] = 0u; // (once per launch; the overflow words with them)
    __syncthreads();

    const float elasticity_coeff = sb_div(c.elasticity + 1.0f, 2.0f); // :143
    // Contact test of k_particles<SB_COLLIDE_ALLPAIRS>: dist = sqrt(d2) (IEEE), contact when dist == 0 or dist < 2r, the root
    // only taken under sb_touch_test's threshold (sb_contact_cells.h; the loops below keep dx, dy and dist for the pair)
    const SbTouchTest tt = sb_touch_test(prm.particle_radius);
    const float two_r = tt.two_r, thr = tt.thr;

    // ---- substeps
    uint32_t cur = 0u;
    uint32_t my_cx = 0u, my_cy = 0u;        // this particle's cell in the substep at hand
    uint32_t n_on_cells = 0u, n_fell_back = 0u; // substeps of this launch (uniform)
    for (uint32_t k = 0; k < n_sub; k++) {
        const bool aux = k + 1u == n_sub; // strain / stress are outputs only (:122-123): stored by the last substep of a launch
        const float2 *rp = s_pos + cur * maxP, *rv = s_vel + cur * maxP;
        float2 *wp = s_pos + (cur ^ 1u) * maxP, *wv = s_vel + (cur ^ 1u) * maxP;
        uint32_t *ccnt = s_ccnt + (k & 1u) * cntw;
        if (COLLIDE == SB_BATCH_CELLS && cells) {
            // bin the READ positions (q.p is rp[tid]).  The count word this thread filled in the substep before goes back to 0
            // first: nobody reads that buffer any more (everybody is past that substep's last barrier), and the buffer filled now
            // was emptied the same way one substep ago, a barrier in front of the adds below.
            if (active) {
                if (k != 0u) s_ccnt[((k & 1u) ^ 1u) * cntw + ((my_cy * G + my_cx) >> 1)] = 0u;
                my_cx = sb_grid_coord(q.p.x, 0.0f, V.cell, G); // monotone, clamped; NaN and -inf: cell 0, +inf: the last one
                my_cy = sb_grid_coord(q.p.y, 0.0f, V.cell, G);
                // (sb_bucket_push in this kernel's own words: through the helper the two arms of the branch change places; this way
                // the kernel's instructions are unchanged)
                const uint32_t cell = my_cy * G + my_cx, sh = (cell & 1u) << 4;
                const uint32_t n = (atomicAdd(&ccnt[cell >> 1], 1u << sh) >> sh) & 0xffffu; // (at most 1024 per cell: no carry)
                if (n < SB_BATCH_CELL_K) s_cent[cell * SB_BATCH_CELL_K + n] = (uint16_t)tid;
                else s_covf[k & 1u] = 1u;
            }
            if (tid == 0u && k != 0u) s_covf[(k & 1u) ^ 1u] = 0u;
        }
        // beam phase (compute.wgsl:96-131)
        for (uint32_t j = tid; j < Bc; j += T) {
            const uint32_t word = s_w[j], ia = word & 0xffffu, ib = word >> 16;
            const float2 tl = s_tl[j];
            const float *m = MAT_LDS ? &s_mat[SB_BATCH_MAT_ROW * j] : &g_bmat[SB_BATCH_MAT_ROW * s_bd[j]];
            const float length = m[0], spring = m[1], damp = m[2], yield = m[3], limit = m[4], inv_length = m[5];
            SbBeamResult r;
            if (aux) {
                r = sb_beam_eval<true>(rp[ia], rp[ib], length, inv_length, tl.x, tl.y, spring, damp, yield, limit);
                g_bstate[s_bd[j]] = make_float4(r.target_length, r.last_length, r.strain, r.stress);
            } else {
                r = sb_beam_eval<false>(rp[ia], rp[ib], length, inv_length, tl.x, tl.y, spring, damp, yield, limit);
            }
            s_tl[j] = make_float2(r.target_length, r.last_length);
            atomicAdd(&s_f[2u * ia], r.ax);
            atomicAdd(&s_f[2u * ia + 1u], r.ay);
            atomicAdd(&s_f[2u * ib], r.bx);
            atomicAdd(&s_f[2u * ib + 1u], r.by);
            if (r.broken) atomicOr(&s_flags[j >> 5], 1u << (j & 31u)); // mark_beam_deleted, :86-88,117
        }
        __syncthreads();
        // particle phase (compute.wgsl:134-202)
        bool walk = COLLIDE != SB_BATCH_NO_CONTACTS;
        if (COLLIDE == SB_BATCH_CELLS && cells) {
            walk = sbb_uniform(s_covf[k & 1u]) != 0u; // a cell was full: every thread of the workgroup takes the loop
            n_fell_back += walk ? 1u : 0u;
            n_on_cells += walk ? 0u : 1u;
        }
        if (active) {
            SbParticle particle = q;
            const SbParticle self = q; // :141
            if (COLLIDE != SB_BATCH_NO_CONTACTS && walk) {
                for (uint32_t o = 0; o < P; o++) { // :144-170, ascending slot order
                    const float2 op = rp[o];
                    const float dx = op.x - self.p.x, dy = op.y - self.p.y;
                    const float d2 = dx * dx + dy * dy;
                    if (d2 > thr) continue;
                    const float dist = sb_sqrt(d2); // sb_length(dx, dy)
                    if (o != tid && (dist == 0.0f || dist < two_r))
                        sb_collide_pair_at(prm, c.friction, elasticity_coeff, particle, self, my_idx, s_pidx[o], dx, dy, dist, rv[o]);
                }
            }
            if (COLLIDE == SB_BATCH_CELLS && !walk) {
                // The same loop restricted to the slots in the 3 x 3 cells around this particle's.  Cells are at least
                // 2r (1 + 1/64) wide and the coordinate map is monotone, so whoever the loop above would find in contact
                // (dist == 0 or dist < 2r) sits in one of them; everybody else is a no-op of that loop.  The contacts are
                // applied in ascending slot order: a sweep collects the four smallest slots above the last one applied
                // (the order of the entries inside a cell does not matter), then they are applied; a sweep that comes back
                // with fewer than four was the last.
                const SbCellWindow win(my_cx, my_cy, G);
                bool have_last = false;
                uint32_t last = 0u;
                for (;;) {
                    uint32_t bs[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, bi[4] = {0u, 0u, 0u, 0u};
                    for (uint32_t yy = win.y0; yy <= win.y1; yy++) {
                        for (uint32_t xx = win.x0; xx <= win.x1; xx++) {
                            const uint32_t cell = yy * G + xx;
                            const uint32_t n = sb_bucket_count(ccnt, cell); // <= SB_BATCH_CELL_K: no cell was full
                            const SbBucketWords ent = sb_bucket_load(s_cent, cell);
#pragma unroll
                            for (uint32_t j = 0; j < SB_BATCH_CELL_K; j++) {
                                const uint32_t o = sb_bucket_entry(ent, j);
                                if (j >= n || o == tid || (have_last && o <= last) || o >= bs[3]) continue;
                                const float2 op = rp[o];
                                const float dx = op.x - self.p.x, dy = op.y - self.p.y;
                                const float d2 = dx * dx + dy * dy;
                                if (d2 > thr) continue;
                                const float dist = sb_sqrt(d2);
                                if (dist == 0.0f || dist < two_r) {
                                    uint32_t slot = o, id = o; // (internal index == slot here)
                                    SB_SELECT_INSERT(4, bs, bi, slot, id)
                                }
                            }
                        }
                    }
                    bool full = true;
#pragma unroll
                    for (int s4 = 0; s4 < 4; s4++) {
                        if (bs[s4] == 0xFFFFFFFFu) {
                            full = false;
                        } else {
                            const uint32_t o = bi[s4];
                            const float2 op = rp[o];
                            const float dx = op.x - self.p.x, dy = op.y - self.p.y;
                            const float dist = sb_sqrt(dx * dx + dy * dy);
                            sb_collide_pair_at(prm, c.friction, elasticity_coeff, particle, self, my_idx, s_pidx[o], dx, dy, dist, rv[o]);
                            last = o;
                            have_last = true;
                        }
                    }
                    if (!full) break;
                }
            }
            const int fx = s_f[2u * tid], fy = s_f[2u * tid + 1u];
            s_f[2u * tid] = 0; // atomicExchange(..., 0), :184-185
            s_f[2u * tid + 1u] = 0;
            if (plain) sb_particle_finish<true>(prm, c, particle, fx, fy);
            else sb_particle_finish<false>(prm, c, particle, fx, fy);
            q = particle;
            wp[tid] = q.p;
            wv[tid] = q.v;
        }
        __syncthreads();
        cur ^= 1u;
    }

    if (COLLIDE == SB_BATCH_CELLS && tid == 0u) { // what the launch ran on, once per launch
        if (n_on_cells) (void)atomicAdd(&V.cell_stats[0], (unsigned long long)n_on_cells);
        if (n_fell_back) (void)atomicAdd(&V.cell_stats[1], (unsigned long long)n_fell_back);
    }
    // ---- store (beam state went out with the last substep)
    if (n_sub != 0u && active) {
        g_part[3u * my_idx] = q.p;
        g_part[3u * my_idx + 1u] = q.v;
        g_part[3u * my_idx + 2u] = q.a;
    }
    if (!do_delete) {
        if (n_sub != 0u)
            for (uint32_t w = tid; w < V.nflagw; w += T) g_bflags[w] = s_flags[w];
        return;
    }
    // ---- delete pass (compute.wgsl:205-246, canonical semantics: in-place forward stable compaction of the beam slots;
    // slots past the new count keep their stale entries, as the oracle's do)
    const uint32_t nw = (Bc + 31u) >> 5;
    if (tid == 0u) {
        uint32_t run = 0u;
        for (uint32_t w = 0; w < nw; w++) {
            const uint32_t valid = (w == nw - 1u && (Bc & 31u) != 0u) ? (1u << (Bc & 31u)) - 1u : 0xFFFFFFFFu;
            s_off[w] = run;
            run += __popc(~s_flags[w] & valid);
        }
        s_off[nw] = run;
    }
    __syncthreads();
    const uint32_t newc = s_off[nw];
    if (newc != Bc) {
        for (uint32_t j = tid; j < Bc; j += T) {
            const uint32_t w = j >> 5, bit = 1u << (j & 31u), fl = s_flags[w], d = s_bd[j];
            if (fl & bit) {
                g_balive[d] = 0;
            } else {
                const uint32_t np = s_off[w] + __popc(~fl & (bit - 1u));
                if (np != j) g_bmap[np] = d;
            }
        }
        if (tid == 0u) meta[SB_BM_B] = newc; // :238
    }
    for (uint32_t w = tid; w < V.nflagw; w += T) g_bflags[w] = 0u; // :241-244
}

// ---------------------------------------------------------------- helper kernels: plain copies
#define SBB_BLOCK 256

// one uploaded scene (staged in device memory) into scenes first .. first + count - 1: constant blob, state blob, reset blob, metadata
__global__ __launch_bounds__(SBB_BLOCK) void k_batch_replicate(SbBatchView V, const uint4 *__restrict__ stage_cst, const uint4 *__restrict__ stage_st,
                                                                const uint32_t *__restrict__ stage_meta, uint32_t first, uint32_t count)
{
    const uint32_t scene = first + blockIdx.x;
    if (blockIdx.x >= count || scene >= V.n_scenes) return;
    uint4 *c = (uint4 *)(V.cst + (size_t)scene * V.cst_bytes), *s = (uint4 *)(V.st + (size_t)scene * V.st_bytes);
    uint4 *r = (uint4 *)(V.rst + (size_t)scene * V.st_bytes);
    for (uint32_t i = threadIdx.x; i < V.cst_bytes / 16u; i += SBB_BLOCK) c[i] = stage_cst[i];
    for (uint32_t i = threadIdx.x; i < V.st_bytes / 16u; i += SBB_BLOCK) {
        const uint4 v = stage_st[i];
        s[i] = v;
        r[i] = v;
    }
    if (threadIdx.x < SB_BM_WORDS) V.meta[(size_t)scene * SB_BM_WORDS + threadIdx.x] = stage_meta[threadIdx.x];
}

__global__ __launch_bounds__(SBB_BLOCK) void k_batch_reset(SbBatchView V, const unsigned char *__restrict__ mask)
{
    const uint32_t scene = blockIdx.x;
    if (scene >= V.n_scenes) return;
    if (mask && mask[scene] == 0) return;
    uint32_t *meta = V.meta + (size_t)scene * SB_BM_WORDS;
    if (meta[SB_BM_LOADED] == 0u) return;
    // particles added since the reset state was made (sb_batch_add_particles_device) give their data indices back: the slots
    // P0 .. P - 1.  (Every thread has read P before thread 0 writes it: the barrier.)
    const uint32_t P = min(SB_AGENT_LOAD(&meta[SB_BM_P]), V.maxP), P0 = SB_AGENT_LOAD(&meta[SB_BM_P0]);
    __syncthreads();
    if (P > P0) {
        unsigned char *cst = V.cst + (size_t)scene * V.cst_bytes;
        const uint32_t *pmap = (const uint32_t *)(cst + V.o_pmap);
        for (uint32_t slot = P0 + threadIdx.x; slot < P; slot += SBB_BLOCK) {
            const uint32_t d = pmap[slot];
            if (d < V.maxP) (cst + V.o_pex)[d] = 0;
        }
    }
    uint4 *s = (uint4 *)(V.st + (size_t)scene * V.st_bytes);
    const uint4 *r = (const uint4 *)(V.rst + (size_t)scene * V.st_bytes);
    for (uint32_t i = threadIdx.x; i < V.st_bytes / 16u; i += SBB_BLOCK) s[i] = r[i];
    if (threadIdx.x == 0u) {
        meta[SB_BM_B] = meta[SB_BM_B0];
        if (P > P0) SB_AGENT_STORE(&meta[SB_BM_P], P0);
    }
}

struct SbBatchWords8 {
    uint32_t w[8];
};
// words [word0, word0 + 8) of the metadata of scenes first .. first + count - 1: from `src` (per scene, 8 words each) or `same`
__global__ __launch_bounds__(SBB_BLOCK) void k_batch_meta8(SbBatchView V, uint32_t first, uint32_t count, uint32_t word0,
                                                            const uint32_t *__restrict__ src, SbBatchWords8 same)
{
    const uint32_t t = blockIdx.x * SBB_BLOCK + threadIdx.x, s = t >> 3, k = t & 7u;
    if (s >= count || first + s >= V.n_scenes) return;
    V.meta[(size_t)(first + s) * SB_BM_WORDS + word0 + k] = src ? src[(size_t)(first + s) * 8u + k] : same.w[k];
}

__global__ __launch_bounds__(SBB_BLOCK) void k_batch_export(SbBatchView V, float *particles, float *beams, unsigned char *alive)
{
    const uint32_t scene = blockIdx.x;
    if (scene >= V.n_scenes) return;
    const unsigned char *cst = V.cst + (size_t)scene * V.cst_bytes, *st = V.st + (size_t)scene * V.st_bytes;
    const unsigned char *pex = cst + V.o_pex, *bex = cst + V.o_bex, *bal = st + V.o_balive;
    const float *part = (const float *)(st + V.o_part), *bstate = (const float *)(st + V.o_bstate);
    if (particles)
        for (uint32_t i = threadIdx.x; i < V.maxP * 6u; i += SBB_BLOCK)
            if (pex[i / 6u]) particles[(size_t)scene * V.maxP * 6u + i] = part[i];
    if (beams)
        for (uint32_t i = threadIdx.x; i < V.maxB * 4u; i += SBB_BLOCK)
            if (bex[i >> 2]) beams[(size_t)scene * V.maxB * 4u + i] = bstate[i];
    if (alive)
        for (uint32_t i = threadIdx.x; i < V.maxB; i += SBB_BLOCK)
            if (bex[i]) alive[(size_t)scene * V.maxB + i] = bal[i];
}

__global__ __launch_bounds__(SBB_BLOCK) void k_batch_import(SbBatchView V, const float *__restrict__ particles)
{
    const uint32_t scene = blockIdx.x;
    if (scene >= V.n_scenes) return;
    const unsigned char *pex = V.cst + (size_t)scene * V.cst_bytes + V.o_pex;
    float *part = (float *)(V.st + (size_t)scene * V.st_bytes + V.o_part);
    for (uint32_t i = threadIdx.x; i < V.maxP * 6u; i += SBB_BLOCK)
        if (pex[i / 6u]) part[i] = particles[(size_t)scene * V.maxP * 6u + i];
}

// ---------------------------------------------------------------- fork, checkpoint, beam import
// Blobs are copied by blockIdx.y's share of the workgroups of a scene: the blobs of the limit capacity are 100 KB and more.
static uint32_t sb_batch_copy_chunks(const SbBatchView &V) { return std::max(1u, cdivb(std::max(V.cst_bytes, V.st_bytes) / 16u, SBB_BLOCK * 4u)); }
SB_DEV void sbb_copy16(unsigned char *dst, const unsigned char *src, uint32_t bytes)
{
    for (uint32_t i = blockIdx.y * SBB_BLOCK + threadIdx.x; i < bytes / 16u; i += gridDim.y * SBB_BLOCK) ((uint4 *)dst)[i] = ((const uint4 *)src)[i];
}
// the scene that scene i becomes a copy of; SB_BATCH_FORK_KEEP: scene i stays (KEEP itself, i, or an entry that names no scene)
SB_DEV uint32_t sbb_fork_source(const uint32_t *__restrict__ src, uint32_t i, uint32_t n)
{
    const uint32_t s = src[i];
    return (s >= n || s == i) ? SB_BATCH_FORK_KEEP : s;
}
SB_DEV size_t sbb_fork_stride(const SbBatchView &V) { return (size_t)SB_BM_WORDS * 4u + V.cst_bytes + 2u * (size_t)V.st_bytes; }

// pass 1 only READS the batch: scene i's staging row gets the metadata words and the blobs of its source
__global__ __launch_bounds__(SBB_BLOCK) void k_batch_fork_gather(SbBatchView V, const uint32_t *__restrict__ src, unsigned char *stage,
                                                                  unsigned long long *bad, uint32_t flags)
{
    const uint32_t scene = blockIdx.x;
    if (scene >= V.n_scenes) return;
    const uint32_t raw = src[scene];
    if (raw >= V.n_scenes && raw != SB_BATCH_FORK_KEEP && blockIdx.y == 0u && threadIdx.x == 0u) (void)atomicAdd(bad, 1ull);
    const uint32_t s = sbb_fork_source(src, scene, V.n_scenes);
    if (s == SB_BATCH_FORK_KEEP) return;
    unsigned char *row = stage + (size_t)scene * sbb_fork_stride(V);
    if (blockIdx.y == 0u && threadIdx.x < SB_BM_WORDS) ((uint32_t *)row)[threadIdx.x] = V.meta[(size_t)s * SB_BM_WORDS + threadIdx.x];
    row += SB_BM_WORDS * 4u;
    sbb_copy16(row, V.cst + (size_t)s * V.cst_bytes, V.cst_bytes);
    sbb_copy16(row + V.cst_bytes, V.st + (size_t)s * V.st_bytes, V.st_bytes);
    if (!(flags & SB_BATCH_FORK_AS_RESET)) sbb_copy16(row + V.cst_bytes + V.st_bytes, V.rst + (size_t)s * V.st_bytes, V.st_bytes);
}

// pass 2 only WRITES it (and reads nothing of it that pass 2 writes): what describes the scene comes from the row, the user
// input stays, the physics constants stay unless asked for
__global__ __launch_bounds__(SBB_BLOCK) void k_batch_fork_scatter(SbBatchView V, const uint32_t *__restrict__ src, const unsigned char *stage,
                                                                   uint32_t flags)
{
    const uint32_t scene = blockIdx.x;
    if (scene >= V.n_scenes) return;
    if (sbb_fork_source(src, scene, V.n_scenes) == SB_BATCH_FORK_KEEP) return;
    const unsigned char *row = stage + (size_t)scene * sbb_fork_stride(V);
    const bool as_reset = (flags & SB_BATCH_FORK_AS_RESET) != 0u;
    if (blockIdx.y == 0u && threadIdx.x < SB_BM_WORDS) {
        const uint32_t k = threadIdx.x, *m = (const uint32_t *)row;
        uint32_t *meta = V.meta + (size_t)scene * SB_BM_WORDS;
        if (k < SB_BM_CONSTS || k == SB_BM_LOADED || ((flags & SB_BATCH_FORK_CONSTANTS) && k < SB_BM_CONSTS + 8u)) meta[k] = m[k];
        else if (k == SB_BM_B0) meta[k] = as_reset ? m[SB_BM_B] : m[SB_BM_B0];
        else if (k == SB_BM_P0) meta[k] = as_reset ? m[SB_BM_P] : m[SB_BM_P0];
    }
    row += SB_BM_WORDS * 4u;
    sbb_copy16(V.cst + (size_t)scene * V.cst_bytes, row, V.cst_bytes);
    sbb_copy16(V.st + (size_t)scene * V.st_bytes, row + V.cst_bytes, V.st_bytes);
    sbb_copy16(V.rst + (size_t)scene * V.st_bytes, row + V.cst_bytes + (as_reset ? 0u : V.st_bytes), V.st_bytes);
}

// k_batch_reset the other way round
__global__ __launch_bounds__(SBB_BLOCK) void k_batch_checkpoint(SbBatchView V, const unsigned char *__restrict__ mask)
{
    const uint32_t scene = blockIdx.x;
    if (scene >= V.n_scenes) return;
    if (mask && mask[scene] == 0) return;
    uint32_t *meta = V.meta + (size_t)scene * SB_BM_WORDS;
    if (meta[SB_BM_LOADED] == 0u) return;
    sbb_copy16(V.rst + (size_t)scene * V.st_bytes, V.st + (size_t)scene * V.st_bytes, V.st_bytes);
    if (blockIdx.y == 0u && threadIdx.x == 0u) meta[SB_BM_B0] = meta[SB_BM_B], meta[SB_BM_P0] = meta[SB_BM_P];
}

__global__ __launch_bounds__(SBB_BLOCK) void k_batch_import_beams(SbBatchView V, const float *__restrict__ beams, uint32_t fields)
{
    const uint32_t scene = blockIdx.x;
    if (scene >= V.n_scenes) return;
    const unsigned char *bex = V.cst + (size_t)scene * V.cst_bytes + V.o_bex;
    float *bstate = (float *)(V.st + (size_t)scene * V.st_bytes + V.o_bstate);
    const float *in = beams + (size_t)scene * V.maxB * 4u;
    for (uint32_t i = threadIdx.x; i < V.maxB; i += SBB_BLOCK) {
        if (!bex[i]) continue;
        if (fields & SB_BATCH_BEAM_TARGET_LENGTH) bstate[4u * i] = in[4u * i];
        if (fields & SB_BATCH_BEAM_LAST_LENGTH) bstate[4u * i + 1u] = in[4u * i + 1u];
    }
}

// ---------------------------------------------------------------- host
thread_local std::string g_batch_create_error;


// threads of a scene's workgroup: one per particle slot of the capacity, and enough that a lane evaluates at most four beams
// per substep; whole waves, 64 .. 1024
static uint32_t sb_batch_threads(uint32_t maxP, uint32_t maxB)
{
    const uint32_t t = std::max((maxP + 63u) / 64u * 64u, (cdivb(maxB, 4u) + 63u) / 64u * 64u);
    return std::min(std::max(t, 64u), 1024u);
}
// the LDS map of k_batch_frame
static uint32_t sb_batch_lds_bytes(uint32_t maxP, uint32_t maxB, bool mats)
{
    const uint32_t nflagw = cdivb(std::max(maxB, 1u), 32u);
    return up16(maxP * (16u + 16u + 8u + 4u) + maxB * (8u + 4u + 4u) + (2u * nflagw + 1u) * 4u + (mats ? maxB * SB_BATCH_MAT_ROW * 4u : 0u));
}
#define SB_BATCH_LDS_LIMIT (160u * 1024u) // one CU of gfx950

// ---- contact cells: geometry
// Scenes of at least this many particles take the cells when sb_batch_options.grid_min_particles is 0: the smallest size of the
// measured sweep (replicated lattices of 64 .. 1024 particles, profiles/batch_grid_timing.json) at which the cells win -- at 64
// and 128 the cap on G makes the cells so coarse that a lattice fills their buckets, and the default scene (119) is 1.96 ms on
// the walk against 2.45 ms on the cells.
#define SB_BATCH_GRID_MIN_PARTICLES_DEFAULT 256u
// (the rule that turns a radius, bounds and a capacity into cells: sb_batch_cell_cap / sb_batch_cell_geometry, sb_batch.h)

const char *sb_batch_last_error(const sb_batch *b) { return b ? b->err.c_str() : g_batch_create_error.c_str(); }

void sb_batch_default_options(sb_batch_options *o)
{
    memset(o, 0, sizeof *o);
    o->struct_size = sizeof *o;
    o->n_scenes = 1;
    o->bounds_size = 1000.0f;   // engineWorker.ts:39
    o->particle_radius = 10.0f; // engineWorker.ts:40
    o->subticks = 64;           // engineWorker.ts:41
    o->max_particles = SB_BATCH_MAX_PARTICLES;
    o->max_beams = SB_BATCH_MAX_BEAMS;
    o->layout = SB_LAYOUT_V1;
    o->collision_mode = SB_COLLIDE_GRID;
    o->device_ordinal = 0;
}

typedef void (*sb_batch_kernel)(SbBatchView, SbParams, uint32_t, uint32_t);
static sb_batch_kernel sb_batch_frame_kernel(const sb_batch *b)
{
    if (b->collide == SB_BATCH_CELLS) return b->mat_lds ? k_batch_frame<SB_BATCH_CELLS, true> : k_batch_frame<SB_BATCH_CELLS, false>;
    if (b->collide == SB_BATCH_WALK) return b->mat_lds ? k_batch_frame<SB_BATCH_WALK, true> : k_batch_frame<SB_BATCH_WALK, false>;
    return b->mat_lds ? k_batch_frame<SB_BATCH_NO_CONTACTS, true> : k_batch_frame<SB_BATCH_NO_CONTACTS, false>;
}

sb_status sb_batch_destroy(sb_batch *b)
{
    if (!b) return SB_ERR_INVALID;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    if (b->V.meta) (void)hipFree(b->V.meta);
    if (b->V.cst) (void)hipFree(b->V.cst);
    if (b->V.st) (void)hipFree(b->V.st);
    if (b->V.rst) (void)hipFree(b->V.rst);
    if (b->V.cell_stats) (void)hipFree(b->V.cell_stats);
    if (b->stage) (void)hipFree(b->stage);
    if (b->fork_stage) (void)hipFree(b->fork_stage);
    if (b->fork_bad) (void)hipFree(b->fork_bad);
    sbb_render_release(b);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
    return SB_OK;
}

sb_status sb_batch_create(const sb_batch_options *opts, sb_batch **out)
{
    sb_batch *none = nullptr;
    if (!opts || !out) SB_FAIL(none, SB_ERR_INVALID, "sb_batch_create: null argument");
    *out = nullptr;
    if (opts->struct_size != sizeof(sb_batch_options))
        SB_FAIL(none, SB_ERR_INVALID, "sb_batch_create: sb_batch_options.struct_size %u != %zu", opts->struct_size, sizeof(sb_batch_options));
    if (opts->n_scenes == 0) SB_FAIL(none, SB_ERR_INVALID, "sb_batch_create: n_scenes is 0");
    if (opts->layout != SB_LAYOUT_V1 && opts->layout != SB_LAYOUT_V2) SB_FAIL(none, SB_ERR_INVALID, "sb_batch_create: unknown layout %u", opts->layout);
    if (opts->layout == SB_LAYOUT_V1 && (opts->max_particles > 65536 || opts->max_beams > 65536))
        SB_FAIL(none, SB_ERR_INVALID, "sb_batch_create: v1 layout holds at most 65536 particles/beams (u16 indices)");
    if (opts->max_particles == 0) SB_FAIL(none, SB_ERR_INVALID, "sb_batch_create: max_particles is 0");
    if (opts->max_particles > SB_BATCH_MAX_PARTICLES)
        SB_FAIL(none, SB_ERR_INVALID, "sb_batch_create: max_particles %u per scene is above the limit of %u (what one workgroup holds)",
                 opts->max_particles, (unsigned)SB_BATCH_MAX_PARTICLES);
    if (opts->max_beams > SB_BATCH_MAX_BEAMS)
        SB_FAIL(none, SB_ERR_INVALID, "sb_batch_create: max_beams %u per scene is above the limit of %u (what one workgroup holds)",
                 opts->max_beams, (unsigned)SB_BATCH_MAX_BEAMS);
    if (opts->collision_mode > SB_COLLIDE_GRID) SB_FAIL(none, SB_ERR_INVALID, "sb_batch_create: unknown collision_mode %u", opts->collision_mode);
    if (!(opts->particle_radius > 0.f) || !(opts->bounds_size > 0.f) || opts->subticks == 0)
        SB_FAIL(none, SB_ERR_INVALID, "sb_batch_create: radius, bounds and subticks must be positive");
    if (opts->grid_min_particles > SB_BATCH_MAX_PARTICLES && opts->grid_min_particles != 0xFFFFFFFFu)
        SB_FAIL(none, SB_ERR_INVALID, "sb_batch_create: grid_min_particles %u is neither 0 (the default), 1 .. %u, nor 0xFFFFFFFF (never)",
                 opts->grid_min_particles, (unsigned)SB_BATCH_MAX_PARTICLES);
    int ndev = 0;
    hipError_t r = hipGetDeviceCount(&ndev);
    if (r != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        SB_FAIL(none, SB_ERR_NO_DEVICE, "no HIP device available (%s); a batch has no CPU fallback",
                 r == hipSuccess ? "device count 0" : hipGetErrorString(r));
    }
    if (opts->device_ordinal < 0 || opts->device_ordinal >= ndev)
        SB_FAIL(none, SB_ERR_NO_DEVICE, "device_ordinal %d out of range (%d devices)", opts->device_ordinal, ndev);

    sb_batch *b = new sb_batch();
    b->opt = *opts;
    b->device = opts->device_ordinal;
    b->subticks = (opts->subticks + 1) / 2 * 2; // engineWorker.ts:90
    b->prm.bounds_size = opts->bounds_size;
    b->prm.particle_radius = opts->particle_radius;
    b->prm.time_step = 1.0f / (float)b->subticks; // engineWorker.ts:331
    {
        // time_step^2 a power of two (any power-of-two subticks): x / dt^2 is the exact multiplication by its reciprocal,
        // resolved here once (SbParams::inv_dt2, as sb_create does)
        const float dt2 = b->prm.time_step * b->prm.time_step;
        uint32_t bits;
        memcpy(&bits, &dt2, 4);
        const bool pow2 = (bits & 0x007fffffu) == 0u && (bits >> 23) > 1u && (bits >> 23) < 253u;
        b->prm.inv_dt2 = pow2 ? 1.0f / dt2 : 0.0f;
    }
    const uint32_t maxP = opts->max_particles, maxB = opts->max_beams, n = opts->n_scenes;
    SbBatchView &V = b->V;
    // SB_COLLIDE_GRID: the cells, for scenes of at least grid_min_particles particles -- unless no scene of this capacity can
    // have that many, or the cell width is not an ordinary number: then the batch is the walk's, with the walk's LDS
    b->collide = opts->collision_mode == SB_COLLIDE_OFF ? SB_BATCH_NO_CONTACTS : SB_BATCH_WALK;
    b->grid_min_particles = opts->grid_min_particles ? opts->grid_min_particles : SB_BATCH_GRID_MIN_PARTICLES_DEFAULT;
    uint32_t cell_bytes = 0u;
    if (opts->collision_mode == SB_COLLIDE_GRID && b->grid_min_particles <= maxP) {
        float cell = 0.f;
        const uint32_t g = sb_batch_cell_geometry(opts->bounds_size, opts->particle_radius, sb_batch_cell_cap(maxP), &cell);
        if (g != 0u) {
            b->collide = SB_BATCH_CELLS;
            V.cell_g = g;
            V.cell = cell;
            V.cell_min_p = b->grid_min_particles;
            cell_bytes = up16(sb_batch_cell_lds_bytes(g));
        }
    }
    b->threads = sb_batch_threads(maxP, maxB);
    // (the material rows give way to the cells: with them in memory the LDS of the limit capacity still holds both)
    b->mat_lds = sb_batch_lds_bytes(maxP, maxB, true) + cell_bytes <= SB_BATCH_LDS_LIMIT;
    V.cell_off = sb_batch_lds_bytes(maxP, maxB, b->mat_lds);
    b->lds_bytes = V.cell_off + cell_bytes;

    V.maxP = maxP;
    V.maxB = maxB;
    V.n_scenes = n;
    V.nflagw = cdivb(std::max(maxB, 1u), 32u);
    uint32_t o = 0;
    V.o_pmap = o, o += up16(maxP * 4u);
    V.o_bword = o, o += up16(maxB * 4u);
    V.o_bmat = o, o += up16(maxB * SB_BATCH_MAT_ROW * 4u);
    V.o_pex = o, o += up16(maxP);
    V.o_bex = o, o += up16(maxB);
    V.cst_bytes = std::max(o, 16u);
    o = 0;
    V.o_part = o, o += up16(maxP * 24u);
    V.o_bstate = o, o += up16(maxB * 16u);
    V.o_bmap = o, o += up16(maxB * 4u);
    V.o_bflags = o, o += up16(V.nflagw * 4u);
    V.o_balive = o, o += up16(maxB);
    V.st_bytes = std::max(o, 16u);

#define SBB_CREATE_HIP(call)                                                                              \
    do {                                                                                                  \
        hipError_t _r = (call);                                                                           \
        if (_r != hipSuccess) {                                                                           \
            (void)hipGetLastError();                                                                      \
            g_batch_create_error = std::string(#call " failed: ") + hipGetErrorString(_r);                \
            (void)sb_batch_destroy(b);                                                                    \
            return _r == hipErrorOutOfMemory ? SB_ERR_OOM : SB_ERR_HIP;                                   \
        }                                                                                                 \
    } while (0)
    SBB_CREATE_HIP(hipSetDevice(b->device));
    SBB_CREATE_HIP(hipStreamCreate(&b->stream));
    SBB_CREATE_HIP(hipMalloc((void **)&V.meta, (size_t)n * SB_BM_WORDS * 4u));
    SBB_CREATE_HIP(hipMalloc((void **)&V.cst, (size_t)n * V.cst_bytes));
    SBB_CREATE_HIP(hipMalloc((void **)&V.st, (size_t)n * V.st_bytes));
    SBB_CREATE_HIP(hipMalloc((void **)&V.rst, (size_t)n * V.st_bytes));
    SBB_CREATE_HIP(hipMalloc((void **)&b->stage, (size_t)SB_BM_WORDS * 4u + V.cst_bytes + V.st_bytes));
    SBB_CREATE_HIP(hipMemsetAsync(V.meta, 0, (size_t)n * SB_BM_WORDS * 4u, b->stream));
    SBB_CREATE_HIP(hipMemsetAsync(V.cst, 0, (size_t)n * V.cst_bytes, b->stream));
    SBB_CREATE_HIP(hipMemsetAsync(V.st, 0, (size_t)n * V.st_bytes, b->stream));
    SBB_CREATE_HIP(hipMemsetAsync(V.rst, 0, (size_t)n * V.st_bytes, b->stream));
    if (b->collide == SB_BATCH_CELLS) {
        SBB_CREATE_HIP(hipMalloc((void **)&V.cell_stats, 2u * sizeof(unsigned long long)));
        SBB_CREATE_HIP(hipMemsetAsync(V.cell_stats, 0, 2u * sizeof(unsigned long long), b->stream));
    }
    const void *fn = (const void *)sb_batch_frame_kernel(b);
    SBB_CREATE_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b->lds_bytes));
    hipFuncAttributes fa{};
    SBB_CREATE_HIP(hipFuncGetAttributes(&fa, fn));
    b->vgprs = fa.numRegs;
    b->scratch = (int)fa.localSizeBytes;
    SBB_CREATE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&b->scenes_per_cu, fn, (int)b->threads, b->lds_bytes));
    SBB_CREATE_HIP(hipStreamSynchronize(b->stream));
#undef SBB_CREATE_HIP
    *out = b;
    return SB_OK;
}

// buffer presence and sizes against the batch's capacity per scene (sb_scene_codec.h); need_all: an upload
static sb_status check_sizes(sb_batch *b, const char *who, bool need_all, const void *metadata, size_t metadata_bytes, const void *mapping,
                             size_t mapping_bytes, const void *particles, size_t particles_bytes, const void *beams, size_t beams_bytes)
{
    const sbc::SizeError sz = sbc::check_sizes(b->opt.layout, b->opt.max_particles, b->opt.max_beams, need_all, metadata, metadata_bytes, mapping,
                                               mapping_bytes, particles, particles_bytes, beams, beams_bytes);
    if (sz.buffer == sbc::BUF_NULL) SB_FAIL(b, SB_ERR_INVALID, "%s: null buffer", who);
    if (sz.buffer) SB_FAIL(b, SB_ERR_INVALID, "%s: %s buffer is %zu bytes, need %zu", who, sbc::buffer_name(sz.buffer), sz.have, sz.need);
    return SB_OK;
}

sb_status sb_batch_write_scene(sb_batch *b, uint32_t first, uint32_t count, const void *metadata, size_t metadata_bytes, const void *mapping,
                               size_t mapping_bytes, const void *particles, size_t particles_bytes, const void *beams, size_t beams_bytes)
{
    if (!b) return SB_ERR_INVALID;
    const uint32_t maxP = b->opt.max_particles, maxB = b->opt.max_beams, layout = b->opt.layout;
    if (count == 0 || first >= b->opt.n_scenes || count > b->opt.n_scenes - first)
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_write_scene: scenes %u .. %u+%u are not all inside the batch of %u", first, first, count, b->opt.n_scenes);
    SB_TRY(check_sizes(b, "sb_batch_write_scene", true, metadata, metadata_bytes, mapping, mapping_bytes, particles, particles_bytes, beams, beams_bytes));
    const uint8_t *md = (const uint8_t *)metadata, *mp = (const uint8_t *)mapping, *pd = (const uint8_t *)particles, *bd = (const uint8_t *)beams;
    const sbc::Header hd(md);
    const uint32_t P = hd.P, B = hd.B;
    if (!hd.capacity_is(maxP, maxB))
        SB_FAIL(b, SB_ERR_INVALID, "metadata max_particles/max_beams (%u/%u) differ from the batch's capacity per scene (%u/%u)", hd.maxP, hd.maxB,
                maxP, maxB);
    if (!hd.counts_fit(maxP, maxB)) SB_FAIL(b, SB_ERR_INVALID, "metadata counts (%u/%u) exceed capacity (%u/%u)", P, B, maxP, maxB);

    const SbBatchView &V = b->V;
    std::vector<unsigned char> img((size_t)SB_BM_WORDS * 4u + V.cst_bytes + V.st_bytes, 0);
    uint32_t *meta = (uint32_t *)img.data();
    unsigned char *cst = img.data() + SB_BM_WORDS * 4u, *st = cst + V.cst_bytes;
    uint32_t *pmap = (uint32_t *)(cst + V.o_pmap), *bword = (uint32_t *)(cst + V.o_bword), *bmap = (uint32_t *)(st + V.o_bmap);
    float *bmat = (float *)(cst + V.o_bmat), *bstate = (float *)(st + V.o_bstate);
    unsigned char *pex = cst + V.o_pex, *bex = cst + V.o_bex, *balive = st + V.o_balive;
    memcpy(meta, md, SB_METADATA_BYTES);
    meta[SB_BM_B0] = B;
    meta[SB_BM_P0] = P;
    meta[SB_BM_LOADED] = 1u;
    for (uint32_t s = 0; s < maxP; s++) pmap[s] = sbc::map_get(layout, mp, s);
    for (uint32_t s = 0; s < maxB; s++) bmap[s] = sbc::map_get(layout, mp, (size_t)maxP + s);
    memcpy(st + V.o_part, pd, (size_t)maxP * SB_PARTICLE_STRIDE);
    // validate (sb_scene_codec.h) and fill the image's beam rows in the same walk
    std::vector<uint32_t> data_of_slot, slot_of;
    const sbc::Scene sc{layout, maxP, maxB, P, B, mp, bd};
    const sbc::SceneError bad = sbc::validate_scene(sc, data_of_slot, slot_of, [&](const sbc::BeamSlot &r) {
        float f[9]; // length, target_length, last_length, spring, damp, yield_strain, strain_break_limit, strain, stress
        memcpy(f, r.f9, sizeof f);
        bex[r.idx] = balive[r.idx] = 1;
        bword[r.idx] = r.a | (r.b << 16);
        float *m = bmat + (size_t)SB_BATCH_MAT_ROW * r.idx, *q = bstate + 4u * (size_t)r.idx;
        m[0] = f[0], m[1] = f[3], m[2] = f[4], m[3] = f[5], m[4] = f[6];
        m[5] = 1.0f / f[0]; // one IEEE divide per beam at upload (compute.wgsl:112 pinned as x * (1 / length))
        q[0] = f[1], q[1] = f[2], q[2] = f[7], q[3] = f[8];
    });
    switch (bad.kind) {
    case sbc::SCENE_OK: break;
    case sbc::PARTICLE_RANGE: SB_FAIL(b, SB_ERR_INVALID, "particle slot %u maps to data index %u >= max_particles", bad.slot, bad.idx);
    case sbc::PARTICLE_TWICE: SB_FAIL(b, SB_ERR_INVALID, "particle data index %u is mapped by two slots (%u and %u)", bad.idx, bad.a, bad.slot);
    case sbc::BEAM_RANGE: SB_FAIL(b, SB_ERR_INVALID, "beam slot %u maps to data index %u >= max_beams", bad.slot, bad.idx);
    case sbc::BEAM_TWICE: SB_FAIL(b, SB_ERR_INVALID, "beam data index %u is mapped by two slots", bad.idx);
    default:
        SB_FAIL(b, SB_ERR_INVALID, "beam slot %u (data index %u) references particle data index %u/%u that no particle slot maps to", bad.slot, bad.idx,
                bad.a, bad.b);
    }
    for (uint32_t idx : data_of_slot) pex[idx] = 1;
    SB_HIP(b, hipSetDevice(b->device));
    SB_HIP(b, hipMemcpyAsync(b->stage, img.data(), img.size(), hipMemcpyHostToDevice, b->stream));
    k_batch_replicate<<<count, SBB_BLOCK, 0, b->stream>>>(V, (const uint4 *)(b->stage + SB_BM_WORDS * 4u),
                                                          (const uint4 *)(b->stage + SB_BM_WORDS * 4u + V.cst_bytes), (const uint32_t *)b->stage, first,
                                                          count);
    const sb_status ls = check_launch(b, "sb_batch_write_scene");
    SB_HIP(b, hipStreamSynchronize(b->stream)); // copy semantics: `img` and the caller's buffers are free again
    return ls;
}

sb_status sb_batch_write_user_input(sb_batch *b, const void *bytes32)
{
    if (!b) return SB_ERR_INVALID;
    if (!bytes32) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_write_user_input: null buffer");
    SbBatchWords8 w;
    memcpy(w.w, bytes32, SB_USER_INPUT_BYTES);
    SB_HIP(b, hipSetDevice(b->device));
    const uint32_t n = b->opt.n_scenes;
    k_batch_meta8<<<cdivb(n * 8u, SBB_BLOCK), SBB_BLOCK, 0, b->stream>>>(b->V, 0u, n, SB_USER_INPUT_OFFSET / 4u, nullptr, w);
    return check_launch(b, "sb_batch_write_user_input");
}

sb_status sb_batch_write_user_input_device(sb_batch *b, const void *device_bytes)
{
    if (!b) return SB_ERR_INVALID;
    if (!device_bytes || ((uintptr_t)device_bytes & 3u)) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_write_user_input_device: null or misaligned device buffer");
    SB_HIP(b, hipSetDevice(b->device));
    const uint32_t n = b->opt.n_scenes;
    k_batch_meta8<<<cdivb(n * 8u, SBB_BLOCK), SBB_BLOCK, 0, b->stream>>>(b->V, 0u, n, SB_USER_INPUT_OFFSET / 4u, (const uint32_t *)device_bytes,
                                                                         SbBatchWords8{});
    return check_launch(b, "sb_batch_write_user_input_device");
}

sb_status sb_batch_set_physics_constants(sb_batch *b, uint32_t first, uint32_t count, const float c8[8])
{
    if (!b) return SB_ERR_INVALID;
    if (!c8) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_set_physics_constants: null buffer");
    if (count == 0 || first >= b->opt.n_scenes || count > b->opt.n_scenes - first)
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_set_physics_constants: scenes %u .. %u+%u are not all inside the batch of %u", first, first, count,
                 b->opt.n_scenes);
    SbBatchWords8 w;
    memcpy(w.w, c8, 32);
    SB_HIP(b, hipSetDevice(b->device));
    k_batch_meta8<<<cdivb(count * 8u, SBB_BLOCK), SBB_BLOCK, 0, b->stream>>>(b->V, first, count, SB_BM_CONSTS, nullptr, w);
    return check_launch(b, "sb_batch_set_physics_constants");
}

static sb_status launch_frame(sb_batch *b, uint32_t n_sub, uint32_t do_delete)
{
    hipLaunchKernelGGL(sb_batch_frame_kernel(b), dim3(b->opt.n_scenes), dim3(b->threads), b->lds_bytes, b->stream, b->V, b->prm, n_sub, do_delete);
    return check_launch(b, "sb_batch frame kernel");
}

sb_status sb_batch_frame(sb_batch *b, uint32_t n_frames)
{
    if (!b) return SB_ERR_INVALID;
    SB_HIP(b, hipSetDevice(b->device));
    for (uint32_t f = 0; f < n_frames; f++) { // engineWorker.ts:646-665
        const sb_status s = launch_frame(b, b->subticks, 1u);
        if (s != SB_OK) return s;
        b->frames_done++;
        b->substeps_done += b->subticks;
    }
    return SB_OK;
}

sb_status sb_batch_step(sb_batch *b, uint32_t n_substeps)
{
    if (!b) return SB_ERR_INVALID;
    if (n_substeps == 0) return SB_OK;
    SB_HIP(b, hipSetDevice(b->device));
    const sb_status s = launch_frame(b, n_substeps, 0u);
    if (s == SB_OK) b->substeps_done += n_substeps;
    return s;
}

sb_status sb_batch_delete_pass(sb_batch *b)
{
    if (!b) return SB_ERR_INVALID;
    SB_HIP(b, hipSetDevice(b->device));
    return launch_frame(b, 0u, 1u);
}

sb_status sb_batch_reset_device(sb_batch *b, const void *device_mask_u8)
{
    if (!b) return SB_ERR_INVALID;
    SB_HIP(b, hipSetDevice(b->device));
    k_batch_reset<<<b->opt.n_scenes, SBB_BLOCK, 0, b->stream>>>(b->V, (const unsigned char *)device_mask_u8);
    return check_launch(b, "sb_batch_reset_device");
}

sb_status sb_batch_read_state_device(sb_batch *b, void *device_particles, void *device_beams, void *device_beam_alive)
{
    if (!b) return SB_ERR_INVALID;
    if (((uintptr_t)device_particles & 3u) || ((uintptr_t)device_beams & 3u))
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_read_state_device: particle and beam buffers must be 4-byte aligned");
    if (!device_particles && !device_beams && !device_beam_alive) return SB_OK;
    SB_HIP(b, hipSetDevice(b->device));
    k_batch_export<<<b->opt.n_scenes, SBB_BLOCK, 0, b->stream>>>(b->V, (float *)device_particles, (float *)device_beams, (unsigned char *)device_beam_alive);
    return check_launch(b, "sb_batch_read_state_device");
}

sb_status sb_batch_write_particles_device(sb_batch *b, const void *device_particles)
{
    if (!b) return SB_ERR_INVALID;
    if (!device_particles || ((uintptr_t)device_particles & 3u))
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_write_particles_device: null or misaligned device buffer");
    SB_HIP(b, hipSetDevice(b->device));
    k_batch_import<<<b->opt.n_scenes, SBB_BLOCK, 0, b->stream>>>(b->V, (const float *)device_particles);
    return check_launch(b, "sb_batch_write_particles_device");
}

sb_status sb_batch_fork_device(sb_batch *b, const void *device_src_u32, uint32_t flags)
{
    if (!b) return SB_ERR_INVALID;
    if (!device_src_u32 || ((uintptr_t)device_src_u32 & 3u)) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_fork_device: null or misaligned device buffer");
    if (flags & ~(SB_BATCH_FORK_CONSTANTS | SB_BATCH_FORK_AS_RESET)) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_fork_device: unknown flags 0x%x", flags);
    const SbBatchView &V = b->V;
    const uint32_t n = b->opt.n_scenes;
    SB_HIP(b, hipSetDevice(b->device));
    if (!b->fork_stage) { // the staging blobs: once, kept
        const size_t bytes = (size_t)n * ((size_t)SB_BM_WORDS * 4u + V.cst_bytes + 2u * (size_t)V.st_bytes);
        unsigned char *stage = nullptr;
        unsigned long long *bad = nullptr;
        hipError_t r = hipMalloc((void **)&stage, bytes);
        if (r == hipSuccess && (r = hipMalloc((void **)&bad, sizeof *bad)) == hipSuccess) r = hipMemsetAsync(bad, 0, sizeof *bad, b->stream);
        if (r != hipSuccess) {
            (void)hipGetLastError();
            if (stage) (void)hipFree(stage);
            if (bad) (void)hipFree(bad);
            SB_FAIL(b, r == hipErrorOutOfMemory ? SB_ERR_OOM : SB_ERR_HIP, "sb_batch_fork_device: %zu bytes of staging: %s", bytes, hipGetErrorString(r));
        }
        b->fork_stage = stage;
        b->fork_bad = bad;
        b->fork_stage_bytes = bytes;
    }
    const dim3 grid(n, sb_batch_copy_chunks(V));
    k_batch_fork_gather<<<grid, SBB_BLOCK, 0, b->stream>>>(V, (const uint32_t *)device_src_u32, b->fork_stage, b->fork_bad, flags);
    SB_TRY(check_launch(b, "sb_batch_fork_device (gather)"));
    k_batch_fork_scatter<<<grid, SBB_BLOCK, 0, b->stream>>>(V, (const uint32_t *)device_src_u32, b->fork_stage, flags);
    return check_launch(b, "sb_batch_fork_device (scatter)");
}

sb_status sb_batch_checkpoint_device(sb_batch *b, const void *device_mask_u8)
{
    if (!b) return SB_ERR_INVALID;
    SB_HIP(b, hipSetDevice(b->device));
    k_batch_checkpoint<<<dim3(b->opt.n_scenes, sb_batch_copy_chunks(b->V)), SBB_BLOCK, 0, b->stream>>>(b->V, (const unsigned char *)device_mask_u8);
    return check_launch(b, "sb_batch_checkpoint_device");
}

sb_status sb_batch_write_beams_device(sb_batch *b, const void *device_beams, uint32_t fields)
{
    if (!b) return SB_ERR_INVALID;
    if (!device_beams || ((uintptr_t)device_beams & 3u)) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_write_beams_device: null or misaligned device buffer");
    if (fields == 0u || (fields & ~(SB_BATCH_BEAM_TARGET_LENGTH | SB_BATCH_BEAM_LAST_LENGTH)))
        SB_FAIL(b, SB_ERR_INVALID, "sb_batch_write_beams_device: fields 0x%x is not a mask of SB_BATCH_BEAM_TARGET_LENGTH / _LAST_LENGTH", fields);
    SB_HIP(b, hipSetDevice(b->device));
    k_batch_import_beams<<<b->opt.n_scenes, SBB_BLOCK, 0, b->stream>>>(b->V, (const float *)device_beams, fields);
    return check_launch(b, "sb_batch_write_beams_device");
}

sb_status sb_batch_load_scene(sb_batch *b, uint32_t scene, void *metadata, size_t metadata_bytes, void *mapping, size_t mapping_bytes, void *particles,
                              size_t particles_bytes, void *beams, size_t beams_bytes)
{
    if (!b) return SB_ERR_INVALID;
    if (scene >= b->opt.n_scenes) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_load_scene: scene %u is not inside the batch of %u", scene, b->opt.n_scenes);
    SB_TRY(check_sizes(b, "sb_batch_load_scene", false, metadata, metadata_bytes, mapping, mapping_bytes, particles, particles_bytes, beams, beams_bytes));
    const SbBatchView &V = b->V;
    const uint32_t maxP = V.maxP, maxB = V.maxB;
    SB_HIP(b, hipSetDevice(b->device));
    SB_HIP(b, hipStreamSynchronize(b->stream));
    uint32_t meta[SB_BM_WORDS];
    std::vector<unsigned char> cst(V.cst_bytes), st(V.st_bytes);
    SB_HIP(b, hipMemcpy(meta, V.meta + (size_t)scene * SB_BM_WORDS, sizeof meta, hipMemcpyDeviceToHost));
    if (meta[SB_BM_LOADED] == 0u) SB_FAIL(b, SB_ERR_STATE, "sb_batch_load_scene: scene %u was never uploaded", scene);
    SB_HIP(b, hipMemcpy(cst.data(), V.cst + (size_t)scene * V.cst_bytes, V.cst_bytes, hipMemcpyDeviceToHost));
    SB_HIP(b, hipMemcpy(st.data(), V.st + (size_t)scene * V.st_bytes, V.st_bytes, hipMemcpyDeviceToHost));
    const uint32_t *pmap = (const uint32_t *)(cst.data() + V.o_pmap), *bword = (const uint32_t *)(cst.data() + V.o_bword);
    const uint32_t *bmap = (const uint32_t *)(st.data() + V.o_bmap);
    const float *bmat = (const float *)(cst.data() + V.o_bmat), *bstate = (const float *)(st.data() + V.o_bstate);
    const unsigned char *bex = cst.data() + V.o_bex;
    const uint32_t P = meta[SB_BM_P];
    if (metadata) memcpy(metadata, meta, SB_METADATA_BYTES);
    if (mapping) {
        uint8_t *m = (uint8_t *)mapping;
        for (uint32_t s = 0; s < maxP; s++) sbc::map_set(b->opt.layout, m, s, pmap[s]);
        for (uint32_t s = 0; s < maxB; s++) sbc::map_set(b->opt.layout, m, (size_t)maxP + s, bmap[s]);
    }
    if (particles)
        for (uint32_t s = 0; s < P; s++)
            memcpy((uint8_t *)particles + (size_t)pmap[s] * SB_PARTICLE_STRIDE, st.data() + V.o_part + (size_t)pmap[s] * SB_PARTICLE_STRIDE, SB_PARTICLE_STRIDE);
    if (beams) {
        const uint32_t stride = sbc::beam_stride(b->opt.layout);
        for (uint32_t idx = 0; idx < maxB; idx++) { // every beam of the upload, removed ones with their last state
            if (!bex[idx]) continue;
            const uint32_t da = pmap[bword[idx] & 0xffffu], db = pmap[bword[idx] >> 16]; // (the batch's own endpoint word: slots)
            const float *m = bmat + (size_t)SB_BATCH_MAT_ROW * idx, *q = bstate + 4u * (size_t)idx;
            const float f[9] = {m[0], q[0], q[1], m[1], m[2], m[3], m[4], q[2], q[3]};
            sbc::encode_beam(b->opt.layout, (uint8_t *)beams + (size_t)idx * stride, da, db, f);
        }
    }
    return SB_OK;
}

sb_status sb_batch_sync(sb_batch *b)
{
    if (!b) return SB_ERR_INVALID;
    SB_HIP(b, hipSetDevice(b->device));
    SB_HIP(b, hipStreamSynchronize(b->stream));
    return SB_OK;
}

sb_status sb_batch_get_stream(sb_batch *b, void **hip_stream)
{
    if (!b) return SB_ERR_INVALID;
    if (!hip_stream) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_get_stream: null argument");
    *hip_stream = (void *)b->stream;
    return SB_OK;
}

sb_status sb_batch_get_info(sb_batch *b, const char *key, uint64_t *value)
{
    if (!b) return SB_ERR_INVALID;
    if (!key || !value) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_get_info: null argument");
    const std::string k(key);
    if (k == "n_scenes") *value = b->opt.n_scenes;
    else if (k == "scene_max_particles") *value = SB_BATCH_MAX_PARTICLES;
    else if (k == "scene_max_beams") *value = SB_BATCH_MAX_BEAMS;
    else if (k == "max_particles") *value = b->opt.max_particles;
    else if (k == "max_beams") *value = b->opt.max_beams;
    else if (k == "threads_per_scene") *value = b->threads;
    else if (k == "lds_bytes_per_scene") *value = b->lds_bytes;
    else if (k == "materials_in_lds") *value = b->mat_lds ? 1u : 0u;
    else if (k == "scenes_per_cu") *value = (uint64_t)std::max(b->scenes_per_cu, 0);
    else if (k == "frame_kernel_vgprs") *value = (uint64_t)std::max(b->vgprs, 0);
    else if (k == "frame_kernel_scratch_bytes") *value = (uint64_t)std::max(b->scratch, 0);
    else if (k == "frames_done") *value = b->frames_done;
    else if (k == "substeps_done") *value = b->substeps_done;
    else if (k == "contact_cells_per_side") *value = b->V.cell_g;
    else if (k == "contact_cell_capacity") *value = SB_BATCH_CELL_K;
    else if (k == "grid_min_particles") *value = b->grid_min_particles;
    else if (k == "cell_substeps" || k == "cell_overflow_substeps") {
        unsigned long long st[2] = {0ull, 0ull};
        if (b->V.cell_stats) {
            SB_HIP(b, hipSetDevice(b->device));
            SB_HIP(b, hipStreamSynchronize(b->stream));
            SB_HIP(b, hipMemcpy(st, b->V.cell_stats, sizeof st, hipMemcpyDeviceToHost));
        }
        *value = st[k == "cell_substeps" ? 0 : 1];
    }
    else if (k == "constant_blob_bytes") *value = b->V.cst_bytes;
    else if (k == "state_blob_bytes") *value = b->V.st_bytes;
    else if (k == "fork_staging_bytes") *value = b->fork_stage_bytes;
    else if (k == "fork_bad_sources") {
        unsigned long long bad = 0ull;
        if (b->fork_bad) {
            SB_HIP(b, hipSetDevice(b->device));
            SB_HIP(b, hipStreamSynchronize(b->stream));
            SB_HIP(b, hipMemcpy(&bad, b->fork_bad, sizeof bad, hipMemcpyDeviceToHost));
        }
        *value = bad;
    }
    else if (sbb_render_info(b, key, value)) return SB_OK;
    else if (sbb_summary_info(b, key, value)) return SB_OK;
    else if (sbb_bodies_info(b, key, value)) return SB_OK;
    else if (sbb_contacts_info(b, key, value)) return SB_OK;
    else if (sbb_body_summary_info(b, key, value)) return SB_OK;
    else if (sbb_cut_info(b, key, value)) return SB_OK;
    else if (sbb_add_info(b, key, value)) return SB_OK;
    else if (sbb_spawn_info(b, key, value)) return SB_OK;
    else if (sbb_graph_info(b, key, value)) return SB_OK;
    else if (sbb_raycast_info(b, key, value)) return SB_OK;
    else if (sbb_nearest_info(b, key, value)) return SB_OK;
    else if (sbb_forces_info(b, key, value)) return SB_OK;
    else if (sbb_pose_info(b, key, value)) return SB_OK;
    else SB_FAIL(b, SB_ERR_INVALID, "sb_batch_get_info: unknown key '%s'", key);
    return SB_OK;
}
