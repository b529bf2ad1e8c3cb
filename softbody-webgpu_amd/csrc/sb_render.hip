// sb_render.hip -- pictures of the state (sb_render / sb_render_device of include/softbody.h) for gfx950 (CDNA4, wave64).
//
// The picture is host/render.js's renderPPM of what sb_load_buffers would return, byte for byte.  render.js
// draws particle slots 0 .. P-1, then beam slots 0 .. B-1 over them, and a pixel shows the last primitive that `put` it.
// Here every put is an atomicMax of a 64-bit key that orders the primitives as render.js draws them:
//     0                                   black
//     1 << 62 | particle slot << 1 | ring  (ring = 1: white, 0: inner colour; a slot puts a pixel at most once)
//     2 << 62 | engine beam slot          (strictly increasing in the caller's slot, sb_engine.h h_user_slot)
// so the result is that of render.js's order for any schedule, and a resolve pass turns keys into RGB8.
// Every double operation of render.js is restated in the same order in double (the library builds with -ffp-contract=off):
// toPx(v) = v / S * res, the box floor / ceil, the pixel centre (p + 0.5) / res * S, V8's Math.hypot (scaled, Kahan-summed),
// the line points floor(a + (b - a) * k / n).  Beams are clipped exactly: every point coordinate is monotone in k (each rounded
// operation is), so the k whose points land in the image form an interval, found by bisection.
//
// Where render.js does not terminate the engine draws nothing: a particle with an infinite coordinate (or a box bound of
// magnitude 2^53 or more: `p++` stops counting there), a beam with a non-finite endpoint coordinate or with n >= 2^53 points;
// a NaN centre draws nothing in both.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <stdexcept>
#include <vector>

#include "sb_engine.h"
#include "sb_render_math.h"

#define SBR_BLOCK 256
#define SBR_WIDE_BLOCKS 2048u // workgroups of the wave-per-primitive kernels (they stride over the list)

static const uint64_t kKeyParticle = 1ull << 62, kKeyBeam = 2ull << 62;

// what sb_render keeps between calls (sb_engine.h rs): the draw tables of the scene of the latest upload (built at the first
// render after it) and the key image (kept until sb_destroy or a larger resolution; not in the scene pool)
struct SbRenderState {
    bool valid = false;             // the tables belong to the scene on the device (sb_write_buffers clears this)
    bool copy_valid = false;        // ... d_copy alone (sbr_copy_table: shared with sb_state_io.hip's beam export)
    uint32_t nbeam_slots = 0;       // engine beam slots the tables cover
    uint2 *d_ends = nullptr;        // per engine beam slot: internal particle indices of A and B; x = 0xFFFFFFFF: not drawn
    uint32_t *d_copy = nullptr;     // per engine beam slot: the copy whose strain / stress is read back for it
    size_t cap_ends = 0, cap_copy = 0;
    uint32_t *d_wide_p = nullptr;   // particles whose clipped box is drawn by a wave
    uint4 *d_wide_b = nullptr;      // beams whose clipped range is drawn by a wave: slot, count, first k (u64)
    size_t cap_wide_p = 0, cap_wide_b = 0;
    uint32_t *d_count = nullptr;    // [2] lengths of the two lists
    unsigned long long *d_keys = nullptr;
    size_t cap_keys = 0;            // pixels
    uint8_t *d_rgb = nullptr;       // sb_render's picture on its way to the host
    size_t cap_rgb = 0;
    double build_ms = 0.0;          // host time of the last table build
};

// ---------------------------------------------------------------- kernels

__device__ __forceinline__ void sbr_put(unsigned long long *keys, uint32_t res, uint32_t px, uint32_t py, unsigned long long key)
{
    if (px < res && py < res) atomicMax(keys + (size_t)(res - 1 - py) * res + px, key); // row res-1-py: render.js's y flip
}

// one pixel of a particle's box
__device__ __forceinline__ void sbr_disc_pixel(unsigned long long *keys, const SbrArgs &a, double cx, double cy, uint32_t px,
                                               uint32_t py, unsigned long long base)
{
    const uint32_t c = sbr_disc_class(a, cx, cy, px, py);
    if (c) sbr_put(keys, a.nres, px, py, base | (unsigned long long)(c - 1u));
}

// a thread per particle: small boxes in place, large ones onto the wave list
__global__ __launch_bounds__(SBR_BLOCK) void k_render_particles(const float2 *__restrict__ pos, const uint32_t *__restrict__ pslot,
                                                                uint32_t P, SbrArgs a, unsigned long long *keys, uint32_t *wide,
                                                                uint32_t *count)
{
    const uint32_t j = blockIdx.x * SBR_BLOCK + threadIdx.x;
    if (j >= P) return;
    const float2 p = pos[j];
    uint32_t x0, x1, y0, y1;
    if (!sbr_box(a, p, x0, x1, y0, y1)) return;
    if ((uint64_t)(x1 - x0 + 1) * (y1 - y0 + 1) > SBR_INLINE_PIXELS) {
        wide[atomicAdd(count, 1u)] = j;
        return;
    }
    const unsigned long long base = kKeyParticle | ((unsigned long long)pslot[j] << 1);
    for (uint32_t py = y0; py <= y1; py++)
        for (uint32_t px = x0; px <= x1; px++) sbr_disc_pixel(keys, a, p.x, p.y, px, py, base);
}

// a wave per listed particle, its lanes over the clipped box
__global__ __launch_bounds__(SBR_BLOCK) void k_render_particles_wide(const float2 *__restrict__ pos, const uint32_t *__restrict__ pslot,
                                                                     SbrArgs a, unsigned long long *keys, const uint32_t *wide,
                                                                     const uint32_t *count)
{
    const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (SBR_BLOCK / 64);
    const uint32_t n = *count;
    for (uint32_t i = blockIdx.x * (SBR_BLOCK / 64) + threadIdx.x / 64u; i < n; i += waves) {
        const uint32_t j = wide[i];
        const float2 p = pos[j];
        uint32_t x0, x1, y0, y1;
        if (!sbr_box(a, p, x0, x1, y0, y1)) continue; // (true: it was listed)
        const uint32_t w = x1 - x0 + 1, h = y1 - y0 + 1;
        const unsigned long long base = kKeyParticle | ((unsigned long long)pslot[j] << 1);
        for (uint64_t q = lane; q < (uint64_t)w * h; q += 64u)
            sbr_disc_pixel(keys, a, p.x, p.y, x0 + (uint32_t)(q % w), y0 + (uint32_t)(q / w), base);
    }
}

// a thread per engine beam slot: the clipped k range, short ranges in place, long ones onto the wave list
__global__ __launch_bounds__(SBR_BLOCK) void k_render_beams(const float2 *__restrict__ pos, const uint2 *__restrict__ ends,
                                                            const uint32_t *__restrict__ dead, uint32_t B, SbrArgs a,
                                                            unsigned long long *keys, uint4 *wide, uint32_t *count)
{
    const uint32_t s = blockIdx.x * SBR_BLOCK + threadIdx.x;
    if (s >= B) return;
    const uint2 en = ends[s];
    if (en.x == 0xFFFFFFFFu || (dead && dead[s])) return;
    SbrLine l;
    if (!sbr_line(a, pos[en.x], pos[en.y], l)) return;
    const double hi = a.res - 1.0;
    uint64_t k0, k1; // [k0, k1)
    if (!sbr_clip_line(l, 0.0, hi, 0.0, hi, k0, k1)) return;
    const uint64_t cnt = k1 - k0;
    if (cnt > SBR_INLINE_POINTS) {
        wide[atomicAdd(count, 1u)] = make_uint4(s, (uint32_t)cnt, (uint32_t)k0, (uint32_t)(k0 >> 32));
        return;
    }
    const unsigned long long key = kKeyBeam | s;
    for (uint64_t k = k0; k < k1; k++)
        sbr_put(keys, a.nres, (uint32_t)sbr_point(l.ax, l.dx, (double)k, l.n), (uint32_t)sbr_point(l.ay, l.dy, (double)k, l.n), key);
}

// a wave per listed beam, its lanes over the clipped points (at most ~2 per pixel along the major axis: cnt < 2^32)
__global__ __launch_bounds__(SBR_BLOCK) void k_render_beams_wide(const float2 *__restrict__ pos, const uint2 *__restrict__ ends,
                                                                 SbrArgs a, unsigned long long *keys, const uint4 *wide,
                                                                 const uint32_t *count)
{
    const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (SBR_BLOCK / 64);
    const uint32_t n = *count;
    for (uint32_t i = blockIdx.x * (SBR_BLOCK / 64) + threadIdx.x / 64u; i < n; i += waves) {
        const uint4 w = wide[i];
        const uint2 en = ends[w.x];
        SbrLine l;
        if (!sbr_line(a, pos[en.x], pos[en.y], l)) continue; // (true: it was listed)
        const uint64_t k0 = (uint64_t)w.z | ((uint64_t)w.w << 32);
        const unsigned long long key = kKeyBeam | w.x;
        for (uint32_t q = lane; q < w.y; q += 64u) {
            const double k = (double)(k0 + q);
            sbr_put(keys, a.nres, (uint32_t)sbr_point(l.ax, l.dx, k, l.n), (uint32_t)sbr_point(l.ay, l.dy, k, l.n), key);
        }
    }
}

// key -> RGB8, one pixel per thread (keys are stored in output row order already)
__global__ __launch_bounds__(SBR_BLOCK) void k_render_resolve(const unsigned long long *__restrict__ keys, size_t npix,
                                                              const uint32_t *__restrict__ copy, const float *__restrict__ strain,
                                                              const float *__restrict__ stress, uint8_t *rgb)
{
    const size_t i = (size_t)blockIdx.x * SBR_BLOCK + threadIdx.x;
    if (i >= npix) return;
    const unsigned long long key = keys[i];
    uint32_t r = 0, g = 0, b = 0;
    if ((key >> 62) == 1u) {
        sbr_particle_rgb(key & 1ull, r, g, b);
    } else if ((key >> 62) == 2u) {
        const uint32_t c = copy[(uint32_t)key];
        sbr_beam_rgb(strain[c], stress[c], r, g, b);
    }
    rgb[i * 3 + 0] = (uint8_t)r;
    rgb[i * 3 + 1] = (uint8_t)g;
    rgb[i * 3 + 2] = (uint8_t)b;
}

// ---------------------------------------------------------------- host side

template <typename T>
static sb_status sbr_grow(sb_engine *e, T **p, size_t &cap, size_t n)
{
    n = std::max<size_t>(n, 1);
    if (*p && cap >= n) return SB_OK;
    if (*p) {
        SB_HIP(e, hipStreamSynchronize(e->stream)); // a render in flight may still read it
        SB_HIP(e, hipFree(*p));
        *p = nullptr;
        cap = 0;
    }
    SB_HIP(e, hipMalloc((void **)p, n * sizeof(T)));
    cap = n;
    return SB_OK;
}

void sbr_invalidate(sb_engine *e)
{
    if (e && e->rs) e->rs->valid = e->rs->copy_valid = false;
}

void sbr_release(sb_engine *e)
{
    if (!e || !e->rs) return;
    SbRenderState *r = e->rs;
    void *ps[] = {r->d_ends, r->d_copy, r->d_wide_p, r->d_wide_b, r->d_count, r->d_keys, r->d_rgb};
    for (void *p : ps)
        if (p) (void)hipFree(p);
    delete r;
    e->rs = nullptr;
}

double sbr_last_build_ms(const sb_engine *e) { return e && e->rs ? e->rs->build_ms : 0.0; }

// the lengths of the two wave lists of the latest render: {particles, beams} (0, 0 before the first); waits for the stream
sb_status sbr_wide_counts(sb_engine *e, uint32_t counts[2])
{
    counts[0] = counts[1] = 0u;
    if (!e->rs || !e->rs->d_count) return SB_OK;
    SB_HIP(e, hipStreamSynchronize(e->stream));
    SB_HIP(e, hipMemcpy(counts, e->rs->d_count, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SB_OK;
}

// per engine beam slot: the copy whose state sb_load_buffers reads back for it (h_copy_of_slot on the device), built at the first
// use after an upload; the draw tables and sb_state_io.hip's beam export share it (copy may be NULL: build only)
sb_status sbr_copy_table(sb_engine *e, const uint32_t **copy)
{
    if (!e->rs) e->rs = new SbRenderState();
    SbRenderState &r = *e->rs;
    if (!r.copy_valid) {
        const uint32_t B = e->B;
        if (e->h_copy_of_slot.size() < B) SB_FAIL(e, SB_ERR_STATE, "host shadows of the scene are inconsistent");
        SB_TRY(sbr_grow(e, &r.d_copy, r.cap_copy, B));
        if (B) SB_HIP(e, hipMemcpyAsync(r.d_copy, e->h_copy_of_slot.data(), (size_t)B * 4, hipMemcpyHostToDevice, e->stream));
        SB_HIP(e, hipStreamSynchronize(e->stream)); // (an upload may rewrite the host array)
        r.copy_valid = true;
    }
    if (copy) *copy = r.d_copy;
    return SB_OK;
}

// per engine beam slot: endpoints as internal particle indices and the copy read back for it (the caller's slots of the latest
// upload only; the engine's slots an upload cut are not drawn)
static sb_status sbr_build_tables(sb_engine *e)
{
    SbRenderState &r = *e->rs;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t P = e->P, B = e->B, maxP = e->opt.max_particles;
    if (e->h_pidx.size() != P || e->h_beams.size() != B || e->h_copy_of_slot.size() < B)
        SB_FAIL(e, SB_ERR_STATE, "sb_render: host shadows of the scene are inconsistent");
    std::vector<uint32_t> internal_of_index(maxP, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < P; i++) internal_of_index[e->h_pidx[i]] = i;
    std::vector<uint2> ends(std::max<uint32_t>(B, 1), make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu));
    const size_t Bu = e->h_user_slot.empty() ? B : e->h_user_slot.size();
    sbt::parallel_ranges(Bu, 1 << 16, [&](size_t u0, size_t u1) {
        for (size_t u = u0; u < u1; u++) {
            const uint32_t s = e->h_user_slot.empty() ? (uint32_t)u : e->h_user_slot[u];
            const SbHostBeam &h = e->h_beams[s];
            ends[s] = make_uint2(internal_of_index[h.da], internal_of_index[h.db]);
        }
    });
    for (const uint2 &v : ends)
        if (v.x != 0xFFFFFFFFu && (v.x >= P || v.y >= P)) SB_FAIL(e, SB_ERR_STATE, "sb_render: beam endpoint outside the scene");
    SB_TRY(sbr_grow(e, &r.d_ends, r.cap_ends, B));
    SB_TRY(sbr_copy_table(e, nullptr));
    SB_HIP(e, hipMemcpyAsync(r.d_ends, ends.data(), (size_t)std::max<uint32_t>(B, 1) * sizeof(uint2), hipMemcpyHostToDevice, e->stream));
    SB_TRY(sbr_grow(e, &r.d_wide_p, r.cap_wide_p, P));
    SB_TRY(sbr_grow(e, &r.d_wide_b, r.cap_wide_b, B));
    SB_HIP(e, hipStreamSynchronize(e->stream)); // (the host vectors go out of scope)
    r.nbeam_slots = B;
    r.valid = true;
    r.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SB_OK;
}

static sb_status sbr_enqueue(sb_engine *e, const sb_render_options *o, uint8_t *d_rgb, size_t bytes_avail, bool host_bytes,
                             uint32_t *res_out)
{
    if (!e) return SB_ERR_INVALID;
    if (o && o->struct_size != 0 && o->struct_size != sizeof(sb_render_options))
        SB_FAIL(e, SB_ERR_INVALID, "sb_render: sb_render_options.struct_size %u != %zu", o->struct_size, sizeof(sb_render_options));
    const bool given = o && o->struct_size;
    const uint32_t res = given && o->resolution ? o->resolution : 512u;
    if (res > SB_RENDER_MAX_RESOLUTION) SB_FAIL(e, SB_ERR_INVALID, "sb_render: resolution %u above %u", res, SB_RENDER_MAX_RESOLUTION);
    if (!e->loaded) SB_FAIL(e, SB_ERR_STATE, "sb_render before sb_write_buffers");
    if (e->n_ghost_p || e->n_send_p || e->n_ghost_b || e->n_send_b)
        SB_FAIL(e, SB_ERR_UNSUPPORTED, "sb_render: the engine has ghost zones configured (ranks are not composited)");
    const size_t npix = (size_t)res * res;
    if (host_bytes && bytes_avail < npix * 3)
        SB_FAIL(e, SB_ERR_INVALID, "sb_render: buffer of %zu bytes, the picture needs %zu", bytes_avail, npix * 3);
    if (!d_rgb && !host_bytes) SB_FAIL(e, SB_ERR_INVALID, "sb_render_device: null destination");
    SbrArgs a;
    a.S = given && o->bounds_size != 0.0 ? o->bounds_size : (double)e->opt.bounds_size;
    a.r = given && o->particle_radius != 0.0 ? o->particle_radius : (double)e->opt.particle_radius;
    a.r08 = a.r * 0.8;
    a.res = (double)res;
    a.nres = res;
    SB_HIP(e, hipSetDevice(e->device));
    if (!e->rs) e->rs = new SbRenderState();
    SbRenderState &r = *e->rs;
    if (!r.valid) SB_TRY(sbr_build_tables(e));
    if (!r.d_count) SB_HIP(e, hipMalloc((void **)&r.d_count, 2 * sizeof(uint32_t)));
    SB_TRY(sbr_grow(e, &r.d_keys, r.cap_keys, npix));
    SB_HIP(e, hipMemsetAsync(r.d_keys, 0, npix * sizeof(unsigned long long), e->stream));
    SB_HIP(e, hipMemsetAsync(r.d_count, 0, 2 * sizeof(uint32_t), e->stream));
    const float2 *pos = e->part[e->cur].pos;
    const uint32_t *dead = e->B && e->delete_gen ? e->d_dead_gen : nullptr; // as sb_load_buffers (fetch_dead) sees it
    const uint32_t P = e->P, B = e->B;
    if (P) {
        k_render_particles<<<(P + SBR_BLOCK - 1) / SBR_BLOCK, SBR_BLOCK, 0, e->stream>>>(pos, e->d_pslot, P, a, r.d_keys, r.d_wide_p,
                                                                                        r.d_count);
        k_render_particles_wide<<<SBR_WIDE_BLOCKS, SBR_BLOCK, 0, e->stream>>>(pos, e->d_pslot, a, r.d_keys, r.d_wide_p, r.d_count);
    }
    if (B) {
        k_render_beams<<<(B + SBR_BLOCK - 1) / SBR_BLOCK, SBR_BLOCK, 0, e->stream>>>(pos, r.d_ends, dead, B, a, r.d_keys, r.d_wide_b,
                                                                                    r.d_count + 1);
        k_render_beams_wide<<<SBR_WIDE_BLOCKS, SBR_BLOCK, 0, e->stream>>>(pos, r.d_ends, a, r.d_keys, r.d_wide_b, r.d_count + 1);
    }
    k_render_resolve<<<(unsigned)((npix + SBR_BLOCK - 1) / SBR_BLOCK), SBR_BLOCK, 0, e->stream>>>(
        r.d_keys, npix, r.d_copy, e->beams.strain, e->beams.stress, d_rgb);
    SB_HIP(e, hipGetLastError());
    *res_out = res;
    return SB_OK;
}

static sb_status sbr_render_device(sb_engine *e, const sb_render_options *opts, void *device_rgb)
{
    uint32_t res = 0;
    return sbr_enqueue(e, opts, (uint8_t *)device_rgb, 0, false, &res);
}

static sb_status sbr_render(sb_engine *e, const sb_render_options *opts, void *rgb, size_t rgb_bytes)
{
    if (!e) return SB_ERR_INVALID;
    if (!rgb) SB_FAIL(e, SB_ERR_INVALID, "sb_render: null destination");
    // the size check needs the resolution before anything is enqueued: sbr_enqueue checks it against rgb_bytes
    const bool given = opts && opts->struct_size;
    const size_t res = given && opts->resolution ? opts->resolution : 512u;
    if (res <= SB_RENDER_MAX_RESOLUTION && e->loaded) {
        if (!e->rs) e->rs = new SbRenderState();
        if (rgb_bytes >= res * res * 3) SB_TRY(sbr_grow(e, &e->rs->d_rgb, e->rs->cap_rgb, res * res * 3));
    }
    uint32_t got = 0;
    SB_TRY(sbr_enqueue(e, opts, e->rs ? e->rs->d_rgb : nullptr, rgb_bytes, true, &got));
    SB_HIP(e, hipMemcpyAsync(rgb, e->rs->d_rgb, (size_t)got * got * 3, hipMemcpyDeviceToHost, e->stream));
    SB_HIP(e, hipStreamSynchronize(e->stream));
    return SB_OK;
}

extern "C" {

sb_status sb_render_device(sb_engine *e, const sb_render_options *opts, void *device_rgb) { SB_GUARDED(e, sbr_render_device(e, opts, device_rgb)) }
sb_status sb_render(sb_engine *e, const sb_render_options *opts, void *rgb, size_t rgb_bytes) { SB_GUARDED(e, sbr_render(e, opts, rgb, rgb_bytes)) }

} // extern "C"
