// sb_batch_render.hip -- one picture per scene of a batch in ONE launch (sb_batch_render_device / sb_batch_render_scene of
// include/softbody.h) for gfx950 (CDNA4, wave64).
//
// The picture of scene i is host/render.js's renderPPM of what sb_batch_load_scene(i) would return, byte for byte: sb_render's
// rules (sb_render.hip) and sb_render's arithmetic (sb_render_math.h, called, not restated).  What differs is the shape:
//
//   grid    count x bands workgroups; a workgroup owns rows_per_band whole picture rows of one scene
//   keys    the band's key image lives in LDS, 32 bits per pixel (a scene has at most 1024 particle and 4096 beam slots):
//               0                                   black
//               1 << 30 | particle slot << 1 | ring  (ring = 1: white, 0: inner colour; a slot puts a pixel at most once)
//               2 << 30 | beam slot                  (the caller's slot: the delete pass compacts the mapping in place)
//           every put is a ds_max_u32, so "last writer wins" is render.js's for any schedule
//   inputs  the batch's blobs as they are: counts from the metadata (agent scope, as k_batch_frame reads them), positions
//           g_part[3 * pmap[slot]] staged in LDS once per workgroup, endpoints g_bword[bmap[slot]], colours g_bstate[bmap[slot]].zw
//   draw    a thread per particle slot, then a thread per beam slot, each primitive clipped to the band's rows (discs: the
//           box's rows; beams: the per-axis bisection with the band's bounds); primitives over SBR_INLINE_PIXELS /
//           SBR_INLINE_POINTS go onto an LDS list that the waves then work off, a wave per primitive, lane-parallel
//   resolve keys -> packed RGB in place, then the band's bytes leave as aligned dwords (bytes at an unaligned head / tail):
//           every output byte is written exactly once, by nobody else; no key image in HBM, no memset, no global atomics
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "sb_batch.h"
#include "sb_render_math.h"

#define SBBR_THREADS 256u
// LDS of one workgroup: four fit a CU (160 KiB); measured faster than 80 and 160 KiB at 128^2 and 256^2, equal at 64^2 (DESIGN.md
// 5.11).  rows_per_band follows from it; at least half of it is keys (a capacity of 1024 / 4096 slots alone takes 28 KiB).
#define SBBR_LDS_BUDGET (40u * 1024u)
#define SBBR_LDS_LIMIT (160u * 1024u)
#define SBBR_KEY_PARTICLE (1u << 30)
#define SBBR_KEY_BEAM (2u << 30)

struct SbBatchRender {
    uint8_t *d_rgb = nullptr; // sb_batch_render_scene's picture on its way to the host
    size_t cap_rgb = 0;
    bool attr_set = false;    // the kernel may use the whole LDS
    uint32_t last_lds = 0, last_bands = 0;
};

// the band of a workgroup: picture rows r0 .. r0 + nrows - 1 are render.js's y = pyhi down to pylo
struct SbbrBand {
    uint32_t res, pylo, pyhi;
};

SB_DEV void sbbr_put(uint32_t *s_key, const SbbrBand &bd, uint32_t px, uint32_t py, uint32_t key)
{
    if (px < bd.res && py >= bd.pylo && py <= bd.pyhi) atomicMax(&s_key[(bd.pyhi - py) * bd.res + px], key);
}

// the particle's box clipped to the band; false: nothing of it in these rows
SB_DEV bool sbbr_box(const SbrArgs &a, const SbbrBand &bd, float2 p, uint32_t &x0, uint32_t &x1, uint32_t &y0, uint32_t &y1)
{
    if (!sbr_box(a, p, x0, x1, y0, y1)) return false;
    y0 = y0 > bd.pylo ? y0 : bd.pylo;
    y1 = y1 < bd.pyhi ? y1 : bd.pyhi;
    return y0 <= y1;
}

SB_DEV void sbbr_disc_pixel(uint32_t *s_key, const SbrArgs &a, const SbbrBand &bd, float2 p, uint32_t px, uint32_t py, uint32_t base)
{
    const uint32_t c = sbr_disc_class(a, p.x, p.y, px, py);
    if (c) sbbr_put(s_key, bd, px, py, base | (c - 1u));
}

// the beam's line and the k range [k0, k1) of its points inside the band; false: nothing of it in these rows
SB_DEV bool sbbr_beam(const SbrArgs &a, const SbbrBand &bd, float2 A, float2 B, SbrLine &l, uint64_t &k0, uint64_t &k1)
{
    if (!sbr_line(a, A, B, l)) return false;
    return sbr_clip_line(l, 0.0, a.res - 1.0, (double)bd.pylo, (double)bd.pyhi, k0, k1);
}

__global__ __launch_bounds__(SBBR_THREADS) void k_batch_render(SbBatchView V, SbrArgs a, uint32_t first, uint32_t bands,
                                                               uint32_t rows_per_band, uint8_t *out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sbbr_lds[];
    const uint32_t tid = threadIdx.x, T = SBBR_THREADS, lane = tid & 63u, wave = tid >> 6, nwaves = T / 64u;
    const uint32_t rel = blockIdx.x / bands, band = blockIdx.x - rel * bands, scene = first + rel, res = a.nres;
    const uint32_t r0 = band * rows_per_band, nrows = min(rows_per_band, res - r0), npix = nrows * res;
    SbbrBand bd;
    bd.res = res;
    bd.pylo = res - r0 - nrows; // row res-1-py: render.js's y flip
    bd.pyhi = res - 1u - r0;
    const uint32_t maxP = V.maxP, maxB = V.maxB;

    // LDS map (sbbr_lds_fixed mirrors it)
    float2 *s_pos = (float2 *)sbbr_lds;                // [maxP] position per particle slot
    uint32_t *s_wide_p = (uint32_t *)(s_pos + maxP);   // [maxP] particle slots a wave draws
    uint32_t *s_wide_b = s_wide_p + maxP;              // [maxB] beam slots a wave draws
    uint32_t *s_cnt = s_wide_b + maxB;                 // [2] lengths of the two lists
    uint32_t *s_key = s_cnt + 2u;                      // [rows_per_band][res] keys, then packed RGB

    const uint32_t *meta = V.meta + (size_t)scene * SB_BM_WORDS;
    // (metadata words are rewritten between launches by other kernels: read at agent scope, never through the scalar cache)
    uint32_t P = sbb_uniform(SB_AGENT_LOAD(&meta[SB_BM_P])), Bc = sbb_uniform(SB_AGENT_LOAD(&meta[SB_BM_B]));
    if (P == 0u || P > maxP || Bc > maxB) P = Bc = 0u; // an empty (or never uploaded) scene: black
    const unsigned char *cst = V.cst + (size_t)scene * V.cst_bytes, *st = V.st + (size_t)scene * V.st_bytes;
    const uint32_t *g_pmap = (const uint32_t *)(cst + V.o_pmap), *g_bword = (const uint32_t *)(cst + V.o_bword);
    const float2 *g_part = (const float2 *)(st + V.o_part);
    const float4 *g_bstate = (const float4 *)(st + V.o_bstate);
    const uint32_t *g_bmap = (const uint32_t *)(st + V.o_bmap);

    for (uint32_t i = tid; i < npix; i += T) s_key[i] = 0u;
    if (tid < 2u) s_cnt[tid] = 0u;
    for (uint32_t s = tid; s < P; s += T) {
        const uint32_t d = g_pmap[s];
        s_pos[s] = d < maxP ? g_part[3u * d] : make_float2(__builtin_nanf(""), 0.f); // (validated at upload)
    }
    __syncthreads();

    // ---- a thread per particle slot
    for (uint32_t s = tid; s < P; s += T) {
        const float2 p = s_pos[s];
        uint32_t x0, x1, y0, y1;
        if (!sbbr_box(a, bd, p, x0, x1, y0, y1)) continue;
        if ((x1 - x0 + 1u) * (y1 - y0 + 1u) > SBR_INLINE_PIXELS) {
            s_wide_p[atomicAdd(&s_cnt[0], 1u)] = s;
            continue;
        }
        const uint32_t base = SBBR_KEY_PARTICLE | (s << 1);
        for (uint32_t py = y0; py <= y1; py++)
            for (uint32_t px = x0; px <= x1; px++) sbbr_disc_pixel(s_key, a, bd, p, px, py, base);
    }
    // ---- a thread per beam slot
    for (uint32_t j = tid; j < Bc; j += T) {
        const uint32_t d = g_bmap[j];
        if (d >= maxB) continue; // (validated at upload)
        const uint32_t word = g_bword[d], ia = word & 0xffffu, ib = word >> 16;
        if (ia >= P || ib >= P) continue;
        SbrLine l;
        uint64_t k0, k1;
        if (!sbbr_beam(a, bd, s_pos[ia], s_pos[ib], l, k0, k1)) continue;
        if (k1 - k0 > SBR_INLINE_POINTS) {
            s_wide_b[atomicAdd(&s_cnt[1], 1u)] = j;
            continue;
        }
        const uint32_t key = SBBR_KEY_BEAM | j;
        for (uint64_t k = k0; k < k1; k++)
            sbbr_put(s_key, bd, (uint32_t)sbr_point(l.ax, l.dx, (double)k, l.n), (uint32_t)sbr_point(l.ay, l.dy, (double)k, l.n), key);
    }
    __syncthreads();

    // ---- a wave per listed primitive, its lanes over the clipped box / points (the clip is computed again: wave-uniform)
    const uint32_t nwp = s_cnt[0], nwb = s_cnt[1];
    for (uint32_t i = wave; i < nwp; i += nwaves) {
        const uint32_t s = s_wide_p[i];
        const float2 p = s_pos[s];
        uint32_t x0, x1, y0, y1;
        if (!sbbr_box(a, bd, p, x0, x1, y0, y1)) continue; // (true: it was listed)
        const uint32_t w = x1 - x0 + 1u, n = w * (y1 - y0 + 1u), base = SBBR_KEY_PARTICLE | (s << 1);
        for (uint32_t q = lane; q < n; q += 64u) sbbr_disc_pixel(s_key, a, bd, p, x0 + q % w, y0 + q / w, base);
    }
    for (uint32_t i = wave; i < nwb; i += nwaves) {
        const uint32_t j = s_wide_b[i], word = g_bword[g_bmap[j]];
        SbrLine l;
        uint64_t k0, k1;
        if (!sbbr_beam(a, bd, s_pos[word & 0xffffu], s_pos[word >> 16], l, k0, k1)) continue; // (true: it was listed)
        const uint32_t key = SBBR_KEY_BEAM | j;
        for (uint64_t k = k0 + lane; k < k1; k += 64u)
            sbbr_put(s_key, bd, (uint32_t)sbr_point(l.ax, l.dx, (double)k, l.n), (uint32_t)sbr_point(l.ay, l.dy, (double)k, l.n), key);
    }
    __syncthreads();

    // ---- keys -> packed RGB (r | g << 8 | b << 16), in place: a thread rewrites the pixels it reads
    for (uint32_t i = tid; i < npix; i += T) {
        const uint32_t key = s_key[i];
        uint32_t r = 0, g = 0, b = 0;
        if ((key >> 30) == 1u) {
            sbr_particle_rgb(key & 1u, r, g, b);
        } else if ((key >> 30) == 2u) {
            const float4 bs = g_bstate[g_bmap[key & 0x3fffffffu]];
            sbr_beam_rgb(bs.z, bs.w, r, g, b);
        }
        s_key[i] = r | (g << 8) | (b << 16);
    }
    __syncthreads();

    // ---- the band's bytes: dwords over the 4-byte aligned interior, single bytes at an unaligned head and tail
    uint8_t *dst = out + ((size_t)rel * res * res + (size_t)r0 * res) * 3u;
    const int nbytes = (int)(npix * 3u), mis = (int)((uintptr_t)dst & 3u);
    const uint32_t ndw = (uint32_t)(mis + nbytes + 3) / 4u;
    for (uint32_t w = tid; w < ndw; w += T) {
        const int off = (int)(4u * w) - mis; // of the dword's first byte in the band
        if (off >= 0 && off + 4 <= nbytes) {
            const uint32_t pix = (uint32_t)off / 3u, c = (uint32_t)off - 3u * pix;
            const uint64_t two = (uint64_t)s_key[pix] | ((uint64_t)s_key[pix + 1u < npix ? pix + 1u : pix] << 24);
            *(uint32_t *)(dst + off) = (uint32_t)(two >> (8u * c));
        } else {
            for (int o = off < 0 ? 0 : off; o < off + 4 && o < nbytes; o++) {
                const uint32_t pix = (uint32_t)o / 3u, c = (uint32_t)o - 3u * pix;
                dst[o] = (uint8_t)(s_key[pix] >> (8u * c));
            }
        }
    }
}

// ---------------------------------------------------------------- host
static inline uint32_t sbbr_lds_fixed(uint32_t maxP, uint32_t maxB) { return maxP * 12u + maxB * 4u + 8u; }

// options -> arguments; everything here is checked before a device is touched
static sb_status sbbr_options(sb_batch *b, const char *who, const sb_batch_render_options *o, SbrArgs &a, uint32_t &first, uint32_t &count)
{
    if (o && o->struct_size != 0 && o->struct_size != sizeof(sb_batch_render_options))
        SB_FAIL(b, SB_ERR_INVALID, "%s: sb_batch_render_options.struct_size %u != %zu", who, o->struct_size, sizeof(sb_batch_render_options));
    const bool given = o && o->struct_size;
    const uint32_t res = given && o->resolution ? o->resolution : 64u;
    if (res > SB_BATCH_RENDER_MAX_RESOLUTION)
        SB_FAIL(b, SB_ERR_INVALID, "%s: resolution %u above %u", who, res, (unsigned)SB_BATCH_RENDER_MAX_RESOLUTION);
    const uint32_t n = b->opt.n_scenes;
    first = given ? o->first : 0u;
    count = given ? o->count : 0u;
    if (first >= n || count > n - first)
        SB_FAIL(b, SB_ERR_INVALID, "%s: scenes %u .. %u+%u are not all inside the batch of %u", who, first, first, count, n);
    if (count == 0u) count = n - first;
    a.S = given && o->bounds_size != 0.0 ? o->bounds_size : (double)b->opt.bounds_size;
    a.r = given && o->particle_radius != 0.0 ? o->particle_radius : (double)b->opt.particle_radius;
    a.r08 = a.r * 0.8;
    a.res = (double)res;
    a.nres = res;
    return SB_OK;
}

static sb_status sbbr_launch(sb_batch *b, const SbrArgs &a, uint32_t first, uint32_t count, uint8_t *d_rgb)
{
    if (!b->render) b->render = new SbBatchRender();
    SbBatchRender &r = *b->render;
    const uint32_t res = a.nres, fixed = sbbr_lds_fixed(b->V.maxP, b->V.maxB), row = res * 4u;
    uint32_t budget = std::max(SBBR_LDS_BUDGET, fixed + SBBR_LDS_BUDGET / 2u);
    if (const char *env = getenv("SB_BATCH_RENDER_LDS_BYTES")) budget = (uint32_t)strtoul(env, nullptr, 10); // measurements
    budget = std::min(std::max(budget, fixed + row), SBBR_LDS_LIMIT);
    const uint32_t rows = std::min(res, (budget - fixed) / row), bands = cdivb(res, rows), lds = fixed + rows * row;
    if (!r.attr_set) {
        SB_HIP(b, hipFuncSetAttribute((const void *)k_batch_render, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SBBR_LDS_LIMIT));
        r.attr_set = true;
    }
    hipLaunchKernelGGL(k_batch_render, dim3(count * bands), dim3(SBBR_THREADS), lds, b->stream, b->V, a, first, bands, rows, d_rgb);
    r.last_lds = lds;
    r.last_bands = bands;
    return check_launch(b, "sb_batch render kernel");
}

void sbb_render_release(sb_batch *b)
{
    if (!b || !b->render) return;
    if (b->render->d_rgb) (void)hipFree(b->render->d_rgb);
    delete b->render;
    b->render = nullptr;
}

// sb_batch_get_info's render keys; false: not one of them
bool sbb_render_info(sb_batch *b, const char *key, uint64_t *value)
{
    const std::string k(key);
    if (k == "render_lds_bytes") *value = b->render ? b->render->last_lds : 0u;
    else if (k == "render_bands") *value = b->render ? b->render->last_bands : 0u;
    else return sbb_kernel_info(b, "render", (const void *)k_batch_render, b->render_res, key, value);
    return true;
}

extern "C" {

sb_status sb_batch_render_device(sb_batch *b, const sb_batch_render_options *opts, void *device_rgb)
{
    if (!b) return SB_ERR_INVALID;
    SbrArgs a;
    uint32_t first, count;
    const sb_status s = sbbr_options(b, "sb_batch_render_device", opts, a, first, count);
    if (s != SB_OK) return s;
    if (!device_rgb) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_render_device: null destination");
    SB_HIP(b, hipSetDevice(b->device));
    return sbbr_launch(b, a, first, count, (uint8_t *)device_rgb);
}

sb_status sb_batch_render_scene(sb_batch *b, uint32_t scene, const sb_batch_render_options *opts, void *rgb, size_t rgb_bytes)
{
    if (!b) return SB_ERR_INVALID;
    SbrArgs a;
    uint32_t first, count; // (of the options: the scene argument decides here)
    const sb_status s = sbbr_options(b, "sb_batch_render_scene", opts, a, first, count);
    if (s != SB_OK) return s;
    if (scene >= b->opt.n_scenes) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_render_scene: scene %u is not inside the batch of %u", scene, b->opt.n_scenes);
    const size_t bytes = (size_t)a.nres * a.nres * 3u;
    if (!rgb) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_render_scene: null destination");
    if (rgb_bytes < bytes) SB_FAIL(b, SB_ERR_INVALID, "sb_batch_render_scene: buffer of %zu bytes, the picture needs %zu", rgb_bytes, bytes);
    SB_HIP(b, hipSetDevice(b->device));
    SB_HIP(b, hipStreamSynchronize(b->stream));
    uint32_t loaded = 0;
    SB_HIP(b, hipMemcpy(&loaded, b->V.meta + (size_t)scene * SB_BM_WORDS + SB_BM_LOADED, 4, hipMemcpyDeviceToHost));
    if (loaded == 0u) SB_FAIL(b, SB_ERR_STATE, "sb_batch_render_scene: scene %u was never uploaded", scene);
    if (!b->render) b->render = new SbBatchRender();
    SbBatchRender &r = *b->render;
    if (r.cap_rgb < bytes) {
        if (r.d_rgb) SB_HIP(b, hipFree(r.d_rgb)); // (the stream is idle)
        r.d_rgb = nullptr, r.cap_rgb = 0;
        SB_HIP(b, hipMalloc((void **)&r.d_rgb, std::max<size_t>(bytes, 1)));
        r.cap_rgb = bytes;
    }
    const sb_status ls = sbbr_launch(b, a, scene, 1u, r.d_rgb);
    if (ls != SB_OK) return ls;
    SB_HIP(b, hipMemcpyAsync(rgb, r.d_rgb, bytes, hipMemcpyDeviceToHost, b->stream));
    SB_HIP(b, hipStreamSynchronize(b->stream));
    return SB_OK;
}

} // extern "C"
