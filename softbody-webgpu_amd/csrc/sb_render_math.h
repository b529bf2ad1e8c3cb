// sb_render_math.h -- the device arithmetic of a picture (host/render.js, in its order), shared by sb_render.hip (one engine,
// key image in device memory) and sb_batch_render.hip (a batch, key image in LDS).  Every double operation of render.js is
// restated in the same order in double (the library builds with -ffp-contract=off): toPx(v) = v / S * res, the box floor / ceil,
// the pixel centre (p + 0.5) / res * S, V8's Math.hypot (scaled, Kahan-summed), the line points floor(a + (b - a) * k / n).
// Beams are clipped exactly: every point coordinate is monotone in k (each rounded operation is), so the k whose points land in
// a rectangle of pixels form an interval, found by bisection.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#define SBR_INLINE_PIXELS 64u // a particle's clipped box up to this many pixels is drawn by its own thread, larger ones by a wave
#define SBR_INLINE_POINTS 32u // the same for a beam's clipped points

static const double kTwo53 = 9007199254740992.0;

struct SbrArgs {
    double S, r, r08, res; // bounds, radius, radius * 0.8, resolution (render.js numbers)
    uint32_t nres;         // resolution as an integer
};

// V8's Math.hypot for two finite arguments: both scaled by the larger magnitude, squares summed with Kahan compensation
__device__ __forceinline__ double sbr_hypot(double a, double b)
{
    const double x = fabs(a), y = fabs(b);
    double mx = 0.0;
    if (x > mx) mx = x;
    if (y > mx) mx = y;
    if (mx == 0.0) return 0.0;
    double sum = 0.0, comp = 0.0;
    {
        const double n = x / mx;
        const double summand = n * n - comp;
        const double pre = sum + summand;
        comp = (pre - sum) - summand;
        sum = pre;
    }
    {
        const double n = y / mx;
        const double summand = n * n - comp;
        const double pre = sum + summand;
        comp = (pre - sum) - summand;
        sum = pre;
    }
    return sqrt(sum) * mx;
}

__device__ __forceinline__ double sbr_to_px(double v, const SbrArgs &a) { return v / a.S * a.res; }

// one pixel of a particle's box: 0 = outside the disc, 1 = inner colour, 2 = ring
__device__ __forceinline__ uint32_t sbr_disc_class(const SbrArgs &a, double cx, double cy, uint32_t px, uint32_t py)
{
    const double wx = ((double)px + 0.5) / a.res * a.S, wy = ((double)py + 0.5) / a.res * a.S;
    const double d = sbr_hypot(wx - cx, wy - cy);
    if (d < a.r08) return 1u;
    if (d < a.r) return 2u;
    return 0u;
}

// the particle's box clipped to the image; false: nothing to draw (including where render.js does not terminate)
__device__ __forceinline__ bool sbr_box(const SbrArgs &a, float2 p, uint32_t &x0, uint32_t &x1, uint32_t &y0, uint32_t &y1)
{
    const double cx = p.x, cy = p.y;
    if (!(isfinite(cx) && isfinite(cy))) return false;
    const double X0 = floor(sbr_to_px(cx - a.r, a)), X1 = ceil(sbr_to_px(cx + a.r, a));
    const double Y0 = floor(sbr_to_px(cy - a.r, a)), Y1 = ceil(sbr_to_px(cy + a.r, a));
    if (!(Y0 <= Y1)) return false; // no row (NaN bounds included)
    if (!(fabs(Y0) < kTwo53 && fabs(Y1) < kTwo53)) return false;
    if (!(X0 <= X1)) return false;
    if (!(fabs(X0) < kTwo53 && fabs(X1) < kTwo53)) return false;
    const double hi = a.res - 1.0;
    const double cx0 = fmax(X0, 0.0), cx1 = fmin(X1, hi), cy0 = fmax(Y0, 0.0), cy1 = fmin(Y1, hi);
    if (cx0 > cx1 || cy0 > cy1) return false;
    x0 = (uint32_t)cx0, x1 = (uint32_t)cx1, y0 = (uint32_t)cy0, y1 = (uint32_t)cy1;
    return true;
}

// a point of a beam: floor(a + (b - a) * k / n)
__device__ __forceinline__ double sbr_point(double a0, double d, double k, double n) { return floor(a0 + d * k / n); }

// smallest k in [lo, hi] with pred(k) (pred false ... true over k), hi + 1 if none
template <typename F>
__device__ __forceinline__ uint64_t sbr_first(uint64_t lo, uint64_t hi, F pred)
{
    uint64_t l = lo, h = hi + 1; // answer in [l, h]
    while (l < h) {
        const uint64_t m = l + (h - l) / 2;
        if (pred(m)) h = m;
        else l = m + 1;
    }
    return l;
}

// the k range [klo, khi) of one coordinate's points inside [lo, hi]; the coordinate is monotone in k
__device__ __forceinline__ void sbr_clip_axis(double a0, double d, double n, uint64_t N, double lo, double hi, uint64_t &klo,
                                              uint64_t &khi)
{
    if (d >= 0.0) { // non-decreasing (d = 0: constant)
        klo = sbr_first(0, N, [&](uint64_t k) { return sbr_point(a0, d, (double)k, n) >= lo; });
        const uint64_t past = sbr_first(0, N, [&](uint64_t k) { return sbr_point(a0, d, (double)k, n) > hi; });
        khi = past; // exclusive
    } else {        // non-increasing
        klo = sbr_first(0, N, [&](uint64_t k) { return sbr_point(a0, d, (double)k, n) <= hi; });
        khi = sbr_first(0, N, [&](uint64_t k) { return sbr_point(a0, d, (double)k, n) < lo; });
    }
}

struct SbrLine {
    double ax, ay, dx, dy, n;
};

// the beam's line; false: nothing to draw
__device__ __forceinline__ bool sbr_line(const SbrArgs &a, float2 A, float2 B, SbrLine &l)
{
    l.ax = sbr_to_px(A.x, a);
    l.ay = sbr_to_px(A.y, a);
    const double bx = sbr_to_px(B.x, a), by = sbr_to_px(B.y, a);
    if (!(isfinite(l.ax) && isfinite(l.ay) && isfinite(bx) && isfinite(by))) return false;
    l.dx = bx - l.ax;
    l.dy = by - l.ay;
    const double m = ceil(fmax(fabs(l.dx), fabs(l.dy))); // (finite operands: fmax = Math.max)
    l.n = m > 1.0 ? m : 1.0;
    return l.n < kTwo53;
}

// the k range [k0, k1) of the line's points inside the pixel rectangle [xlo, xhi] x [ylo, yhi] (y before the flip);
// false: none
__device__ __forceinline__ bool sbr_clip_line(const SbrLine &l, double xlo, double xhi, double ylo, double yhi, uint64_t &k0,
                                              uint64_t &k1)
{
    const uint64_t N = (uint64_t)l.n;
    k0 = 0, k1 = N + 1;
    const double x0 = sbr_point(l.ax, l.dx, 0.0, l.n), xN = sbr_point(l.ax, l.dx, l.n, l.n);
    const double y0 = sbr_point(l.ay, l.dy, 0.0, l.n), yN = sbr_point(l.ay, l.dy, l.n, l.n);
    if (!(x0 >= xlo && x0 <= xhi && xN >= xlo && xN <= xhi && y0 >= ylo && y0 <= yhi && yN >= ylo && yN <= yhi)) {
        uint64_t xl, xh, yl, yh;
        sbr_clip_axis(l.ax, l.dx, l.n, N, xlo, xhi, xl, xh);
        sbr_clip_axis(l.ay, l.dy, l.n, N, ylo, yhi, yl, yh);
        k0 = xl > yl ? xl : yl;
        k1 = xh < yh ? xh : yh;
        if (k0 >= k1) return false;
    }
    return true;
}

// render.js's byte of a Float32Array component: Math.round(clamp01(c) * 255), NaN -> 0 (Buffer stores ToUint8(NaN) = 0)
__device__ __forceinline__ uint32_t sbr_byte(float c)
{
    const double v = c;
    if (v != v) return 0u;
    const double cl = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
    return (uint32_t)floor(cl * 255.0 + 0.5); // exact: a float times 255 has at most 32 significant bits
}

// JS Math.max(0, Math.min(1, v)) (NaN stays NaN), then the Float32Array store
__device__ __forceinline__ float sbr_clamp01_f32(double v)
{
    if (v != v) return __builtin_nan("");
    return (float)(v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v));
}

// the bytes of a particle's pixel: ring (1, 1, 1), inner (0, 0.35, 0.5): f32(0.35) * 255 = 89.25, 0.5 * 255 = 127.5
__device__ __forceinline__ void sbr_particle_rgb(bool ring, uint32_t &r, uint32_t &g, uint32_t &b)
{
    if (ring) r = g = b = 255u;
    else r = 0u, g = 89u, b = 128u;
}

// the bytes of a beam's pixel from its strain and stress
__device__ __forceinline__ void sbr_beam_rgb(float strain, float stress, uint32_t &r, uint32_t &g, uint32_t &b)
{
    const double sn = strain, ss = stress;
    r = sbr_byte(sbr_clamp01_f32(ss + 1.0));
    g = sbr_byte(sbr_clamp01_f32(1.0 - ss));
    const double bb = 1.0 - fabs(sn);
    b = sbr_byte(bb != bb ? __builtin_nanf("") : (float)(bb < 0.0 ? 0.0 : bb)); // Math.max(0, .) keeps NaN
}
