// sb_cut_math.h -- "does this shape hit this beam?", the one predicate behind sb_cut_device / sb_cut (sb_cut.hip) and
// sb_batch_cut_device (sb_batch_cut.hip); include/softbody.h states it.  Host and device: float32, one rounding
// per operator in the order written (the library builds with -ffp-contract=off; tests/cut_check.cpp builds it the same way), no
// division, no square root.  Every comparison with a NaN is false, so a NaN hits nothing; an infinity follows the operators like
// any other number (an infinite radius over a finite beam is a hit).  Header-only and HIP-free on the host.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBX_HD __host__ __device__ inline
#else
#define SBX_HD inline
#endif

#define SBX_SHAPE_WORDS 8u // {kind, x0, y0, x1, y1, 0, 0, 0}: the kind an integer word, the rest floats

namespace sbx {

struct P2 {
    float x, y;
};

struct Shape {
    uint32_t kind; // SB_CUT_NONE / SB_CUT_SEGMENT / SB_CUT_DISC; any other kind hits nothing
    float x0, y0, x1, y1;
};

SBX_HD float word_as_float(uint32_t w)
{
    float f;
    memcpy(&f, &w, sizeof f);
    return f;
}

SBX_HD Shape shape_of(const uint32_t *w) { return Shape{w[0], word_as_float(w[1]), word_as_float(w[2]), word_as_float(w[3]), word_as_float(w[4])}; }

SBX_HD float orient(P2 u, P2 v, P2 w) { return (v.x - u.x) * (w.y - u.y) - (v.y - u.y) * (w.x - u.x); }

// w inside the box of u and v, edges included (written with comparisons only: no minimum whose NaN rule could differ)
SBX_HD bool inbox(P2 u, P2 v, P2 w)
{
    const float lox = u.x < v.x ? u.x : v.x, hix = u.x < v.x ? v.x : u.x;
    const float loy = u.y < v.y ? u.y : v.y, hiy = u.y < v.y ? v.y : u.y;
    return lox <= w.x && w.x <= hix && loy <= w.y && w.y <= hiy;
}

SBX_HD bool segment_hits(P2 P, P2 Q, P2 A, P2 B)
{
    const float d1 = orient(P, Q, A), d2 = orient(P, Q, B), d3 = orient(A, B, P), d4 = orient(A, B, Q);
    if (((d1 > 0.0f && d2 < 0.0f) || (d1 < 0.0f && d2 > 0.0f)) && ((d3 > 0.0f && d4 < 0.0f) || (d3 < 0.0f && d4 > 0.0f))) return true;
    if (d1 == 0.0f && inbox(P, Q, A)) return true;
    if (d2 == 0.0f && inbox(P, Q, B)) return true;
    if (d3 == 0.0f && inbox(A, B, P)) return true;
    if (d4 == 0.0f && inbox(A, B, Q)) return true;
    return false;
}

SBX_HD bool disc_hits(P2 C, float r, P2 A, P2 B)
{
    if (!(r >= 0.0f)) return false;
    const P2 d{B.x - A.x, B.y - A.y}, w{C.x - A.x, C.y - A.y};
    const float L2 = d.x * d.x + d.y * d.y, t = w.x * d.x + w.y * d.y, r2 = r * r;
    if (!(t > 0.0f)) return w.x * w.x + w.y * w.y <= r2;
    if (t >= L2) {
        const P2 u{C.x - B.x, C.y - B.y};
        return u.x * u.x + u.y * u.y <= r2;
    }
    const float c = d.x * w.y - d.y * w.x;
    return c * c <= r2 * L2;
}

// (the device variant of the call cannot see the shapes: an unknown kind, or a disc with y1 != 0, hits nothing)
SBX_HD bool shape_hits(const Shape &s, P2 A, P2 B)
{
    if (s.kind == 1u) return segment_hits(P2{s.x0, s.y0}, P2{s.x1, s.y1}, A, B);
    if (s.kind == 2u) return s.y1 == 0.0f && disc_hits(P2{s.x0, s.y0}, s.x1, A, B);
    return false;
}

} // namespace sbx
