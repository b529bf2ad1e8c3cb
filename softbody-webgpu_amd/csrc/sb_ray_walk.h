// sb_ray_walk.h -- which cells of a uniform grid a ray must look into so that no primitive the float32 tests of sb_batch_ray_math.h
// would meet is left out: the cells' rule, what is recorded where, the walkable gate and the walk itself, shared by the kernels of
// sb_raycast.hip and by the host model that tests/ray_walk_check.cpp runs.  Header-only and HIP-free on the host.
// The walk's own arithmetic is binary64: its rounding (2^-53 relative) is far below every margin below, so only the float32 TESTS
// need an error analysis.  What the walk visits never changes an output bit -- the answer is an integer minimum over keys -- as long
// as it is a superset of what the tests would meet; that is what this file has to guarantee.
//
// GRID.  G x G cells of side `cell` over [0, bounds]^2, cell id = iy * G + ix, coord(x) = min(G - 1, (uint32) (x / cell)) in float32
// (sb_grid_coord's value for 0 <= x).  A particle is IN-GRID iff both coordinates are finite and inside [0, bounds]; it is recorded
// in its cell.  A live beam is SHORT iff both endpoints are in-grid and their cells differ by at most one per axis; it is recorded
// once, in the lower-left cell (min ix, min iy) of those.  Everything else -- a particle outside, infinite or NaN; a beam with such
// an endpoint or a wider box -- goes on the LEFTOVER list, which every valid row is tested against.
//
// WHAT A FLOAT TEST CAN MEET (u = 2^-24; W: the distance from the origin O to the centre, or to endpoint A; |D| = sqrt(a)).
// Disc.  wx, wy are exact for a centre moved by at most u W.  b carries at most 2u W |D|, ww = wx wx + wy wy at most 2u W^2,
//   c = ww - r2 at most 3u W^2 + 2u r^2, b b at most 5u a W^2, a c at most a u (6 W^2 + 2 r^2) (each bound times 1 + O(u)).  The test
//   passes iff fl(b b) >= fl(a c) (the last subtraction keeps the sign), so exactly b^2 - a c >= -a u (11 W^2 + 2 r^2); with
//   b^2 - a c = a (r^2 - p^2), p the distance of the centre from the ray's LINE:  p <= r (1 + u) + sqrt(11 u) W + u W.
//   sqrt(11 u) = 3.32 * 2^-12: with KAPPA = 2^-9 the bound  p <= r + KAPPA (W + r)  holds with a factor two to spare.  It grows
//   linearly with the distance: the cancellation in q loses about half the bits of W^2, and that half is what KAPPA is.
//   c <= 0 ("inside") needs W <= r (1 + 3u).  b > 0 needs the centre at most 2u W behind O along the ray.  The t of a hit is at
//   least (s - r - KAPPA (W + r)) / |D| (1 - 5u), s the centre's distance along the ray: the same bound on sqrt(q).
// Segment.  With the computed w and e exact for endpoints moved by at most u (W + L) (L: the beam's length), den carries at most
//   2u |D| L, un at most 2u W |D|.  un = -|D| (signed distance of A from the line), den - un = +|D| (that of B).  The test needs
//   0 <= un <= den after both are given den's sign: one endpoint is at most 2u (W + L) on the far side of the line from the other,
//   or they straddle it.  So the segment comes within 4u (W + L) of the LINE -- far inside the discs' margin.  But nothing bounds
//   WHERE along the line: a beam that is collinear with the ray to within rounding yields den, un and tn that are all noise, and
//   the float test can then meet it at any t in [0, tmax], even when it lies behind the origin or beyond tmax.  Brute force reports
//   such a meeting, so must the walk: a row whose mask has SB_RAY_BEAMS walks the whole line across the grid and never stops early.
//
// THE WALK runs along the ray's major axis (|slope| <= 1 against it), one step per column of cells (a row of cells when y is the
// major axis).  In a step whose column spans [xa, xb] the line's minor coordinates span [ya, yb]; with X = max |x - ox| over the
// column, every in-grid centre of that column that a test can meet lies within
//     R(X) = r + 2^-8 (X + 4 r) + 2^-20 bounds
// of the line (W <= sqrt 2 (X + R) + R turns KAPPA (W + r) into at most 2^-8 (0.72 X + 1.22 r); the last term covers the float32
// coord() against the exact floor and G cell against bounds, 16 ulps of bounds), so within 1.5 R >= sqrt 2 R of [ya, yb] in the
// minor coordinate.  The step visits the minor cells of [ya - 1.5 R, yb + 1.5 R], two more below and one more above: a short beam
// is recorded in the lower-left cell of a 2 x 2 box, so the cell where it comes within reach of the line may be one column on and,
// against a falling line, two rows up from where it is recorded.  A row without SB_RAY_BEAMS walks the columns of
// [ox, ox + tmax dx] widened by 2 R(Xmax) and one column each way (Xmax: the largest X of the grid); with beams, all G columns.
// EARLY EXIT (rows without SB_RAY_BEAMS only).  Behind a column whose far edge is `f` ahead of O on the major axis, every centre
// still to come has t >= (f - 2 R(Xmax) - 2^-20 bounds) / |d_major| (1 - 2^-20) =: T.  The walk stops iff the best t so far is
// STRICTLY below T: a later cell could at best tie T's own bits only from above, and a tie on t is resolved by kind and index,
// which only a visit can settle.
//
// WALKABLE GATE.  The derivation assumes ordinary numbers: a row is walkable iff ox, oy lie in [-bounds, 2 bounds] and
// a = dx dx + dy dy (float32) lies in [2^-40, 2^40].  Every other valid row (a zero direction among them) is answered by the sweep
// over all records; counts[4] counts them.  A grid whose radius or bounds are not in [2^-20, 2^30] has G = 1: one cell, always visited.
#pragma once
#include <math.h>
#include <stdint.h>

#include "sb_batch_ray_math.h"

#define SRW_MAX_CELLS_PER_SIDE 8192u
#define SRW_KIND_BIT 0x80000000u // in a record's index word: a beam

namespace srw {

struct Grid {
    uint32_t G;
    float cell, bounds, radius;
};

// a record of the counting sort: a particle (ax, ay; bx, by unused) or a short / leftover beam; lsrc: the particle data index whose label skips it
struct Rec {
    float ax, ay, bx, by;
    uint32_t index; // data index | SRW_KIND_BIT for a beam
    uint32_t lsrc;
};

// the default rule's cap: the largest G with G * G <= particles / 2, at least 1, at most SRW_MAX_CELLS_PER_SIDE
SBR_HD uint32_t default_cap(uint32_t particles)
{
    const uint64_t most = particles / 2u;
    uint64_t g = 1;
    while ((g + 1) * (g + 1) <= most && g < SRW_MAX_CELLS_PER_SIDE) g++;
    return (uint32_t)g;
}
// "are radius and bounds numbers the derivation covers?" (false: one cell)
SBR_HD bool ordinary(float bounds, float radius) { return radius >= 0x1p-20f && radius <= 0x1p30f && bounds >= 0x1p-20f && bounds <= 0x1p30f; }

SBR_HD uint32_t coord(float x, float cell, uint32_t G)
{
    const float q = x / cell;
    if (!(q > 0.0f)) return 0u;
    if (q >= (float)G) return G - 1u;
    return (uint32_t)q;
}
SBR_HD bool in_grid(float x, float y, float bounds)
{
    return sbr::finite_bits(sbr::float_as_word(x)) && sbr::finite_bits(sbr::float_as_word(y)) && x >= 0.0f && x <= bounds && y >= 0.0f && y <= bounds;
}
// the bin of a particle: its cell, or G * G (the leftover list)
SBR_HD uint32_t particle_bin(float x, float y, const Grid &g)
{
    if (!in_grid(x, y, g.bounds)) return g.G * g.G;
    return coord(y, g.cell, g.G) * g.G + coord(x, g.cell, g.G);
}
// the bin of a live beam: the lower-left cell of a short one, or G * G
SBR_HD uint32_t beam_bin(float ax, float ay, float bx, float by, const Grid &g)
{
    if (!in_grid(ax, ay, g.bounds) || !in_grid(bx, by, g.bounds)) return g.G * g.G;
    const uint32_t xa = coord(ax, g.cell, g.G), xb = coord(bx, g.cell, g.G), ya = coord(ay, g.cell, g.G), yb = coord(by, g.cell, g.G);
    const uint32_t x0 = xa < xb ? xa : xb, x1 = xa < xb ? xb : xa, y0 = ya < yb ? ya : yb, y1 = ya < yb ? yb : ya;
    if (x1 - x0 > 1u || y1 - y0 > 1u) return g.G * g.G;
    return y0 * g.G + x0;
}

SBR_HD bool walkable(const sbr::Ray &r, float bounds)
{
    const float lo = -bounds, hi = 2.0f * bounds;
    return r.ox >= lo && r.ox <= hi && r.oy >= lo && r.oy <= hi && r.a >= 0x1p-40f && r.a <= 0x1p40f;
}

SBR_HD double reach(double X, const Grid &g) { return (double)g.radius + 0x1p-8 * (X + 4.0 * (double)g.radius) + 0x1p-20 * (double)g.bounds; }

// floor(v / cell) clamped into [-4, G + 4] (v may be infinite; never NaN for a walkable row)
SBR_HD int64_t cell_floor(double v, double cell, uint32_t G)
{
    const double q = floor(v / cell);
    if (!(q > -4.0)) return -4;
    if (q > (double)G + 4.0) return (int64_t)G + 4;
    return (int64_t)q;
}

// The walk's margins and its exit rule, in one place.  tests/ray_walk_check.cpp derives WRONG policies from it (no pad; `<=`) to show
// that its cases catch them; the library only ever instantiates this one.
struct Policy {
    SBR_HD static double along(double Rmax, double fuzz) { return 2.0 * Rmax + fuzz; } // widens [ox, ox + tmax dx] on the major axis
    SBR_HD static int64_t columns() { return 1; }                                      // and columns more, each way
    SBR_HD static double across(double R) { return 1.5 * R; }                          // widens [ya, yb] on the minor axis
    SBR_HD static int64_t below() { return 2; }                                        // and cells more below
    SBR_HD static int64_t above() { return 1; }                                        // and above
    // "may the walk stop behind a column whose far edge is `ahead` of O?" -- t: the best so far; STRICTLY below the bound
    SBR_HD static bool stops(double t, double ahead, double Rmax, double fuzz, double dm, double radius)
    {
        (void)radius;
        return t < (ahead - 2.0 * Rmax - fuzz) / dm * (1.0 - 0x1p-20);
    }
};

// The walk of one walkable row.  cells(first, count, stride): look into `count` cells first, first + stride, ...; best(): the t bits
// of the smallest key so far as a float, or a negative number while there is none.  Returns the number of steps taken.  A row that
// asks for neither particles nor beams has nothing to look for: no step.
template <class P = Policy, class Cells, class Best>
SBR_HD uint32_t walk(const sbr::Ray &r, const Grid &g, Cells &&cells, Best &&best)
{
    if (!(r.mask & (sbr::MASK_PARTICLES | sbr::MASK_BEAMS))) return 0u;
    if (g.G == 1u) {
        cells(0u, 1u, 1u);
        return 1u;
    }
    const bool xmajor = fabsf(r.dx) >= fabsf(r.dy), beams = (r.mask & sbr::MASK_BEAMS) != 0u;
    const double om = xmajor ? r.ox : r.oy, on = xmajor ? r.oy : r.ox, dm = xmajor ? r.dx : r.dy, dn = xmajor ? r.dy : r.dx;
    const double slope = dn / dm, cell = g.cell, top = (double)g.G * cell; // (dm != 0: a >= 2^-40)
    const double Xmax = fmax(fabs(om), fabs(top - om)), Rmax = reach(Xmax, g), fuzz = 0x1p-20 * (double)g.bounds;
    int64_t m0 = 0, m1 = (int64_t)g.G - 1;
    if (!beams) {
        const double end = om + (double)r.tmax * dm; // (tmax = +inf: an infinity of dm's sign; tmax = 0: om)
        const double lo = fmin(om, end) - P::along(Rmax, fuzz), hi = fmax(om, end) + P::along(Rmax, fuzz);
        const int64_t c0 = cell_floor(lo, cell, g.G) - P::columns(), c1 = cell_floor(hi, cell, g.G) + P::columns();
        if (c0 > m0) m0 = c0;
        if (c1 < m1) m1 = c1;
    }
    const bool up = dm > 0.0;
    uint32_t steps = 0u;
    for (int64_t k = 0; k <= m1 - m0; k++) {
        const int64_t m = up ? m0 + k : m1 - k;
        const double xa = (double)m * cell, xb = xa + cell;
        const double ya = on + (xa - om) * slope, yb = on + (xb - om) * slope;
        const double X = fmax(fabs(xa - om), fabs(xb - om)), V = P::across(reach(X, g));
        int64_t n0 = cell_floor(fmin(ya, yb) - V, cell, g.G) - P::below(), n1 = cell_floor(fmax(ya, yb) + V, cell, g.G) + P::above();
        if (n0 < 0) n0 = 0;
        if (n1 > (int64_t)g.G - 1) n1 = (int64_t)g.G - 1;
        if (n0 <= n1) {
            const uint32_t count = (uint32_t)(n1 - n0 + 1);
            if (xmajor) cells((uint32_t)n0 * g.G + (uint32_t)m, count, g.G);
            else cells((uint32_t)m * g.G + (uint32_t)n0, count, 1u);
        }
        steps++;
        if (beams) continue;
        const float t = best();
        if (!(t >= 0.0f)) continue;
        const double ahead = up ? xb - om : om - xa; // the far edge of this column, ahead of O
        if (P::stops((double)t, ahead, Rmax, fuzz, fabs(dm), (double)g.radius)) break;
    }
    return steps;
}

} // namespace srw
