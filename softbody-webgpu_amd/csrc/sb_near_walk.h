// sb_near_walk.h -- which cells of the ray casts' uniform grid a proximity query must look into so that nothing the float32 distances
// of sb_batch_near_math.h would keep, and nothing that could win, is left out: the local gate, the rings of cells round a point and
// the rule that ends them, shared by the kernels of sb_nearest.hip and by the host model that tests/near_walk_check.cpp runs
// (DESIGN.md 5.31).  Header-only and HIP-free on the host.  The grid, the records and what is recorded where are sb_ray_walk.h's,
// unchanged: G x G cells of side `cell` over [0, bounds]^2, an in-grid particle in its cell, a short beam once, in the lower-left cell
// of its 2 x 2 box, everything else on the leftover list.  The walk's own arithmetic is binary64 (2^-53 relative: far below every
// margin here), so only the float32 DISTANCES and the float32 coord() of the sort need an error analysis.
//
// LOCAL GATE.  A row is LOCAL iff px and py lie in [-bounds, 2 bounds]; every other valid row is answered by the sweep over all
// records (counts[4]).  A grid whose radius or bounds are no ordinary numbers has G = 1: one cell, visited, nothing to derive.
//
// RINGS.  The point's VIRTUAL cell is (cx, cy) = (floor(px / cell), floor(py / cell)), not clipped: it may lie outside the grid.  After
// ring h = 0, 1, 2 ... the walk has seen the cells of S(h) = [cx - h - 1, cx + h] x [cy - h - 1, cy + h], clipped to the grid: the
// square of Chebyshev half-width h round the virtual cell and one more column and row towards LOWER x and y, because a short beam
// that reaches into the square from the left or from below is recorded one cell left of or below the cells it crosses.  Ring h
// visits S(h) \ S(h - 1): the rows cy + h and cy - h - 1 as one run of neighbouring cells each, and in every row between them the
// two cells cx - h - 1 and cx + h.  The sets are disjoint, so every cell is visited exactly once -- `within` counts, it does not
// take a minimum.  The first ring is h0 = max(0, -cx, cx - G, -cy, cy - G), the first whose S meets the grid (it visits all of
// S(h0)); the rings before it hold no cell and cost no step of the budget.
//
// WHAT IS LEFT AFTER RING h (u = 2^-24).  An in-grid particle in cell ix satisfies ix cell - e <= x <= (ix + 1) cell + e with
// e = 1.01 u bounds: coord() rounds x / cell once (relative u, at most u G cell absolute), G cell lies within (1 +- 2u) bounds, and
// the clamp to G - 1 only ever moves an x <= bounds.  The point satisfies cx cell <= px < (cx + 1) cell to 2^-50 bounds.  A particle
// NOT in S(h) has ix >= cx + h + 1 or ix <= cx - h - 2 (or the same in y), so on that axis it is at least
//     A(h) = h cell - 2^-23 bounds
// from the point.  A short beam NOT in S(h) is recorded in x0 >= cx + h + 1 or x0 <= cx - h - 2; both endpoints lie in the cells
// x0 and x0 + 1, and so does every point between them: EVERY point of the segment is at least A(h) from the point on that axis
// (towards lower x the recorded cell is one further away than the cells the beam crosses: that is the extra column and row).
// The float distances.
//   Particle (and a beam clamped to an endpoint, the same expression bit for bit).  vx = fl(cx - px) has relative error u, the two
//   squares and their sum relative u each: d2 >= A^2 (1 - u)^4.  There is no cancellation: the coordinates are given floats, only
//   the operators round -- unlike the ray's disc, whose b b - a c loses half the bits.  A(h) > 0 in a bound that is used is at
//   least 2^-41 (bounds and radius are >= 2^-20), its square is a normal number: no underflow touches the bound.
//   Beam, projected inside.  u_f = fl(we / ee) is computed from rounded products whose error is NOT small against we when the point
//   is far away -- and it does not matter: the branch has 0 < we < ee in floats, so 0 <= u_f < 1 whatever its error, and
//   Q' = A + u_f (B - A), in exact arithmetic, is a point OF THE SEGMENT: at least A(h) from the point on the axis.  The computed
//   qx = fl(ax + fl(u_f fl(bx - ax))) differs from Q'x by at most u_f |bx - ax| (2u + u^2) + u |qx| <= u (2 len + bounds) (1 + 2u):
//   an ABSOLUTE error of a few ulps of (bounds + the beam's length), with len <= sqrt 2 bounds at most 3.83 u bounds < 2^-22 bounds.
//   Then vx = fl(qx - px) and the squares as for a particle: d2 >= (A - 2^-22 bounds)^2 (1 - u)^4.
// Together: every in-grid primitive outside S(h) has a float d2 of at least (h cell - (1/8 + 1/4) 2^-20 bounds)^2 (1 - 2^-22).  The
// library's bound takes c = 1 where the derivation needs c = 3/8:
//     L(h) = (h cell - 2^-20 bounds) (1 - 2^-20),    every unvisited in-grid d2 >= L(h)^2 when L(h) > 0  (no bound while L(h) <= 0).
//
// STOP.  After ring h the walk stops iff
//     rmax2 < L(h)^2                                  -- nothing further on can be kept, or
//     `within` is not asked for and best d2 < L(h)^2  -- nothing further on can win (best: the row's smallest key so far, its walls
//                                                        among them),
// both STRICTLY: a later ring could at best tie L(h)^2 from above, and a tie on d2 is settled by kind and index, which only a visit
// can settle.  The walk is also complete once S(h) covers the grid.  It ends WITHOUT being complete after max_rings rings; the row
// is then answered by the sweep, which counts its `within` afresh (the walk's partial counts are discarded; its keys may stay: a
// minimum does not mind).  So rmax = +inf WITH `within` sweeps by construction unless the rings cover the grid -- the count of
// everything is a sum over everything --, and rmax = +inf WITHOUT `within` stops at the first ring whose bound exceeds the winner.
// The leftover list is tested against every row that the sweep does not answer, whatever its walk saw.
#pragma once
#include <math.h>
#include <stdint.h>

#include "sb_batch_near_math.h"
#include "sb_ray_walk.h" // srw::Grid, srw::Rec, the bins

#define SNW_MAX_RINGS 8192u
#define SNW_DEFAULT_RINGS 8u // sb_nearest_options.max_rings == 0 (tools/nearest_timing.py sweeps it)

namespace snw {

SBN_HD bool local(const sbn::Probe &p, float bounds)
{
    const float lo = -bounds, hi = 2.0f * bounds;
    return p.px >= lo && p.px <= hi && p.py >= lo && p.py <= hi;
}

// The walk's margins and its stop rule, in one place.  tests/near_walk_check.cpp derives WRONG policies from it (no extra cell; `<=`;
// no slack) to show that its cases catch them; the library only ever instantiates this one.
struct Policy {
    SBN_HD static int64_t low() { return 1; }                                   // cells more towards lower x and y
    SBN_HD static double slack(double bounds) { return 0x1p-20 * bounds; }      // c 2^-20 bounds, c = 1
    SBN_HD static double shrink() { return 1.0 - 0x1p-20; }                     // the relative part of L(h)
    SBN_HD static bool below(double d2, double bound2) { return d2 < bound2; }  // STRICTLY
};

// L(h)^2, or a negative number while there is no bound
template <class P>
SBN_HD double bound2(int64_t h, const srw::Grid &g)
{
    const double l = ((double)h * (double)g.cell - P::slack((double)g.bounds)) * P::shrink();
    return l > 0.0 ? l * l : -1.0;
}

// the first ring that holds a cell of the grid
template <class P>
SBN_HD int64_t first_ring(int64_t cx, int64_t cy, int64_t G)
{
    const int64_t past = (cx > cy ? cx : cy) - P::low() - (G - 1), before = -(cx < cy ? cx : cy);
    const int64_t h = past > before ? past : before;
    return h > 0 ? h : 0;
}

// The walk of one local row.  cells(first, count): look into the `count` neighbouring cells from `first`; best(): the d2 of the
// smallest key so far, or a negative number while there is none.  Returns true iff the walk is COMPLETE (it stopped, or it covered
// the grid), false iff it ran out of rings: the sweep must answer the row.  *rings: the rings it took.  A row that asks for neither
// particles nor beams has nothing to look for: complete, no ring.
template <class P = Policy, class Cells, class Best>
SBN_HD bool walk(const sbn::Probe &p, const srw::Grid &g, uint32_t max_rings, bool within, Cells &&cells, Best &&best, uint32_t *rings = nullptr)
{
    uint32_t taken = 0u;
    if (rings) *rings = 0u;
    if (!(p.mask & (sbn::MASK_PARTICLES | sbn::MASK_BEAMS))) return true;
    const int64_t G = (int64_t)g.G;
    if (G == 1) {
        cells(0u, 1u);
        if (rings) *rings = 1u;
        return true;
    }
    const int64_t cx = (int64_t)floor((double)p.px / (double)g.cell), cy = (int64_t)floor((double)p.py / (double)g.cell); // (local: |.| <= 2 G + 1)
    const int64_t h0 = first_ring<P>(cx, cy, G);
    const double rmax2 = (double)p.rmax2;
    for (int64_t h = h0;; h++) {
        const int64_t x0 = cx - h - P::low(), x1 = cx + h, y0 = cy - h - P::low(), y1 = cy + h;
        const int64_t X0 = x0 > 0 ? x0 : 0, X1 = x1 < G - 1 ? x1 : G - 1, Y0 = y0 > 0 ? y0 : 0, Y1 = y1 < G - 1 ? y1 : G - 1; // (h >= h0: not empty)
        const uint32_t run = (uint32_t)(X1 - X0 + 1);
        if (h == h0) { // all of S(h0)
            for (int64_t y = Y0; y <= Y1; y++) cells((uint32_t)(y * G + X0), run);
        } else {
            if (y0 >= 0 && y0 < G) cells((uint32_t)(y0 * G + X0), run);
            for (int64_t y = y0 + 1 > 0 ? y0 + 1 : 0; y <= (y1 - 1 < G - 1 ? y1 - 1 : G - 1); y++) {
                if (x0 >= 0 && x0 < G) cells((uint32_t)(y * G + x0), 1u);
                if (x1 >= 0 && x1 < G) cells((uint32_t)(y * G + x1), 1u);
            }
            if (y1 >= 0 && y1 < G) cells((uint32_t)(y1 * G + X0), run);
        }
        taken++;
        if (rings) *rings = taken;
        if (x0 <= 0 && x1 >= G - 1 && y0 <= 0 && y1 >= G - 1) return true; // the grid is covered
        const double l2 = bound2<P>(h, g);
        if (P::below(rmax2, l2)) return true;
        if (!within) {
            const float b = best();
            if (b >= 0.0f && P::below((double)b, l2)) return true;
        }
        if (taken >= max_rings) return false;
    }
}

} // namespace snw
