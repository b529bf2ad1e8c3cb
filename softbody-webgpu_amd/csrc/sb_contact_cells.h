// sb_contact_cells.h -- "who is in contact with this particle, taken in ascending index order?", stated once for the kernels that
// ask it (k_batch_frame's cells, k_batch_contacts, k_batch_forces, k_contacts_visit / k_contacts_list, k_batch_add_particles;
// DESIGN.md 5.33):
//   the test       sb_touch under the threshold of sb_touch_test(radius): dist == 0 or dist < 2r, the step's own expressions
//   the cells      sb_batch_cell_cap / sb_batch_cell_geometry: G x G cells at least 2r (1 + 1/64) wide over [0, bounds]^2.  With a
//                  monotone, clamped coordinate map (sb_grid_coord, sb_physics.h) whoever touches a particle sits in the 3 x 3
//                  cells around its own:
//   the window     SbCellWindow, the 3 x 3 cells clamped to the grid, over either storage form:
//                  sorted runs   the indices sorted by cell, end[c] the end of cell c's run: row yy of the window is ONE run
//                  buckets       SB_BATCH_CELL_K 16-bit entries a cell in LDS, two 16-bit counts to a word; a full bucket says so
//   the selection  SbSelect4 / sb_select_ascending: sweeps that keep the four smallest partners above the last one applied.  The
//                  order of the partners is their indices', whatever the order inside a cell and whichever form stores them.
// Host and device, header-only and HIP-free on the host: tests/contact_cells_check.cpp runs all of it against brute force under
// sanitizers.  Floats take one rounding per operator in the order written (build with -ffp-contract=off).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include "sb_physics.h" // sb_sqrt: the root the step takes (SB_ABLATE & 16 swaps it)
#define SBCC_HD __host__ __device__ __forceinline__
#define SBCC_UNROLL _Pragma("unroll")
#else
#define SBCC_HD inline
#define SBCC_UNROLL
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SBCC_SQRT sb_sqrt
#else
#define SBCC_SQRT __builtin_sqrtf
#endif

// ---------------------------------------------------------------- the contact test
// The root is only taken where d2 <= thr = (2r)^2 * 1.001 (beyond it sqrt(d2) > 2r * 1.0004, which no rounding brings back under
// 2r, and d2 > 0).  thr is +inf where that product is no ordinary number (a tiny, huge or NaN radius): the shortcut is off.
struct SbTouchTest { float two_r, thr; };
SBCC_HD SbTouchTest sb_touch_test(float radius)
{
    const float two_r = radius * 2.0f, thr0 = two_r * two_r * 1.001f;
    return SbTouchTest{two_r, (thr0 >= 0x1p-100f && thr0 <= 0x1p100f) ? thr0 : __builtin_inff()};
}

// The contact test of the step's collision loop on two positions.  A NaN d2 fails `d2 > thr` and then every comparison: a NaN or
// infinite distance is no contact.
SBCC_HD bool sb_touch_xy(float mx, float my, float ox, float oy, float thr, float two_r)
{
    const float dx = ox - mx, dy = oy - my, d2 = dx * dx + dy * dy;
    if (d2 > thr) return false;
    const float dist = SBCC_SQRT(d2); // sb_length(dx, dy)
    return dist == 0.0f || dist < two_r;
}
template <class Float2> // (float2 on the device; any {x, y} of floats on the host)
SBCC_HD bool sb_touch(Float2 me, Float2 other, float thr, float two_r) { return sb_touch_xy(me.x, me.y, other.x, other.y, thr, two_r); }

// ---------------------------------------------------------------- the cells: geometry
// the most cells per side a capacity gets: the largest G with G^2 <= 2.5 * max_particles (17 at 128, 25 at 256, 50 at 1024)
SBCC_HD uint32_t sb_batch_cell_cap(uint32_t maxP)
{
    uint32_t g = 1u;
    while (2u * (g + 1u) * (g + 1u) <= 5u * maxP) g++;
    return g;
}
// cells per side and their width for a radius and bounds: SbGrid's rule, cell >= 2r (1 + 1/64); G = clamp(floor(bounds / that),
// 1, cap), the cells then as wide as G of them need to cover the bounds (never narrower than the rule: coarser is always right;
// whatever lies past the last cell is clamped into it).  0: the width is not an ordinary number (the batch walks, the contacts
// reports test all pairs).
SBCC_HD uint32_t sb_batch_cell_geometry(float bounds, float radius, uint32_t cap, float *cell)
{
    const float two_r = radius * 2.0f, cell_min = two_r * (1.0f + 1.0f / 64.0f);
    if (!(cell_min >= 0x1p-60f && cell_min <= 0x1p60f) || !(bounds >= 0x1p-60f && bounds <= 0x1p60f)) return 0u;
    const float per_side = bounds / cell_min; // (ordinary: both are)
    const uint32_t g = per_side >= (float)cap ? cap : (per_side >= 1.0f ? (uint32_t)per_side : 1u);
    *cell = cell_min < bounds / (float)g ? bounds / (float)g : cell_min;
    return g;
}

// ---------------------------------------------------------------- the window
// the 3 x 3 cells around cell (cx, cy) of a G x G grid, clamped: columns x0 .. x1 of rows y0 .. y1
struct SbCellWindow {
    uint32_t x0, x1, y0, y1, G;
    SBCC_HD SbCellWindow(uint32_t cx, uint32_t cy, uint32_t g) : G(g)
    {
        x0 = cx > 0u ? cx - 1u : 0u, x1 = cx + 1u < G ? cx + 1u : G - 1u, y0 = cy > 0u ? cy - 1u : 0u, y1 = cy + 1u < G ? cy + 1u : G - 1u;
    }
    // sorted runs (end[c]: where cell c's run ends; cell 0's begins at 0): the cells x0 .. x1 of row yy are neighbours in the
    // sorted array, one run [*from, *to)
    SBCC_HD void run(const uint32_t *__restrict__ end, uint32_t yy, uint32_t *from, uint32_t *to) const
    {
        const uint32_t r0 = yy * G + x0, r1 = yy * G + x1;
        *from = r0 ? end[r0 - 1u] : 0u, *to = end[r1];
    }
};

// ---------------------------------------------------------------- the selection
#define SB_SELECT_NONE 0xFFFFFFFFu
// One sweep's state: the four smallest indices offered so far, ascending (the carry of sb_physics.h's SB_SELECT_INSERT, on one
// array), and the index the sweep must stay above, if there is one.
struct SbSelect4 {
    uint32_t bs[4], last;
    bool have_last;
    // "could o still be one of the four?" -- asked before the float test, so that most candidates never take it
    SBCC_HD bool wants(uint32_t o) const { return !(have_last && o <= last) && o < bs[3]; }
    SBCC_HD void insert(uint32_t o)
    {
SBCC_UNROLL
        for (int q = 0; q < 4; q++) {
            const uint32_t small = o < bs[q] ? o : bs[q];
            o = o < bs[q] ? bs[q] : o, bs[q] = small;
        }
    }
};
// The partners of one particle in ascending order: sweep(sel) offers every partner that sel.wants() to sel.insert(); the (up to)
// four it kept go to apply(o), smallest first, which returns false to end the walk (a full pair list); a sweep that comes back
// with fewer than four was the last.  Starts above `last` where have_last (a pair list: last = the particle itself).
template <class Sweep, class Apply>
SBCC_HD void sb_select_ascending(bool have_last, uint32_t last, Sweep &&sweep, Apply &&apply)
{
    SbSelect4 sel{{0u, 0u, 0u, 0u}, last, have_last};
    for (;;) {
SBCC_UNROLL
        for (int q = 0; q < 4; q++) sel.bs[q] = SB_SELECT_NONE;
        sweep(sel);
SBCC_UNROLL
        for (int q = 0; q < 4; q++) {
            if (sel.bs[q] != SB_SELECT_NONE) {
                if (!apply(sel.bs[q])) return;
                sel.last = sel.bs[q], sel.have_last = true;
            }
        }
        if (sel.bs[3] == SB_SELECT_NONE) return; // (fewer than four were left)
    }
}

// ---------------------------------------------------------------- the buckets
#define SB_BATCH_CELL_K 4u // slot entries a cell holds
// words of a G x G grid's entries, u16[G * G][SB_BATCH_CELL_K], and of ONE array of its counts, two 16-bit counts to a word; the
// counts follow the entries
SBCC_HD uint32_t sb_bucket_entry_words(uint32_t g) { return g * g * SB_BATCH_CELL_K / 2u; }
SBCC_HD uint32_t sb_bucket_count_words(uint32_t g) { return (g * g + 1u) / 2u; }

// slot into cell c; true: the cell was full and the slot is NOT in it (the counts were zeroed; at most 65535 pushes a cell: no
// carry into the neighbour's half).  On the device the count is taken by an LDS atomic: any number of lanes may push at once.
SBCC_HD bool sb_bucket_push(uint16_t *ent, uint32_t *cnt, uint32_t c, uint32_t slot)
{
    const uint32_t sh = (c & 1u) << 4;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t before = atomicAdd(&cnt[c >> 1], 1u << sh);
#else
    const uint32_t before = cnt[c >> 1];
    cnt[c >> 1] = before + (1u << sh);
#endif
    const uint32_t n = (before >> sh) & 0xffffu;
    const bool room = n < SB_BATCH_CELL_K;
    if (room) ent[c * SB_BATCH_CELL_K + n] = (uint16_t)slot;
    return !room;
}
// pushes cell c has seen (its entries: the first min(that, SB_BATCH_CELL_K))
SBCC_HD uint32_t sb_bucket_count(const uint32_t *cnt, uint32_t c) { return (cnt[c >> 1] >> ((c & 1u) << 4)) & 0xffffu; }
// the entries of cell c in one 8-byte load, and entry j of them
struct alignas(8) SbBucketWords { uint32_t x, y; };
SBCC_HD SbBucketWords sb_bucket_load(const uint16_t *ent, uint32_t c)
{
    SbBucketWords w;
#if defined(__HIP_DEVICE_COMPILE__)
    w = *(const SbBucketWords *)(ent + c * SB_BATCH_CELL_K); // (one ds_read_b64; the entries start 8-byte aligned)
#else
    memcpy(&w, ent + c * SB_BATCH_CELL_K, sizeof w);
#endif
    return w;
}
SBCC_HD uint32_t sb_bucket_entry(SbBucketWords w, uint32_t j) { return ((j < 2u ? w.x : w.y) >> ((j & 1u) << 4)) & 0xffffu; }
// f(slot) for every entry of the window's cells (no cell was full: the caller looked at what the pushes returned)
template <class F>
SBCC_HD void sb_bucket_for_window(const SbCellWindow &w, const uint16_t *ent, const uint32_t *cnt, F &&f)
{
    for (uint32_t yy = w.y0; yy <= w.y1; yy++) {
        for (uint32_t xx = w.x0; xx <= w.x1; xx++) {
            const uint32_t c = yy * w.G + xx, n = sb_bucket_count(cnt, c);
            const SbBucketWords e = sb_bucket_load(ent, c);
SBCC_UNROLL
            for (uint32_t j = 0; j < SB_BATCH_CELL_K; j++)
                if (j < n) f(sb_bucket_entry(e, j));
        }
    }
}
