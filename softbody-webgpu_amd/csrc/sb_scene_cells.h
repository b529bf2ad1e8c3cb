// sb_scene_cells.h -- the cells of the whole scene of an sb_engine that its contact reports sort into (sb_contacts.hip, sb_forces.hip;
// DESIGN.md 5.20, 5.34): how many cells a side and how wide (sb_contact_cells.h's rule under a cap of about eight cells a
// particle), the cell of a position, the window of a record's 3 x 3 cells, and the wave's one atomic per run of lanes that share a
// cell.  What a report sorts (its record) and what it does with a partner stay in its file.
#pragma once
#include <algorithm>

#include "sb_report.h"
#include "sb_batch.h" // sb_contact_cells.h: the cells' rule, the contact test, the window and the selection

#define SBC_NONE 0xFFFFFFFFu
#define SBC_MAX_CELLS_PER_SIDE 8192u    // 2^26 cells: 256 MiB of counts
#define SBC_ALL_PAIRS_MAX 4096u         // particles up to which a degenerate geometry is answered by the all-pairs test

struct SbcGeo {
    uint32_t G;
    float cell;
};

SB_DEV uint32_t sbc_cell(float x, float y, SbcGeo g) { return sb_grid_coord(y, 0.0f, g.cell, g.G) * g.G + sb_grid_coord(x, 0.0f, g.cell, g.G); }

// Add each maximal run of lanes with the same cell c != SBC_NONE to count[c] with one atomic of its first lane (sbd_add_runs'
// form: neighbouring data indices mostly lie in neighbouring places).  Every lane of the wave calls it.
SB_DEV void sbc_count_runs(uint32_t *count, uint32_t c)
{
    const uint32_t run = sbq_run_length(c, c != SBC_NONE);
    if (run) atomicAdd(&count[c], run);
}

// the window of a record's 3 x 3 cells (sb_contact_cells.h): row yy of them is sorted[from .. to), SbCellWindow::run
SB_DEV SbCellWindow sbc_window(float x, float y, SbcGeo g) { return SbCellWindow(sb_grid_coord(x, 0.0f, g.cell, g.G), sb_grid_coord(y, 0.0f, g.cell, g.G), g.G); }

// The most cells per side for P particles: the largest G with G^2 <= 8 P (at least 1, at most SBC_MAX_CELLS_PER_SIDE).  Eight
// cells a particle keep the counts a small multiple of the records (4 bytes a cell against 12 a record) while a scene spread
// over its bounds gets cells of the narrowest width the rule allows; coarser is always right.
static inline uint32_t sbc_cell_cap(uint32_t P)
{
    const uint64_t most = 8ull * std::max<uint32_t>(P, 1u);
    uint64_t g = 1;
    while ((g + 1) * (g + 1) <= most && g < SBC_MAX_CELLS_PER_SIDE) g++;
    return (uint32_t)g;
}

// false: the cell side is no ordinary number (G = 1, every pair is tested)
static inline bool sbc_geometry(const sb_engine *e, SbcGeo *geo)
{
    float cell = 1.0f;
    const uint32_t g = sb_batch_cell_geometry(e->prm.bounds_size, e->prm.particle_radius, sbc_cell_cap(e->P), &cell);
    geo->G = std::max(g, 1u);
    geo->cell = g ? cell : 1.0f;
    return g != 0u;
}
