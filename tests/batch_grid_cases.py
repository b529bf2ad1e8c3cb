"""Scenes of the batch's contact cells (SB_COLLIDE_GRID in a BatchEngine), each small and chosen to break a grid.

Cases are batch_cases' dicts, with two optional keys more: `bounds`, `radius` (default 1000 / 10).  tests/test_batch_grid_cpu.py
shows on the oracle alone that the cases bite (contacts, more than one selection sweep, full cells); tests/test_gpu_batch_grid.py
runs them through BatchEngine against one all-pairs OracleEngine per scene, bit for bit.
"""
import numpy as np

import batch_cases as bc

F = np.float32
CELL_K = 4                       # info("contact_cell_capacity")
NEVER = 0xFFFFFFFF               # grid_min_particles: no scene takes the cells
PILE_SEED = 12                   # the oracle stays finite with it (half of the seeds 0 .. 29 burst to NaN); test_the_pile_bites asserts the rest


def cell_rule(radius):
    """The narrowest cell: 2r (1 + 1/64), in float32 as the library computes it."""
    return F(F(radius) * F(2.0)) * F(1.0 + 1.0 / 64.0)


def cell_cap(max_particles):
    """The documented cap on cells per side: the largest G with G^2 <= 2.5 max_particles."""
    g = 1
    while 2 * (g + 1) * (g + 1) <= 5 * max_particles:
        g += 1
    return g


def cell_geometry(bounds, radius, max_particles):
    """(G, cell side) of a batch, float32 step by step as documented: G = clamp(floor(bounds / rule), 1, cap); the side is
    bounds / G, never below the rule."""
    rule, cap = cell_rule(radius), cell_cap(max_particles)
    per_side = F(bounds) / rule
    g = cap if per_side >= F(cap) else (int(per_side) if per_side >= F(1.0) else 1)
    return g, max(rule, F(bounds) / F(g))


def free_particles(sb, layout, cap, pts, data_index=None):
    """Free particles (no beams); data_index: the data index of each slot (None: the identity)."""
    pts = np.asarray(pts, "f4")
    buf = sb.Buffers(layout, *cap)
    if data_index is None:
        buf.set_scene(pts, np.zeros(0, sb.layout.BEAM_DTYPE[layout]))
        return buf
    data_index = np.asarray(data_index)
    assert len(set(data_index.tolist())) == len(pts) and data_index.max() < cap[0]
    buf.particles[data_index, :pts.shape[1]] = pts
    buf.mapping[:len(pts)] = data_index
    buf.particle_count, buf.beam_count = len(pts), 0
    return buf


# ---------------------------------------------------------------- the pile
def pile_buffers(sb, seed=PILE_SEED, cap=(256, 0)):
    """256 free discs of radius 10 drawn into a 150 x 150 patch in the corner of the floor and the left wall: on average 4.7 to
    a cell of the narrowest side, every disc overlapping a dozen others."""
    rng = np.random.default_rng(seed)
    pts = np.zeros((256, 6), "f4")
    pts[:, :2] = 10.0 + 150.0 * rng.random((256, 2))
    return free_particles(sb, 2, cap, pts)


def case_pile(sb):
    return dict(name="pile", layout=2, cap=(256, 0), mode=bc.ALLPAIRS, bufs=[pile_buffers(sb)], program=[("frame", 1), ("step", 5)])


# ---------------------------------------------------------------- cell edges
EDGE_CAP = (1024, 64)            # 49 cells per side at bounds 1000 / radius 10: the cap (50) is not in the way


def edge_points():
    """(points, data index per slot) around the borders of the 49 x 49 grid of EDGE_CAP."""
    g, cell = cell_geometry(1000.0, 10.0, EDGE_CAP[0])
    assert g == 49
    up, dn = (lambda v: np.nextafter(F(v), F(np.inf))), (lambda v: np.nextafter(F(v), F(-np.inf)))
    pts = []
    # on multiples of the cell side and one ulp either side, in x and in y; 25 apart along the other axis: no contacts
    for n, k in enumerate((1, 7, 24, 48)):
        b = F(k) * cell
        for m, v in enumerate((dn(b), b, up(b))):
            pts.append((v, 300.0 + 100.0 * n + 25.0 * m))
            pts.append((500.0 + 100.0 * n + 25.0 * m - 400.0 * (n >= 2), v if k != 48 else dn(dn(v))))
    # pairs across the border between cells 9 and 10 at distance 2r - ulp, 2r, 2r + ulp (ulp of the coordinate), in x, then in y
    b = F(10) * cell
    a0 = b - F(10.0)
    assert F(a0 + F(20.0)) - a0 == F(20.0)
    for m, far in enumerate((dn(a0 + F(20.0)), a0 + F(20.0), up(a0 + F(20.0)))):
        pts += [(a0, 40.0 + 40.0 * m), (far, 40.0 + 40.0 * m)]
        pts += [(700.0 + 40.0 * m, a0), (700.0 + 40.0 * m, far)]
    # on the walls, the floor and the ceiling
    pts += [(0.0, 250.0), (1000.0, 250.0), (0.0, 262.0), (1000.0, 262.0), (450.0, 0.0), (450.0, 1000.0), (0.0, 0.0), (1000.0, 1000.0)]
    # six on one spot, and a neighbour within reach in the next cell
    spot = (F(20) * cell + F(3.0), F(30) * cell + F(3.0))
    pts += [spot] * 6 + [(spot[0] - F(9.0), spot[1])]
    rng = np.random.default_rng(11)
    return np.array(pts, "f4"), rng.permutation(EDGE_CAP[0])[:len(pts)]


def case_edges(sb):
    pts6 = np.zeros((len(edge_points()[0]), 6), "f4")
    pts6[:, :2], idx = edge_points()
    return dict(name="cell edges", layout=2, cap=EDGE_CAP, mode=bc.ALLPAIRS, bufs=[free_particles(sb, 2, EDGE_CAP, pts6, idx)],
                program=[("step", 1), ("step", 2), ("frame", 1)])


# ---------------------------------------------------------------- out of range
def case_out_of_range(sb):
    """A dozen ordinary particles (some touching) and one each at NaN, +inf, -inf, -50 and bounds + 50; step(3)."""
    pts = np.zeros((17, 6), "f4")
    pts[:12, 0] = 400.0 + 17.0 * (np.arange(12) % 4)
    pts[:12, 1] = 300.0 + 18.0 * (np.arange(12) // 4)
    pts[12:, 0] = (np.nan, np.inf, -np.inf, -50.0, 1050.0)
    pts[12:, 1] = (500.0, 520.0, np.nan, 1050.0, -50.0)
    return dict(name="out of range", layout=2, cap=EDGE_CAP, mode=bc.ALLPAIRS, bufs=[free_particles(sb, 2, EDGE_CAP, pts)],
                program=[("step", 3)], finite=False)


# ---------------------------------------------------------------- geometries
R_INTEGER = 1000.0 / (2.0 * (1.0 + 1.0 / 64.0) * 40.0)      # bounds / cell lands on an integer
GEOMETRIES = [(1000.0, 10.0), (1000.0, 0.5), (1000.0, 600.0), (100.0, 10.0), (1000.0, R_INTEGER)]
GEOMETRY_CAP = (256, 512)


def thrown_lattice(sb, cap=GEOMETRY_CAP, velocity=(-40.0, -35.0)):
    """batch_cases.case_break's 12 x 12 lattice (v1, slack 8), thrown at the corner."""
    src = sb.scenes.lattice_buffers(12, 12, d=30.0, origin=(30.0, 30.0), spring=50.0, damp=100.0, yield_strain=0.05,
                                    strain_limit=0.12, layout=1, velocity=velocity, slack=8)
    return bc.fit(sb, src, *cap)


# The lattice spans 30 .. 360: a box of 100 squeezes its 144 discs of radius 10 against the far walls, and a disc of radius 600 is
# wider than its box.  Both burst: the oracle's state is finite for 8 / 3 substeps and has NaNs soon after (64 / 8 substeps),
# and a NaN that arithmetic GENERATES has the sign bit set on the oracle's CPU and clear on the GPU, in every collision mode.  So
# these two run for as long as the state is finite; the others a frame and three substeps.
SUBSTEPS_WHILE_FINITE = {(1000.0, 600.0): 3, (100.0, 10.0): 8}


def case_geometry(sb, bounds, radius):
    short = SUBSTEPS_WHILE_FINITE.get((bounds, radius))
    return dict(name="geometry %g / %g" % (bounds, radius), layout=1, cap=GEOMETRY_CAP, mode=bc.ALLPAIRS, bounds=bounds, radius=radius,
                bufs=[thrown_lattice(sb)], program=[("step", 1), ("step", short - 1)] if short else [("frame", 1), ("step", 3)])


def lattice_at_rest(sb, cap=GEOMETRY_CAP):
    """12 x 12, spacing 30, in mid-air, at rest: at most one particle to a cell for as long as it falls."""
    return bc.fit(sb, sb.scenes.lattice_buffers(12, 12, d=30.0, origin=(300.0, 500.0), strain_limit=0.5, layout=1), *cap)


def case_rest(sb):
    return dict(name="lattice at rest", layout=1, cap=GEOMETRY_CAP, mode=bc.ALLPAIRS, bufs=[lattice_at_rest(sb)], program=[("step", 16)])


# ---------------------------------------------------------------- mixed sizes
def case_mixed(sb):
    """Scenes of 2, 119, 144 and 1024 particles in one batch (the threshold test: grid_min_particles = 128)."""
    cap, L = (1024, 4096), 2
    h = bc.case_hetero(sb)["bufs"]
    bufs = [bc.two_particles(sb, L, cap, vx=4.0), h[0], h[1], h[2]]
    assert [b.particle_count for b in bufs] == [2, 119, 144, 1024]
    return dict(name="mixed sizes", layout=L, cap=cap, mode=bc.ALLPAIRS, bufs=bufs, program=[("frame", 1), ("step", 7)])


# ---------------------------------------------------------------- rings
RING_CAP = (64, 0)               # 12 cells per side, 83.3 wide, at bounds 1000 / radius 10: a whole ring fits into one
RING_PARTNERS = (0, 1, 3, 4, 5, 7, 8, 9)         # around 4 and 8: where a selection sweep that comes back full was the last
RING_RADIUS = 19.9               # just inside 2r


def ring_points(k, crowded=False, seed=0):
    """(points, slot of the centre): a centre with k partners RING_RADIUS away, evenly around it from 0.35 rad on.  The centre sits
    one unit beside the corner of four cells, so the ring spreads over them and none holds more than four; crowded: in the middle
    of a cell, which then holds all k + 1.  Slots are shuffled: the partners' order in a cell is not their indices'."""
    cell = cell_geometry(1000.0, 10.0, RING_CAP[0])[1]
    c = float(cell) * (4.5 if crowded else 4.0) + (0.0 if crowded else 1.0)
    ang = 0.35 + 2.0 * np.pi * np.arange(k) / max(k, 1)
    pts = np.array([(c, c)] + [(c + RING_RADIUS * np.cos(a), c + RING_RADIUS * np.sin(a)) for a in ang], "f4")
    order = np.random.default_rng(40 + seed).permutation(k + 1)
    return pts[order], int(np.nonzero(order == 0)[0][0])


def ring_scenes():
    """[(k, crowded)] of case_rings' scenes, in order."""
    return [(k, False) for k in RING_PARTNERS] + [(max(RING_PARTNERS), True)]


def case_rings(sb):
    """Eight scenes of a centre with 0 .. 9 partners spread over four cells (the cells' path), and the fullest ring once more
    inside one cell (the overflow's); tests/test_batch_grid_cpu.py asserts the counts and the cells' load."""
    bufs = []
    for n, (k, crowded) in enumerate(ring_scenes()):
        pts6 = np.zeros((k + 1, 6), "f4")
        pts6[:, :2] = ring_points(k, crowded, n)[0]
        bufs.append(free_particles(sb, 2, RING_CAP, pts6, np.random.default_rng(60 + n).permutation(RING_CAP[0])[:k + 1]))
    return dict(name="rings", layout=2, cap=RING_CAP, mode=bc.ALLPAIRS, bufs=bufs, program=[("step", 1), ("step", 3)])


def substeps_of(program, subticks=64):
    return sum(op[1] * subticks if op[0] == "frame" else op[1] if op[0] == "step" else 0 for op in program)


def finite_cases(sb):
    return [case_pile(sb), case_edges(sb), case_rest(sb), case_mixed(sb), case_rings(sb)] + [case_geometry(sb, b, r) for b, r in GEOMETRIES]


def make_oracle(orc, case, buf):
    """batch_cases.make_oracle with the case's own bounds and radius: ALLPAIRS, always."""
    ref = orc.OracleEngine(case.get("bounds", 1000.0), case.get("radius", 10.0), case.get("subticks", 64), case["layout"],
                           bc.ALLPAIRS, threads=4)
    ref.write_buffers(buf)
    return ref


def run_oracles(orc, case, checkpoint=None):
    refs = [make_oracle(orc, case, b) for b in case["bufs"]]
    for k, op in enumerate(case["program"]):
        bc.apply_to_oracles(refs, op)
        if checkpoint:
            checkpoint(refs, k)
    return refs


def positions(ref):
    """Current positions of an oracle's particles, in SLOT order."""
    cur = ref.particles_b if ref.final_in_b else ref.particles_a
    return cur[ref.mapping[:int(ref.metadata[1])].astype(np.int64), :2]
