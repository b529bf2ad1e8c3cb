"""Seeded fuzz cases of the batch's frame kernel (k_batch_frame): the hand-built scenes of batch_cases.py and
batch_grid_cases.py all run at bounds 1000, radius 10, 64 subticks and one of five capacities; these draw all of that.

case(sb, seed) is a batch_cases-style dict (bufs, layout, cap, mode, bounds, radius, subticks, program) with, besides,
  grid_min_particles   what BatchEngine gets (None: the build's default)
  expect               what the batch must report about itself, from the restatement of the host's formulas below
  expect_variant       (collide, materials in LDS): which of the six instances of the kernel the batch launches
  empty, never, clump, coincident, full_p, full_b    indices of the scenes of that kind (None: the case has none)
tests/test_batch_fuzz_cpu.py runs the oracle alone over every committed seed (every scene finite at every op; the family bites);
tests/test_gpu_batch_fuzz.py runs them through BatchEngine against one all-pairs oracle per scene, bit for bit."""
import functools
import os

import numpy as np

import batch_cases as bc
import batch_grid_cases as gc

F = np.float32
OFF, ALLPAIRS, GRID = bc.OFF, bc.ALLPAIRS, bc.GRID
BASE = 31000
NSEEDS = 24                      # the committed seeds: 0 .. NSEEDS - 1
# SB_FUZZ_OFFSET=n shifts every seed by n (a soak over other cases than the committed ones), SB_FUZZ_COUNT widens the run
SEED0 = int(os.environ.get("SB_FUZZ_OFFSET", "0"))
COUNT = int(os.environ.get("SB_FUZZ_COUNT", str(NSEEDS)))
NEVER = gc.NEVER
GRID_MIN_DEFAULT = 256           # SB_BATCH_GRID_MIN_PARTICLES_DEFAULT
MAX_PARTICLES, MAX_BEAMS = 1024, 4096                           # SB_BATCH_MAX_PARTICLES / _BEAMS
LDS_LIMIT = 160 * 1024           # SB_BATCH_LDS_LIMIT
MAT_ROW = 6                      # SB_BATCH_MAT_ROW
CELL_K = gc.CELL_K
NONE, WALK, CELLS = "none", "walk", "cells"                     # k_batch_frame's COLLIDE
VARIANTS = [(c, m) for c in (NONE, WALK, CELLS) for m in (True, False)]
BOUNDS, RADII, SUBTICKS = (700.0, 1000.0, 1600.0), (10.0, 7.5, 12.0), (64, 128, 48, 100, 63)
DRAG = [(0.0, 2.0), (0.002, 2.0), (0.002, 2.5), (0.00002, 3.0), (0.02, 1.0)]      # test_gpu_fuzz.py's table


# ---------------------------------------------------------------- sb_batch.hip / sb_batch.h, restated
def up16(x):
    return (x + 15) & ~15


def cdiv(a, b):
    return (a + b - 1) // b


def batch_threads(max_p, max_b):
    """sb_batch_threads: one per particle slot, at most four beams to a lane, whole waves, 64 .. 1024"""
    t = max(cdiv(max_p, 64) * 64, cdiv(cdiv(max_b, 4), 64) * 64)
    return min(max(t, 64), 1024)


def batch_lds_bytes(max_p, max_b, mats):
    """sb_batch_lds_bytes: positions and velocities twice, force sums, data index per particle; {target, last}, endpoint word, data
    index per beam; break flags and their prefix; the material rows"""
    nflagw = cdiv(max(max_b, 1), 32)
    return up16(max_p * (16 + 16 + 8 + 4) + max_b * (8 + 4 + 4) + (2 * nflagw + 1) * 4 + (max_b * MAT_ROW * 4 if mats else 0))


def batch_cell_lds_bytes(g):
    """sb_batch_cell_lds_bytes: u16 entries [g * g][K], two 16-bit counts to a word twice over, two overflow words"""
    return g * g * CELL_K * 2 + 2 * ((g * g + 1) // 2) * 4 + 8


def resolve(cap, mode, bounds, radius, grid_min_particles):
    """What sb_batch_create decides: the kernel's COLLIDE, the cells per side, whether the material rows are in LDS, the threads
    and the LDS bytes of a scene."""
    max_p, max_b = cap
    gmin = grid_min_particles or GRID_MIN_DEFAULT
    collide, g, cell_bytes = (NONE if mode == OFF else WALK), 0, 0
    if mode == GRID and gmin <= max_p:
        collide, g = CELLS, gc.cell_geometry(bounds, radius, max_p)[0]
        cell_bytes = up16(batch_cell_lds_bytes(g))
    mats = batch_lds_bytes(max_p, max_b, True) + cell_bytes <= LDS_LIMIT
    return dict(collide=collide, cells_per_side=g, materials_in_lds=mats, threads=batch_threads(max_p, max_b),
                lds_bytes=batch_lds_bytes(max_p, max_b, mats) + cell_bytes, grid_min_particles=gmin)


def mats_fit(max_p, max_b, cell_bytes):
    return batch_lds_bytes(max_p, max_b, True) + cell_bytes <= LDS_LIMIT


def last_fitting_beams(max_p, cell_bytes):
    """The largest max_beams at which the material rows still fit beside everything else (the formula grows with max_beams)."""
    fit = [b for b in range(MAX_BEAMS + 1) if mats_fit(max_p, b, cell_bytes)]
    assert fit and fit[-1] < MAX_BEAMS and fit == list(range(fit[-1] + 1))
    return fit[-1]


# (max_particles, max_beams); a max_beams of ("fit", d, cells) is the boundary capacity + d of a batch without / with cells, which
# for a batch with cells depends on the case's bounds and radius: case() resolves it.  The table is dealt by seed (seed modulo its
# length), so any run of len(TABLE) seeds has every row.
TABLE = [(37, 90), (64, 256), (65, 261), (200, 1000), (63, 700), (1024, 4096),
         (1024, ("fit", 0, False)), (1024, ("fit", 1, False)), (1024, ("fit", 0, True)), (1024, ("fit", 1, True))]


def capacity(row, bounds, radius):
    max_p, max_b = row
    if isinstance(max_b, tuple):
        cell_bytes = up16(batch_cell_lds_bytes(gc.cell_geometry(bounds, radius, max_p)[0])) if max_b[2] else 0
        max_b = last_fitting_beams(max_p, cell_bytes) + max_b[1]
    return max_p, max_b


# ---------------------------------------------------------------- scenes
def scatter(sb, layout, cap, particles, beams, rng, cross_first_pair=False):
    """batch_edit_cases.scatter at any capacity: particle and beam slots and data indices are independent draws.
    cross_first_pair: particles 0 and 1 get data indices in the opposite order of their slots."""
    max_p, max_b = cap
    P, B = len(particles), len(beams)
    D, S = rng.permutation(max_p)[:P], rng.permutation(P)
    if cross_first_pair and (S[0] < S[1]) == (D[0] < D[1]):
        D[[0, 1]] = D[[1, 0]]
    E, T = rng.permutation(max_b)[:B], rng.permutation(B)
    buf = sb.Buffers(layout, max_p, max_b)
    buf.particles[D, :particles.shape[1]] = particles
    buf.mapping[S] = D
    rec = beams.copy()
    rec["a"], rec["b"] = D[beams["a"].astype(np.int64)], D[beams["b"].astype(np.int64)]
    buf.beams[E] = rec
    buf.mapping[max_p + T] = E
    buf.particle_count, buf.beam_count = P, B
    return buf


class Geometry:
    def __init__(self, layout, bounds, radius, subticks):
        self.layout, self.bounds, self.radius = layout, bounds, radius
        self.u = radius / 10.0                                   # spacings and speeds scale with the radius
        # springs and dampers are integrated explicitly: what is stable at dt = 1 / 64 is scaled down for a longer substep
        self.soft = min(1.0, ((subticks + 1) // 2 * 2 / 64.0) ** 2)


def no_beams(sb, geo):
    return np.zeros(0, sb.layout.BEAM_DTYPE[geo.layout])


def blob(sb, geo, rng, w, h, origin, base=0, speed=30.0, material=None):
    """A w x h lattice with a drawn material (yield and break limits within reach, or out of it), jittered, thrown."""
    d = geo.radius * float(rng.uniform(2.4, 4.0))
    spring, damp, yld, limit = material or (float(rng.choice([1, 3, 50, 500])), float(rng.choice([10, 50, 700])),
                                            float(rng.choice([0.02, 0.05, 0.2, 2.0])), float(rng.choice([0.1, 0.12, 0.5, 1e9])))
    ox, oy = origin(w, h, d) if callable(origin) else origin
    p, b = sb.scenes.rectangle(ox, oy, d, w, h, spring * geo.soft, damp * geo.soft, yld, limit, base=base,
                               anti_diagonal=bool(rng.integers(0, 2)), layout=geo.layout)
    pv = np.zeros((len(p), 6), "f4")
    pv[:, :2] = p + rng.uniform(-1, 1, p.shape).astype("f4") * F(geo.u)
    pv[:, 2:4] = (rng.uniform(-speed, speed, 2) * geo.u).astype("f4")
    return pv, b, d


def anywhere(geo, rng):
    m = geo.radius + 10.0
    return lambda w, h, d: (rng.uniform(m, max(m + 1.0, geo.bounds - m - (w - 1) * d)), rng.uniform(m, max(m + 1.0, geo.bounds - m - (h - 1) * d)))


def blobs_scene(sb, geo, rng, max_p, max_b):
    """One to three blobs anywhere in the box (they may overlap the walls' reach and each other's)."""
    parts, beams = [], []
    for _ in range(int(rng.integers(1, 4))):
        w, h = int(rng.integers(2, 7)), int(rng.integers(2, 7))
        base = sum(len(p) for p in parts)
        if base + w * h > max_p:
            break
        pv, b, _ = blob(sb, geo, rng, w, h, anywhere(geo, rng), base=base, speed=40.0)
        if sum(len(x) for x in beams) + len(b) > max_b:
            break
        parts.append(pv)
        beams.append(b)
    if not parts:
        return cloud_scene(sb, geo, rng, max_p, max_b, False)
    return np.concatenate(parts), np.concatenate(beams)


def cloud_scene(sb, geo, rng, max_p, max_b, pair):
    """Free particles on a jittered grid (nobody overlaps at the start); pair: particles 0 and 1 on one spot."""
    g = geo.radius * float(rng.uniform(2.7, 4.5))
    side = int((geo.bounds - 4.0 * geo.radius) // g)
    n = int(rng.integers(min(12, max_p), min(max_p, 120, side * side) + 1))
    cells = rng.permutation(side * side)[:n]
    pv = np.zeros((n, 6), "f4")
    pv[:, 0] = 2.0 * geo.radius + (cells % side) * g + rng.uniform(-0.3, 0.3, n) * geo.radius
    pv[:, 1] = 2.0 * geo.radius + (cells // side) * g + rng.uniform(-0.3, 0.3, n) * geo.radius
    pv[:, 2:4] = rng.uniform(-1, 1, (n, 2)) * float(rng.choice([5.0, 30.0, 80.0])) * geo.u
    if pair:
        pv[1, :2] = pv[0, :2]
    return pv, no_beams(sb, geo)


def clump_scene(sb, geo, rng, max_p, max_b, cell):
    """A dense clump of free particles, five and more to a contact cell, dropped on a blob."""
    w, h = (int(rng.integers(3, 6)), int(rng.integers(2, 4))) if max_p >= 60 else (3, 2)
    ox, oy = rng.uniform(0.2, 0.6) * geo.bounds, rng.uniform(0.1, 0.4) * geo.bounds
    pv, b, d = blob(sb, geo, rng, w, h, (ox, oy), speed=5.0, material=(50.0, 700.0, 0.2, 0.5))
    if len(b) > max_b:
        b = b[:max_b]
    n = int(min(max_p - len(pv), rng.integers(10, 25)))
    # about six to a cell, and, where the cells are coarse, still close enough for half a dozen contacts each
    side = max(min(float(cell) * np.sqrt(n / 6.0), 1.45 * geo.radius * np.sqrt(n)), 1.2 * geo.radius)
    cv = np.zeros((n, 6), "f4")
    cv[:, 0] = ox + 0.5 * (w - 1) * d - 0.5 * side + side * rng.random(n)
    cv[:, 1] = oy + (h - 1) * d + 2.2 * geo.radius + side * rng.random(n)
    cv[:, 3] = -10.0 * geo.u
    return np.concatenate([pv, cv]), b


def full_dims(max_p):
    h = int(np.floor(np.sqrt(max_p)))
    return max_p // h, h


def full_p_scene(sb, geo, rng, max_p, max_b):
    """Exactly max_particles: the widest lattice that fits them, the rest free in a row above it; beams past max_beams left out."""
    w, h = full_dims(max_p)
    d = min(2.5 * geo.radius, (geo.bounds - 4.0 * geo.radius - 20.0) / (max(w, h + 1)))
    assert d >= 2.05 * geo.radius, (max_p, geo.bounds, geo.radius)
    o = 2.0 * geo.radius + 5.0
    p, b = sb.scenes.rectangle(o, o, d, w, h, 50.0 * geo.soft, 700.0 * geo.soft, 0.2, 0.5, anti_diagonal=False, layout=geo.layout)
    rest = max_p - w * h
    row = np.stack([o + d * np.arange(rest), np.full(rest, o + d * h)], axis=1).reshape(rest, 2)
    pv = np.zeros((max_p, 6), "f4")
    pv[:, :2] = np.concatenate([p, row.astype("f4")]) + rng.uniform(-0.5, 0.5, (max_p, 2)).astype("f4") * F(geo.u)
    pv[:, 2:4] = (rng.uniform(-10, 10, 2) * geo.u).astype("f4")
    return pv, b[:max_b]


def full_b_scene(sb, geo, rng, max_p, max_b):
    """Exactly max_beams: a lattice of at most 200 particles, then soft beams between drawn pairs at their present distance."""
    w, h = full_dims(min(max_p, 200))
    pv, b, d = blob(sb, geo, rng, w, h, anywhere(geo, rng), speed=10.0, material=(50.0, 700.0, 0.2, 0.5))
    b = b[:max_b]
    extra = np.zeros(max_b - len(b), b.dtype)
    if len(extra):
        ia = rng.integers(0, w * h - 1, len(extra))
        ib = ia + 1 + rng.integers(0, w * h - 1 - ia)
        dx, dy = pv[ib, 0] - pv[ia, 0], pv[ib, 1] - pv[ia, 1]
        ln = np.sqrt(dx * dx + dy * dy, dtype=np.float32)
        extra["a"], extra["b"] = ia, ib
        for f, v in (("length", ln), ("target_length", ln), ("last_length", ln), ("spring", 1.0 * geo.soft), ("damp", 10.0 * geo.soft),
                     ("yield_strain", 2.0), ("strain_break_limit", 1e9)):
            extra[f] = v
    return pv, np.concatenate([b, extra])


def draw_consts(rng, calm=False):
    """test_gpu_fuzz.make_case's constants; calm: exponent 2 only (a clump bursts: its speeds are no place for v^3)."""
    drag_coeff, drag_exp = DRAG[int(rng.integers(0, 2 if calm else 5))]
    return np.array([rng.uniform(-0.3, 0.3), rng.uniform(-1.0, 0.2), rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0, 1),
                     rng.uniform(0, 1), drag_coeff, drag_exp], "f4")


def draw_input(sb, geo, rng, mouse=None):
    b = sb.Buffers(1, 4, 4)
    b.user_strength = float(rng.uniform(0.5, 2.0))
    b.set_user_input(applied_force=tuple(rng.uniform(-0.3, 0.3, 2)), mouse_pos=tuple(rng.uniform(0, geo.bounds, 2)),
                     mouse_vel=tuple(rng.uniform(-5, 5, 2)), mouse_active=bool(rng.integers(0, 3) == 0) if mouse is None else mouse)
    return b.user_input_bytes()


def draw_program(sb, geo, rng, n_scenes, subticks, calm):
    """Six to ten ops, at most about four frames' worth of substeps, a frame among them."""
    st = (subticks + 1) // 2 * 2
    budget, ops = 3 * st, []                                     # (the fourth frame's worth: the frame that is always there)
    kinds = [str(k) for k in rng.choice(["frame", "step", "step", "delete", "consts", "inputs", "input"], int(rng.integers(5, 10)))]
    kinds.insert(int(rng.integers(0, len(kinds) + 1)), "one frame")
    for kind in kinds:
        if kind == "one frame":
            ops.append(("frame", 1))
        if kind == "frame":
            n = int(rng.integers(1, 3))
            if n * st > budget:
                kind = "step"
            else:
                ops.append(("frame", n))
                budget -= n * st
        if kind == "step":
            n = int([1, st - 1, 2 * int(rng.integers(1, st // 2)), 1 + 2 * int(rng.integers(0, st // 2))][int(rng.integers(0, 4))])
            n = min(n, budget)
            if n == 0:
                kind = "delete"
            else:
                ops.append(("step", n))
                budget -= n
        if kind == "delete":
            ops.append(("delete",))
        elif kind == "consts":
            i = int(rng.integers(0, n_scenes))
            ops.append(("consts", i, draw_consts(rng, calm=i in calm)))
        elif kind == "inputs":
            ops.append(("inputs", [draw_input(sb, geo, rng, mouse=False if i in calm else None) for i in range(n_scenes)]))
        elif kind == "input":
            ops.append(("input", draw_input(sb, geo, rng, mouse=False)))
    return ops


@functools.lru_cache(maxsize=None)
def _case(sb, seed):
    rng = np.random.default_rng(BASE + seed)
    row = TABLE[seed % len(TABLE)]
    max_p = row[0]
    with_cells = row[1][2] if isinstance(row[1], tuple) else None
    # 1024 discs of radius 12 do not fit a box of 700: the limit capacity draws from the larger boxes
    bounds = float(rng.choice(BOUNDS[1:] if max_p == MAX_PARTICLES else BOUNDS))
    radius = float(rng.choice(RADII))
    subticks = int(rng.choice(SUBTICKS))
    layout = int(rng.integers(1, 3))
    cap = capacity(row, bounds, radius)
    mode = int(rng.choice([OFF, ALLPAIRS, GRID, GRID]))
    if with_cells is not None:
        # (the boundary without cells is dealt its three modes in turn: any run of 3 * len(TABLE) seeds has all six variants)
        mode = GRID if with_cells else [OFF, ALLPAIRS, GRID][seed // len(TABLE) % 3]
    geo = Geometry(layout, bounds, radius, subticks)

    kinds = ["full_p", "full_b", "empty", "never", "cloud", "clump" if mode == GRID else "blobs"]
    kinds += [str(k) for k in rng.choice(["blobs", "blobs", "cloud"], int(rng.integers(8, 13)) - len(kinds))]
    kinds = [kinds[i] for i in rng.permutation(len(kinds))]
    pair = bool(rng.integers(0, 3) == 0)
    cell = gc.cell_geometry(bounds, radius, max_p)[1]
    bufs, where = [], {}
    for i, kind in enumerate(kinds):
        where.setdefault(kind, i)
        first = where[kind] == i
        if kind == "never":
            bufs.append(None)
            continue
        if kind == "empty":
            pv, b = np.zeros((0, 6), "f4"), no_beams(sb, geo)
        elif kind == "cloud":
            pv, b = cloud_scene(sb, geo, rng, *cap, pair and first)
        elif kind == "blobs":
            pv, b = blobs_scene(sb, geo, rng, min(cap[0], 200), cap[1])
        else:
            pv, b = dict(clump=lambda *a: clump_scene(*a, cell), full_p=full_p_scene, full_b=full_b_scene)[kind](sb, geo, rng, *cap)
        buf = scatter(sb, layout, cap, pv, b, rng, cross_first_pair=kind == "cloud" and pair and first)
        c = draw_consts(rng, calm=kind == "clump")
        buf.set_physics_constants(gravity=(c[0], c[1]), border_elasticity=c[2], border_friction=c[3], elasticity=c[4], friction=c[5],
                                  drag_coeff=c[6], drag_exp=c[7])
        buf.metadata[20:28] = np.frombuffer(draw_input(sb, geo, rng, mouse=False if kind == "clump" else None), "<u4")
        bufs.append(buf)

    counts = sorted(b.particle_count for b in bufs if b is not None and b.particle_count)
    gmin = None
    if mode == GRID:
        between = bufs[where["clump"]].particle_count            # between the smallest and the largest scene: the clump takes the cells
        assert counts[0] <= between <= counts[-1]
        gmin = [1, between, None, between if with_cells else NEVER][int(rng.integers(0, 4))]
        if with_cells is False:
            gmin = NEVER
    expect = resolve(cap, mode, bounds, radius, gmin)
    assert with_cells is None or (expect["collide"] == CELLS) == with_cells
    calm = {where["clump"]} if mode == GRID else set()
    return dict(name="fuzz %d" % seed, seed=seed, bufs=bufs, layout=layout, cap=cap, mode=mode, bounds=bounds, radius=radius,
                subticks=subticks, grid_min_particles=gmin, expect=expect, expect_variant=(expect["collide"], expect["materials_in_lds"]),
                program=draw_program(sb, geo, rng, len(bufs), subticks, calm), kinds=kinds, empty=where["empty"], never=where["never"],
                clump=where.get("clump"), coincident=where["cloud"] if pair else None, full_p=where["full_p"], full_b=where["full_b"])


def case(sb, seed):
    return _case(sb, seed)


def takes_cells(case, i):
    """Does scene i of the case step on the contact cells?"""
    b = case["bufs"][i]
    return case["expect"]["collide"] == CELLS and b is not None and b.particle_count >= case["expect"]["grid_min_particles"]


def make_oracle(orc, case, buf):
    """As batch_grid_cases.make_oracle: ALLPAIRS always, with the case's bounds, radius and subticks (or none: collisions off)."""
    ref = orc.OracleEngine(case["bounds"], case["radius"], case["subticks"], case["layout"], ALLPAIRS if case["mode"] else OFF, threads=4)
    ref.write_buffers(buf)
    return ref


def live_particles(ref):
    """The oracle's current particle rows, in slot order."""
    cur = ref.particles_b if ref.final_in_b else ref.particles_a
    return cur[ref.mapping[:int(ref.metadata[1])].astype(np.int64)]
