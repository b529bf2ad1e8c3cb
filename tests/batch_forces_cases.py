"""Scenes of the forces tests (sb_batch_forces_device).  A case is tests/batch_cases.py's dict (bufs, layout, cap,
mode, subticks) with an optional `grid_min_particles`.  tests/test_batch_forces_cpu.py shows on the restatement and the oracle
alone that the cases bite; tests/test_gpu_batch_forces.py runs them through BatchEngine.forces()."""
import numpy as np

import batch_cases as bc
import batch_contacts_cases as cs
import batch_grid_cases as gc

F = np.float32
L = 2                            # layout of every scene here
GRID_MIN = 16                    # grid_min_particles of the contact cases: P = 15 walks, P = 16 takes the cells


def up(v):
    return np.nextafter(F(v), F(np.inf))


def dn(v):
    return np.nextafter(F(v), F(-np.inf))


def scene(sb, cap, pts, beams=(), data_index=None, consts=None):
    """pts: rows of 2, 4 or 6 floats; beams: (a, b, length, target, last, spring, damp[, yield, limit]) with a, b SLOTS of `pts`;
    data_index: the data index of each particle slot (None: the identity); beams sit at the head of the beam buffer."""
    pts = np.asarray(pts, "f4")
    n = len(pts)
    buf = sb.Buffers(L, *cap)
    d = np.arange(n) if data_index is None else np.asarray(data_index)
    assert len(set(d.tolist())) == n and (n == 0 or d.max() < cap[0]) and len(beams) <= cap[1]
    buf.particles[d, :pts.shape[1]] = pts
    buf.mapping[:n] = d
    for j, bm in enumerate(beams):
        rec = buf.beams[j]
        rec["a"], rec["b"] = d[bm[0]], d[bm[1]]
        for f, v in zip(("length", "target_length", "last_length", "spring", "damp"), bm[2:7]):
            rec[f] = v
        rec["yield_strain"], rec["strain_break_limit"] = (bm[7], bm[8]) if len(bm) > 7 else (5.0, 50.0)
        buf.beams[j] = rec
        buf.mapping[cap[0] + j] = j
    buf.particle_count, buf.beam_count = n, len(beams)
    if consts:
        buf.set_physics_constants(**dict(sb.layout.DEFAULT_CONSTANTS, **consts))
    return buf


def recap(sb, src, cap):
    """`src` in Buffers of a larger capacity: the same data indices, slots, constants and user input."""
    P, B, mp, mb = src.particle_count, src.beam_count, src.max_particles, src.max_beams
    assert cap[0] >= mp and cap[1] >= mb
    out = sb.Buffers(src.layout, *cap)
    out.particles[:mp], out.beams[:mb] = src.particles, src.beams
    out.mapping[:P], out.mapping[cap[0]:cap[0] + B] = src.mapping[:P], src.mapping[mp:mp + B]
    out.particle_count, out.beam_count = P, B
    out.metadata[12:28] = src.metadata[12:28]
    return out


def case(name, cap, bufs, **kw):
    return dict(dict(name=name, layout=L, cap=cap, mode=bc.ALLPAIRS, bufs=bufs, program=[]), **kw)


# ---------------------------------------------------------------- beams
def hand_scene(sb):
    """Two particles 40 apart along x and one beam of rest length 30, spring 2, damp 0.5, last_length 38: worked out by hand in
    tests/test_batch_forces_cpu.py."""
    return scene(sb, (8, 8), [(100.0, 200.0), (140.0, 200.0)], [(0, 1, 30.0, 30.0, 38.0, 2.0, 0.5)], data_index=[5, 2])


def beam_kinds(sb):
    """A stretched, a compressed and an at-rest beam (its endpoints exactly its length apart), oblique and far from one another."""
    pts = [(100.0, 100.0), (130.0, 140.0), (300.0, 100.0), (318.0, 124.0), (500.0, 100.0), (515.0, 120.0)]
    beams = [(0, 1, 40.0, 40.0, 45.0, 50.0, 700.0), (2, 3, 35.0, 35.0, 31.0, 3.0, 50.0), (4, 5, 25.0, 25.0, 25.0, 500.0, 800.0)]
    return scene(sb, (8, 8), pts, beams, data_index=[7, 0, 3, 6, 1, 4])


def star(sb, spring):
    """64 beams on particle slot 0: 63 particles in a fan to its right (all pull it the same way), the last one joined twice.
    spring 20: each contribution is near 2^27, the sum wraps past 2^31; spring 1e9: every contribution saturates."""
    ang = np.linspace(-1.0, 1.0, 63)
    rad = np.where(np.arange(63) % 2, 300.0, 345.0)
    pts = [(300.0, 500.0)] + [(300.0 + r * np.cos(a), 500.0 + r * np.sin(a)) for a, r in zip(ang, rad)]
    beams = [(0, 1 + k % 63, 250.0, 250.0, 250.0, spring, 0.0) for k in range(64)]
    rng = np.random.default_rng(7)
    return scene(sb, (64, 64), pts, beams, data_index=rng.permutation(64))


def odd_beams(sb):
    """A beam of length zero with an ordinary spring; a NaN endpoint (conversion gives 0, counted as not finite); one saturating
    beam along x (INT_MAX on one side, INT_MIN on the other)."""
    pts = [(100.0, 100.0), (100.0, 100.0), (300.0, 300.0), (np.nan, 340.0), (500.0, 500.0), (620.0, 500.0)]
    beams = [(0, 1, 30.0, 30.0, 30.0, 50.0, 700.0), (2, 3, 30.0, 30.0, 30.0, 50.0, 700.0), (4, 5, 100.0, 100.0, 100.0, 1e9, 0.0)]
    return scene(sb, (8, 8), pts, beams)


def case_beams(sb):
    return case("beam kinds, stars, odd beams", (64, 64), [recap(sb, hand_scene(sb), (64, 64)), recap(sb, beam_kinds(sb), (64, 64)), star(sb, 20.0),
                                                           star(sb, 1e9), recap(sb, odd_beams(sb), (64, 64)),
                                                           recap(sb, bc.saturation_scene(sb), (64, 64))], mode=bc.OFF)


def case_small(sb):
    """Capacity 8 / 8: the hand scene (permuted data indices), the beam kinds, the odd beams, batch_cases' saturation scene."""
    return case("capacity 8", (8, 8), [hand_scene(sb), beam_kinds(sb), odd_beams(sb), bc.saturation_scene(sb)], mode=bc.OFF)


MATERIAL_CAPS = ((128, 320), (1024, 4096))     # info("materials_in_lds") is 1 at the first and 0 at the second


def case_materials(sb, cap):
    """The reference's default scene (six materials), blown up by 2 % so that every beam is stretched, at a capacity on either
    side of the frame kernel's materials_in_lds limit."""
    buf = sb.scenes.default_buffers(L, *cap)
    buf.particles[:, :2] *= F(1.02)
    return case("default scene at %d / %d" % cap, cap, [buf])


# ---------------------------------------------------------------- contacts
def five_partners():
    """Slot 0 in the middle of five partners whose overlaps span three orders of magnitude, in an order of slots that is neither
    ascending nor descending in overlap: the float sums depend on the order.  (x, y, vx, vy)"""
    c = (500.0, 500.0)
    pts = [c + (0.3, -0.2)]
    for dist, a, v in ((19.99, 0.3, (0.5, 0.1)), (3.0, 2.1, (-0.2, 0.4)), (12.7, 3.9, (0.0, -0.6)), (0.011, 5.2, (0.7, 0.7)), (17.3, 1.2, (-0.9, 0.2))):
        pts.append((c[0] + dist * np.cos(a), c[1] + dist * np.sin(a)) + v)
    return pts


CONTACT_CAP = (1024, 64)         # 49 cells per side of 20.4 at bounds 1000 / radius 10 (at 64 particles a cell is 83 wide)


def contact_zoo(sb, n_extra=0, cap=CONTACT_CAP, consts=None):
    """The five partners (moving, so impulse is not zero); a pair exactly 2r apart (absent) and one an ulp closer (present), in x
    and in y; a pair on one spot; n_extra lone particles far away (to set P)."""
    pts = five_partners()
    pts += [(100.0, 100.0, 1.0, 0.0), (120.0, 100.0, -1.0, 0.0), (100.0, 200.0, 1.0, 0.5), (dn(120.0), 200.0, -1.0, 0.0)]
    pts += [(700.0, 100.0, 0.0, 1.0), (700.0, 120.0, 0.0, -1.0), (800.0, 100.0, 0.0, 1.0), (800.0, dn(120.0), 0.25, -1.0)]
    pts += [(300.0, 700.0, 2.0, 0.0), (300.0, 700.0, -2.0, 1.0)]
    assert len(pts) == 16 - 0 and n_extra >= -1
    pts = pts[:len(pts) + min(n_extra, 0)]                    # (-1: drop the last particle, the partner on the spot)
    pts += [(50.0 + 40.0 * k, 900.0, 0.0, 0.0) for k in range(max(n_extra, 0))]
    rng = np.random.default_rng(11)
    return scene(sb, cap, pts, data_index=rng.permutation(cap[0])[:len(pts)], consts=consts)


def crowded_cell(sb, cap=CONTACT_CAP):
    """Five particles inside one cell (the cells hold four): the workgroup falls back to the loop; eleven more elsewhere."""
    pts = [(492.0 + 3.0 * k, 492.0 + 2.0 * (k % 2), 0.1 * k, -0.2) for k in range(5)]
    pts += [(60.0 + 45.0 * k, 300.0 + 7.0 * (k % 3), 0.0, 0.3) for k in range(11)]
    return scene(sb, cap, pts)


def case_contacts(sb, subticks=64):
    """P = 16 (the cells), 15 (the loop), 20, a crowded cell (the fallback), friction and elasticity other than the defaults."""
    bufs = [contact_zoo(sb), contact_zoo(sb, -1), contact_zoo(sb, 4), crowded_cell(sb),
            contact_zoo(sb, 2, consts=dict(friction=0.7, elasticity=0.9))]
    return case("contact zoo, subticks %d" % subticks, CONTACT_CAP, bufs, subticks=subticks, grid_min_particles=GRID_MIN)


def case_rings(sb):
    """tests/batch_grid_cases.py's rings, every scene on the cells: a centre with 0, 1, 3, 4, 5, 7, 8 and 9 partners spread over
    four cells, and the fullest ring once more inside one cell (the fallback)."""
    return dict(gc.case_rings(sb), grid_min_particles=1)


def case_two_bodies(sb):
    """tests/batch_contacts_cases.py's two lattices pressed together: spacing 15 inside a body (every particle touches its own
    body: the self-contact that other_body leaves out), 18 between them."""
    return case("two bodies pressed together", cs.TWO_BODIES_CAP, [cs.two_bodies(sb)[0], bc.empty_scene(sb, L, cs.TWO_BODIES_CAP)])


def _refit(sb, src, cap):
    """`src` in Buffers of a smaller capacity, its particles in slot order at the identity mapping (velocities kept)."""
    P = src.particle_count
    return scene(sb, cap, src.particles[src.mapping[:P].astype(int), :4])


def case_mixed(sb):
    """Twelve scenes of different sizes in one batch, a never-uploaded and an empty one among them."""
    cap = (128, 320)
    lat = sb.scenes.lattice_buffers(8, 8, d=18.0, origin=(100.0, 300.0), strain_limit=0.5, layout=L, velocity=(3.0, -2.0), jitter=1.0)
    bufs = [sb.scenes.default_buffers(L, *cap), None, bc.fit(sb, lat, *cap), bc.empty_scene(sb, L, cap), bc.two_particles(sb, L, cap, vx=4.0),
            _refit(sb, contact_zoo(sb), cap), recap(sb, star(sb, 20.0), cap), recap(sb, beam_kinds(sb), cap), _refit(sb, crowded_cell(sb), cap),
            recap(sb, odd_beams(sb), cap), _refit(sb, contact_zoo(sb, 30), cap), recap(sb, cs.two_bodies(sb)[0], cap)]
    assert len(bufs) == 12
    return case("twelve mixed scenes", cap, bufs, grid_min_particles=GRID_MIN)


def case_full_width(sb):
    """Two scenes at 1024 / 4096: a 32 x 32 lattice of spacing 19 (below 2r: every particle touches its neighbours), jittered."""
    cap = (1024, 4096)
    bufs = []
    for seed in (1, 2):
        lat = sb.scenes.lattice_buffers(32, 32, d=19.0, origin=(100.0, 100.0), spring=50.0, damp=700.0, yield_strain=0.2, strain_limit=0.5,
                                        jitter=1.5, layout=L, velocity=(0.5 * seed, -0.25))
        assert lat.particle_count == 1024
        bufs.append(bc.fit(sb, lat, *cap))
    return case("full width", cap, bufs)


# ---------------------------------------------------------------- the oracle anchor
ANCHOR_CONSTS = dict(gravity=(0.0, 0.0), drag_coeff=0.0)


def anchor_scenes(sb):
    """name -> Buffers: gravity 0, drag 0, no user force, every velocity and acceleration 0, nothing near a wall.  One oracle
    substep at subticks 64 then leaves v = (push + beam) * 2^-6 and stress = tension / 20."""
    beams_only = scene(sb, (8, 8), [p[:2] for p in np.asarray(beam_kinds(sb).particles[[7, 0, 3, 6, 1, 4]])],
                       [(0, 1, 40.0, 40.0, 45.0, 50.0, 700.0), (2, 3, 35.0, 35.0, 31.0, 3.0, 50.0), (4, 5, 25.0, 25.0, 25.0, 500.0, 800.0),
                        (1, 2, 150.0, 150.0, 150.0, 1.0, 50.0)], consts=ANCHOR_CONSTS)
    rng = np.random.default_rng(21)
    pts = 400.0 + 60.0 * rng.random((24, 2))
    contacts_only = scene(sb, (32, 8), pts, data_index=rng.permutation(32)[:24], consts=ANCHOR_CONSTS)
    both, _, _ = cs.two_bodies(sb)
    both = both.copy()
    both.set_physics_constants(**dict(sb.layout.DEFAULT_CONSTANTS, **ANCHOR_CONSTS))
    both.beams["target_length"][both.beams["length"] > 0] = 17.0
    return {"beams only": beams_only, "contacts only": contacts_only, "both": both}


def case_anchor(sb, name):
    buf = anchor_scenes(sb)[name]
    return case("anchor: " + name, (buf.max_particles, buf.max_beams), [buf])
