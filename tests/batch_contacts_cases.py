"""Scenes and programs of the contacts tests (sb_batch_contacts_device).  A case is tests/batch_cases.py's dict with
tests/batch_grid_cases.py's optional `bounds` / `radius` / `finite`, plus `max_pairs`: a pair list long enough for every pair the
case ever has (tests/test_batch_contacts_cpu.py asserts that against the reference).  Contacts are compared before the program and
after every op of it.  The scenes are those of the grid, batch and bodies tests, plus three built for this call: two bodies that
touch (same-body and cross-body pairs), particles on and one ulp either side of the four walls, and a batch of a never-uploaded, an
empty and a one-particle scene.  test_batch_contacts_cpu.py shows on the reference alone that the cases bite."""
import numpy as np

import batch_cases as bc
import batch_grid_cases as gc
import batch_bodies_cases as bo
import batch_bodies_ref as br
import batch_contacts_ref as cr

F = np.float32
TRUNCATIONS = (1, 7)             # and count - 1: the max_pairs of the truncation test on the pile


def up(v):
    return np.nextafter(F(v), F(np.inf))


def dn(v):
    return np.nextafter(F(v), F(-np.inf))


def _with(case, max_pairs, name=None, **kw):
    out = dict(case, max_pairs=max_pairs, **kw)
    if name:
        out["name"] = name
    return out


# ---------------------------------------------------------------- scenes built for this call
TWO_BODIES_CAP = (32, 64)
BODY_SPACING, BODY_GAP = 15.0, 18.0      # both below 2r = 20; the diagonals (21.2, 23.4) are above it


def two_bodies(sb):
    """(a) A 3 x 3 and a 2 x 3 lattice side by side, each held together by beams along its rows and columns: spacing 15 inside
    a lattice, 18 between the facing columns.  Data indices and slots are shuffled.  Returns (Buffers, D, body of each particle)."""
    maxP, maxB = TWO_BODIES_CAP
    pts, body, edges = [], [], []
    for which, (w, x0) in enumerate(((3, 300.0), (2, 300.0 + 2 * BODY_SPACING + BODY_GAP))):
        base = len(pts)
        for r in range(3):
            for c in range(w):
                pts.append((x0 + BODY_SPACING * c, 400.0 + BODY_SPACING * r))
                body.append(which)
                if c:
                    edges.append((base + r * w + c - 1, base + r * w + c))
                if r:
                    edges.append((base + (r - 1) * w + c, base + r * w + c))
    n, m = len(pts), len(edges)
    rng = np.random.default_rng(5)
    D, S = rng.permutation(maxP)[:n], rng.permutation(n)
    E, T = rng.permutation(maxB)[:m], rng.permutation(m)
    buf = sb.Buffers(2, maxP, maxB)
    buf.particles[D, :2] = np.array(pts, "f4")
    buf.mapping[S] = D
    e = np.asarray(edges, dtype=np.int64)
    rec = buf.beams[E]
    rec["a"], rec["b"] = D[e[:, 0]], D[e[:, 1]]
    for f, v in (("length", BODY_SPACING), ("target_length", BODY_SPACING), ("last_length", BODY_SPACING), ("spring", 50.0), ("damp", 700.0),
                 ("yield_strain", 0.2), ("strain_break_limit", 0.5)):
        rec[f] = v
    buf.beams[E] = rec
    buf.mapping[maxP + T] = E
    buf.particle_count, buf.beam_count = n, m
    return buf, D, np.array(body)


def case_two_bodies(sb):
    return dict(name="two bodies that touch", layout=2, cap=TWO_BODIES_CAP, mode=bc.ALLPAIRS, bufs=[two_bodies(sb)[0], bc.empty_scene(sb, 2, TWO_BODIES_CAP)],
                program=[("step", 2)], max_pairs=64)


WALL_CAP = (16, 0)


def wall_points():
    """(b) For each of the four walls a particle exactly on lo / hi, one ulp inside and one ulp outside; 40 apart along the wall:
    no particle contacts.  [(x, y, expected wall word)]."""
    lo, hi = F(10.0), F(1000.0) - F(10.0)
    pts = []
    for k, (v, bit_on) in enumerate(((dn(lo), True), (lo, True), (up(lo), False))):
        pts.append((v, 300.0 + 40.0 * k, cr.LEFT if bit_on else 0))
        pts.append((300.0 + 40.0 * k, v, cr.LOW if bit_on else 0))
    for k, (v, bit_on) in enumerate(((up(hi), True), (hi, True), (dn(hi), False))):
        pts.append((v, 600.0 + 40.0 * k, cr.RIGHT if bit_on else 0))
        pts.append((600.0 + 40.0 * k, v, cr.HIGH if bit_on else 0))
    return pts


def case_walls(sb):
    pts = np.zeros((12, 6), "f4")
    pts[:, :2] = np.array([(x, y) for x, y, _ in wall_points()], "f4")
    rng = np.random.default_rng(6)
    return dict(name="on the walls", layout=2, cap=WALL_CAP, mode=bc.ALLPAIRS, bufs=[gc.free_particles(sb, 2, WALL_CAP, pts, rng.permutation(WALL_CAP[0])[:12])],
                program=[("step", 1)], max_pairs=4)


SMALL_CAP = (8, 8)


def case_never_empty_one(sb):
    """(c) A scene never uploaded, an empty one, one particle (in the corner: two wall bits), two particles."""
    one = np.zeros((1, 6), "f4")
    one[0, :2] = (10.0, 990.0)
    bufs = [None, bc.empty_scene(sb, 2, SMALL_CAP), gc.free_particles(sb, 2, SMALL_CAP, one, [5]), bc.two_particles(sb, 2, SMALL_CAP, vx=1.0)]
    return dict(name="never uploaded, empty, one particle", layout=2, cap=SMALL_CAP, mode=bc.ALLPAIRS, bufs=bufs, program=[("step", 1)], max_pairs=4)


def case_two_in_1024(sb):
    """Two particles at capacity 1024 / 4096: the defined rows far beyond the particles."""
    cap = (1024, 4096)
    return dict(name="two particles at 1024 / 4096", layout=2, cap=cap, mode=bc.ALLPAIRS, bufs=[bc.two_particles(sb, 2, cap, x=500.0), None], program=[],
                max_pairs=4)


# ---------------------------------------------------------------- the cases of the other suites
def case_pile(sb):
    return _with(gc.case_pile(sb), 4096)


def case_edges(sb):
    return _with(gc.case_edges(sb), 64)


def case_out_of_range(sb):
    return _with(gc.case_out_of_range(sb), 64)


def case_geometry(sb, bounds, radius):
    return _with(gc.case_geometry(sb, bounds, radius), 144 * 143 // 2)      # (radius 600: every pair touches)


def case_mixed(sb):
    return _with(gc.case_mixed(sb), 4096)


def case_rings(sb):
    """batch_grid_cases' rings: a centre with 0, 1, 3, 4, 5, 7, 8 and 9 partners; at most 9 spokes and 9 pairs along a ring."""
    return _with(gc.case_rings(sb), 32)


def case_mapping(sb):
    """batch_cases' permuted default scene and its `coincident` scene (particles on one spot: dist == 0)."""
    return _with(bc.case_mapping(sb), 1024)


def case_hetero(sb):
    return _with(bc.case_hetero(sb), 4096, name="heterogeneous (batch_cases' program)")


def case_break(sb):
    return _with(bc.case_break(sb), 1024, name="yield / break / delete (batch_cases' program)")


def case_saturation(sb):
    """batch_bodies_cases' saturation case: its fourth scene holds a NaN coordinate and an infinite velocity, so it is not
    compared on the oracle (a generated NaN's sign differs between the oracle's CPU and the GPU), only on load_scene."""
    return _with(bo.case_saturation(sb), 16, finite=False)


def grid_cases(sb):
    return [case_pile(sb), case_edges(sb), case_out_of_range(sb), case_mixed(sb), case_rings(sb)] + [case_geometry(sb, b, r) for b, r in gc.GEOMETRIES]


def batch_cases(sb):
    return [case_mapping(sb), case_hetero(sb), case_break(sb)]


def bodies_cases(sb):
    """The stepped cases of the bodies tests (their mapping case is batch_cases', their pile the grid's: not run twice)."""
    return [_with(bo.case_hetero(sb), 4096), _with(bo.case_break(sb), 1024), _with(bo.case_default(sb), 1024),
            _with(bo.case_default_120_300(sb), 1024), case_saturation(sb)]


def own_cases(sb):
    return [case_two_bodies(sb), case_walls(sb), case_never_empty_one(sb)]


def all_cases(sb):
    cases = grid_cases(sb) + batch_cases(sb) + bodies_cases(sb) + own_cases(sb)
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


def case_named(sb, name):
    return {c["name"]: c for c in all_cases(sb)}[name]


# ---------------------------------------------------------------- the reference side
def geometry(case):
    return case.get("radius", 10.0), case.get("bounds", 1000.0)


def make_oracles(orc, case):
    radius, bounds = geometry(case)
    out = []
    for b in case["bufs"]:
        if b is None:
            out.append(None)
            continue
        ref = orc.OracleEngine(bounds, radius, case.get("subticks", 64), case["layout"], bc.ALLPAIRS if case["mode"] else bc.OFF, threads=4)
        ref.write_buffers(b)
        out.append(ref)
    return out


def contacts_with_bodies(bufs_now, case, max_pairs=None, other_body=False, labels=True):
    """(touch, pairs, counts, labels) of a batch whose scenes are `bufs_now`: the reference with the labels of the bodies
    reference (labels=False: without labels)."""
    maxP = case["cap"][0]
    radius, bounds = geometry(case)
    lab = br.bodies_of(bufs_now, maxP)[0] if labels else None
    m = case["max_pairs"] if max_pairs is None else max_pairs
    return cr.contacts_of(bufs_now, maxP, radius, bounds, lab, m, other_body) + (lab,)


def expected_contacts(orc, case):
    """{op index: (touch, pairs, counts, labels)} of the case on one oracle per scene; -1: before the program."""
    refs, out = make_oracles(orc, case), {}

    def now():
        return contacts_with_bodies([None if r is None else r.load_buffers(b.copy()) for r, b in zip(refs, case["bufs"])], case)

    out[-1] = now()
    for k, op in enumerate(case["program"]):
        bc.apply_to_oracles(refs, op)
        out[k] = now()
    return out
