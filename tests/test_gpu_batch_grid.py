"""The batch's contact cells (BatchEngine with COLLIDE_GRID) against one all-pairs OracleEngine per scene: every
comparison is batch_cases.assert_same on load_scene(i), bit for bit, no tolerance.  info("cell_substeps") and
info("cell_overflow_substeps") show that the cells, and their fallback, really ran.  Scenes: tests/batch_cases.py (every case with
collisions on, forced onto the cells) and tests/batch_grid_cases.py (chosen to break a grid; tests/test_batch_grid_cpu.py shows
that they bite)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
from batch_harness import apply_to_batch, make_batch, upload_each  # noqa: E402
import batch_grid_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

OFF, ALLPAIRS, GRID = 0, 1, 2
_reference = {}


def reference(oracle, case):
    """Per op of the case's program, per scene: what the oracle's load_buffers gives (None: never uploaded).  Computed once per
    case and shared by the tests; never changed."""
    if case["name"] not in _reference:
        refs = [None if b is None else gc.make_oracle(oracle, case, b) for b in case["bufs"]]
        out = []
        for op in case["program"]:
            bc.apply_to_oracles(refs, op)
            out.append([None if r is None else r.load_buffers(b.copy()) for r, b in zip(refs, case["bufs"])])
        _reference[case["name"]] = out
    return _reference[case["name"]]


def compare(be, case, exp_per_scene, what):
    for i, (buf, exp) in enumerate(zip(case["bufs"], exp_per_scene)):
        if exp is None:
            continue
        if case.get("finite", True):
            assert np.isfinite(exp.particles).all()
        bc.assert_same(be.load_scene(i, buf.copy()), exp, "%s %s: scene %d" % (case["name"], what, i))


def run(sb, oracle, case, mode=GRID, grid_min_particles=1):
    """The case's program on a batch, compared with the oracle after every op."""
    exp = reference(oracle, case)
    be = make_batch(sb, case, mode=mode, grid_min_particles=grid_min_particles)
    upload_each(be, case["bufs"])
    for k, op in enumerate(case["program"]):
        apply_to_batch(be, op)
        compare(be, case, exp[k], "after op %d" % k)
    return be


ON_CASES = ["default v1", "default v2", "heterogeneous", "yield / break / delete", "permuted mapping + coincident particles",
            "user input", "default scene, 4 frames + 5 substeps"]


@pytest.mark.parametrize("name", ON_CASES)
def test_every_batch_case_with_collisions_on_the_cells(sb, oracle, name):
    cases = {c["name"]: c for c in bc.all_cases(sb) if c["mode"]}
    assert sorted(cases) == sorted(ON_CASES)                    # none left out
    be = run(sb, oracle, cases[name])
    assert be.info("cell_substeps") > 0 and be.info("contact_cells_per_side") > 0
    assert be.info("grid_min_particles") == 1 and be.info("contact_cell_capacity") == gc.CELL_K
    assert be.info("frame_kernel_scratch_bytes") == 0
    with pytest.raises(sb.EngineError) as ei:
        be.info("cell_substep")
    assert "cell_substep" in str(ei.value)
    be.destroy()


def test_pile_overflows_and_falls_back(sb, oracle):
    be = run(sb, oracle, gc.case_pile(sb))
    assert be.info("cell_overflow_substeps") > 0 and be.info("cell_substeps") > 0
    assert be.info("cell_overflow_substeps") + be.info("cell_substeps") == 69
    be.destroy()


def test_lattice_at_rest_never_overflows(sb, oracle):
    be = run(sb, oracle, gc.case_rest(sb))
    assert be.info("cell_overflow_substeps") == 0 and be.info("cell_substeps") == 16
    be.destroy()


def test_rings_take_the_cells_and_the_crowded_one_the_fallback(sb, oracle):
    """A centre with 0, 1, 3, 4, 5, 7, 8 and 9 partners, spread over four cells; the ninth scene's ring in one cell."""
    case = gc.case_rings(sb)
    be = run(sb, oracle, case)
    assert be.info("max_particles") == 64 and be.info("grid_min_particles") == 1 and be.info("contact_cells_per_side") == 12
    assert be.info("cell_substeps") > 0 and be.info("cell_overflow_substeps") > 0
    assert be.info("cell_substeps") + be.info("cell_overflow_substeps") == len(case["bufs"]) * gc.substeps_of(case["program"])
    be.destroy()


def test_cell_edges(sb, oracle):
    be = run(sb, oracle, gc.case_edges(sb))
    assert be.info("contact_cells_per_side") == 49 and be.info("cell_substeps") > 0
    be.destroy()


def test_out_of_range_coordinates(sb, oracle):
    case = gc.case_out_of_range(sb)
    be = run(sb, oracle, case)
    exp = reference(oracle, case)[-1][0]
    assert not np.isfinite(exp.particles[:17]).all() and np.isfinite(exp.particles[:12]).all()
    assert be.info("cell_substeps") > 0 and be.info("cell_substeps") + be.info("cell_overflow_substeps") == 3
    be.destroy()


@pytest.mark.parametrize("bounds,radius", gc.GEOMETRIES)
def test_geometries(sb, oracle, bounds, radius):
    case = gc.case_geometry(sb, bounds, radius)
    be = run(sb, oracle, case)
    g = be.info("contact_cells_per_side")
    assert g == gc.cell_geometry(bounds, radius, gc.GEOMETRY_CAP[0])[0]
    if radius == 600.0:
        assert g == 1
    if radius == 0.5:
        assert g == gc.cell_cap(gc.GEOMETRY_CAP[0]) == 25
    assert be.info("cell_substeps") + be.info("cell_overflow_substeps") == gc.substeps_of(case["program"])
    be.destroy()


def test_threshold_picks_the_scenes(sb, oracle):
    case = gc.case_mixed(sb)
    n_sub = gc.substeps_of(case["program"])
    be = run(sb, oracle, case, grid_min_particles=128)
    assert be.info("grid_min_particles") == 128
    assert be.info("cell_substeps") == 2 * n_sub and be.info("cell_overflow_substeps") == 0      # the scenes of 144 and 1024
    be.destroy()
    never = run(sb, oracle, case, grid_min_particles=gc.NEVER)
    assert never.info("cell_substeps") == 0 and never.info("cell_overflow_substeps") == 0
    assert never.info("contact_cells_per_side") == 0
    never.destroy()


@pytest.mark.parametrize("which", ["pile", "break"])
def test_grid_and_allpairs_batches_agree(sb, oracle, which):
    import torch
    src = gc.case_pile(sb) if which == "pile" else bc.case_break(sb)
    case = dict(src, name=src["name"] + " / frame 2, step 7, delete", program=[("frame", 2), ("step", 7), ("delete",)])
    out = []
    for mode in (GRID, ALLPAIRS):
        be = run(sb, oracle, case, mode=mode)
        p, b, a = be.state_tensors()
        out.append((p, b, a, be.render(64).clone(), be.info("cell_substeps")))
        be.sync()
        be.destroy()
    (p0, b0, a0, r0, n0), (p1, b1, a1, r1, n1) = out
    assert n0 > 0 and n1 == 0
    for x, y in ((p0, p1), (b0, b1)):
        assert torch.equal(x.isnan(), y.isnan()) and torch.equal(x.nan_to_num(nan=0.0).view(torch.int32), y.nan_to_num(nan=0.0).view(torch.int32))
    assert torch.equal(a0, a1) and torch.equal(r0, r1) and int(r0.max()) > 0


def test_cells_follow_positions_changed_outside_the_kernel(sb, oracle):
    """A masked reset in the middle of a program and write_particles_device between frames: the next launch bins what is there."""
    import torch
    case = bc.case_break(sb)
    bufs = case["bufs"]
    be = make_batch(sb, case, mode=GRID, grid_min_particles=1)
    upload_each(be, bufs)
    refs = [bc.make_oracle(oracle, case, b) for b in bufs]

    def check(what):
        for i, (buf, ref) in enumerate(zip(bufs, refs)):
            bc.assert_same(be.load_scene(i, buf.copy()), ref.load_buffers(buf.copy()), "%s: scene %d" % (what, i))

    be.frame(1)
    bc.apply_to_oracles(refs, ("frame", 1))
    check("frame")
    mask = [1, 0, 1, 0, 0, 1]
    be.reset(torch.tensor(mask, dtype=torch.uint8, device="cuda"))
    for i, m in enumerate(mask):
        if m:
            refs[i] = bc.make_oracle(oracle, case, bufs[i])
    be.step(9)
    bc.apply_to_oracles(refs, ("step", 9))
    check("masked reset + 9 substeps")
    p, _, _ = be.state_tensors()
    q = p.clone()
    q[..., 0] = 400.0 - p[..., 0]                               # mirrored about x = 200: the lattices land in other cells
    q[..., 2] = -p[..., 2]
    be.write_particles_device(q)
    for ref, buf in zip(refs, bufs):
        cur = ref.particles_b if ref.final_in_b else ref.particles_a
        rows = buf.mapping[:buf.particle_count].astype(np.int64)
        cur[rows, 0] = np.float32(400.0) - cur[rows, 0]
        cur[rows, 2] = -cur[rows, 2]
    check("import")
    be.frame(1)
    bc.apply_to_oracles(refs, ("frame", 1))
    check("frame after the import")
    assert be.info("cell_substeps") + be.info("cell_overflow_substeps") == 6 * (64 + 9 + 64) and be.info("cell_substeps") > 0
    be.destroy()
