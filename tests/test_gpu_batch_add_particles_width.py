"""BatchEngine.add_particles at full width and capacity, bit for bit against tests/batch_add_particles_ref.py and the
oracle: 64 rows in one call, the limit capacity filled to exactly 1024 with the free indices in the last bitmap words, the particle
count taken across the default grid_min_particles, capacities that are no multiple of the bitmap word, and SKIP_TOUCHING with the
upper half of the rows blocked by the lower.  tests/test_batch_add_particles_cpu.py asserts what each case is built for."""
import numpy as np
import pytest

import batch_add_particles_cases as cases
import batch_add_particles_ref as ref
from test_gpu_batch_add_particles import ALLPAIRS, GRID, OFF, batch, check_against_ref, oracle_frames
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu


def test_sixty_four_rows_fill_the_limit_capacity(sb, oracle):
    """960 -> exactly 1024 with 64 rows, the free indices in the last bitmap words; 1000 -> 1024 with 40 x FULL; then one frame"""
    case = cases.sixty_four_case(sb)
    be = batch(sb, case, GRID)
    after, res, cnt = check_against_ref(be, case, what="64 rows")
    assert cnt == [[64, 0, 0, 0], [24, 0, 0, 40]] and res[0, -1] == 1023 and be.summary().cpu().numpy()[:, 0].tolist() == [1024.0, 1024.0]
    assert check_against_ref(be, case, what="full")[2] == [[0, 0, 0, 64]] * 2
    be.frame()
    for i in range(2):
        assert_same(be.load_scene(i, after[i].copy()), oracle_frames(oracle, after[i], 1, ALLPAIRS), "scene %d: the frame after == oracle" % i)
    be.destroy()


def test_across_the_grid_threshold(sb, oracle):
    """P from 250 to 260 across the default grid_min_particles of 256: the next frame runs on the cells and matches the oracle"""
    case = cases.threshold_case(sb)
    be = batch(sb, case, GRID)
    assert be.info("grid_min_particles") == 256
    be.step(2)
    assert be.info("cell_substeps") == 0, "250 particles walk"
    after, res, cnt = check_against_ref(be, case, what="threshold")
    assert cnt == [[10, 0, 0, 0]] and after[0].particle_count == 260
    be.frame()
    assert be.info("cell_substeps") > 0, "260 particles run on the cells"
    assert_same(be.load_scene(0, after[0].copy()), oracle_frames(oracle, after[0], 1, ALLPAIRS), "the frame on the cells == oracle")
    be.destroy()


@pytest.mark.parametrize("cap", cases.ODD_CAPS, ids=lambda c: "%dx%d" % c)
def test_odd_capacities(sb, oracle, cap):
    case = cases.odd_case(sb, cap)
    be = batch(sb, case, OFF)
    after, res, cnt = check_against_ref(be, case, what="odd %s" % (cap,))
    assert cnt == [[0, 0, 0, 0], [cap[0] - 25, 0, 0, 2], [0, 0, 0, 0]]
    be.frame()
    for i in range(3):
        assert_same(be.load_scene(i, after[i].copy()), oracle_frames(oracle, after[i], 1, OFF), "scene %d: the frame after == oracle" % i)
    be.destroy()


def test_upper_half_blocked_by_the_lower(sb):
    case = cases.halves_case(sb)
    be = batch(sb, case, OFF)
    _, res, cnt = check_against_ref(be, case, what="halves")
    assert res[0].tolist() == list(range(16, 48)) + [ref.BLOCKED] * 32 and cnt == [[32, 0, 32, 0]]
    be.destroy()
