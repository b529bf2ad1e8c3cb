"""Parity at the edges of the exact-arithmetic gates, gate by gate AS COMPILED INTO EACH KERNEL: every case of tests/gate_cases.py
(one launch holding lanes on both sides of a gate; whole launches beyond either edge) on every schedule that contains the gate,
against OracleEngine, bit for bit (test_gpu_parity.assert_same: particles, beams, mapping, metadata).  tests/test_gate_cases_cpu.py
shows on the oracle alone that every case is finite and really lies across the gate it names."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
import gate_cases as gc  # noqa: E402
from test_gpu_parity import ALLPAIRS, ATOMIC, GRID, OFF, TILED, assert_same  # noqa: E402

pytestmark = pytest.mark.gpu

_cases, _reference = {}, {}


def the_case(sb, name):
    if not _cases:
        _cases.update((c["name"], c) for c in gc.all_cases(sb))
    return _cases[name]


def reference(oracle, c, mode, buf=None, key=None):
    """{substeps: the oracle's state} at the case's checkpoints; computed once per (case, collision scan), shared, never changed."""
    key = (key or c["name"], gc.ref_mode(mode))
    if key not in _reference:
        _reference[key] = gc.oracle_states(oracle, c, mode, buf)
    return _reference[key]


def run_engine(sb, oracle, c, mode, what, **options):
    """The case on one Engine, compared after every checkpoint; returns what info() said."""
    buf = c["buf"]
    exp = reference(oracle, c, mode)
    eng = sb.Engine(bounds_size=c["bounds"], particle_radius=c["radius"], subticks=64, layout=2, max_particles=buf.max_particles,
                    max_beams=buf.max_beams, collision_mode=mode, **options)
    eng.write_buffers(buf)
    info = {k: eng.info(k) for k in ("path", "tiles", "substeps_per_launch", "material_mode")}
    done = 0
    for n in c["checkpoints"]:
        eng.step(n - done)
        done = n
        assert np.isfinite(exp[n].particles).all()
        assert_same(eng.load_buffers(buf.copy()), exp[n], "%s, %s, mode %d, %d substeps" % (c["name"], what, mode, n))
    eng.destroy()
    return info


NAMES = gc.NAMES
NOT_BLOCKED = ["M4 two particles 1e-15 apart"]                    # (collisions on: no blocked plan)
MIXED = [n for n in NAMES if not n.startswith("scaled")]


def test_the_names_are_the_cases(sb):
    assert sorted(NAMES) == sorted(c["name"] for c in gc.all_cases(sb))
    assert sorted(NOT_BLOCKED) == sorted(c["name"] for c in gc.all_cases(sb) if c["blocked"] is None)
    assert sorted(MIXED) == sorted(c["name"] for c in gc.all_cases(sb) if c["batch"])


@pytest.mark.parametrize("name", NAMES)
def test_atomic(sb, oracle, name):
    """k_beams (sb_beam_eval) and the particle kernel with the all-pairs scan."""
    c = the_case(sb, name)
    for mode in c["modes"]:
        if mode != GRID:
            info = run_engine(sb, oracle, c, mode, "atomic", path=ATOMIC)
            assert info["path"] == ATOMIC


@pytest.mark.parametrize("name", NAMES)
def test_tiled(sb, oracle, name):
    """k_substep_tiled, one substep per launch, several tiles of 64 and of 256; with the hash and its neighbour lists where the case
    has contacts."""
    c = the_case(sb, name)
    for mode in c["modes"]:
        if mode != ALLPAIRS:
            for tile in (64, 256):
                info = run_engine(sb, oracle, c, mode, "tiled %d" % tile, path=TILED, tile_particles=tile, block_substeps=1)
                assert info["path"] == TILED and info["substeps_per_launch"] == 1
                assert info["tiles"] >= (2 if tile == 64 or c["buf"].particle_count > 256 else 1)


@pytest.mark.parametrize("name", [n for n in NAMES if n not in NOT_BLOCKED])
@pytest.mark.parametrize("K", [3, 5])
def test_blocked(sb, oracle, name, K):
    """sb_beam_group and the blocked kernel's own 1/length gates, K substeps per launch (23 = 4 * 5 + 3: a launch of K, a remainder).
    A scene the host routes away from the blocked kernel (a spring below 2^-50) runs one substep per launch and is compared all the same."""
    c = the_case(sb, name)
    info = run_engine(sb, oracle, c, OFF, "blocked K=%d" % K, path=TILED, tile_particles=64, block_substeps=K)
    assert info["substeps_per_launch"] == (K if c["blocked"] else 1), info
    if "material_mode" in c and c["blocked"]:   # (the blocked plan's dictionary holds 256 rows; the tiled kernel's 2048 take every length here)
        assert info["material_mode"] == c["material_mode"]


@pytest.mark.parametrize("name", MIXED)
def test_batch_offender_beside_plain_lattices(sb, oracle, name):
    """Four scenes, one workgroup each: the offender in slot 2, the plain lattice in the others; contacts by the walk and by the cell
    grid.  Every scene against its own oracle: the plain ones must come out as the plain lattice alone does."""
    c = the_case(sb, name)
    off = c["buf"]
    cap = (off.max_particles, off.max_beams)
    plain = bc.fit(sb, gc.base_lattice(sb), *cap)
    bufs = [plain, plain, off, plain]
    exp_plain = reference(oracle, c, ALLPAIRS, buf=plain, key="plain lattice %s %s" % (cap, c["checkpoints"]))
    exp_off = reference(oracle, c, ALLPAIRS)
    for mode in (ALLPAIRS, GRID):
        be = sb.BatchEngine(n_scenes=4, bounds_size=c["bounds"], particle_radius=c["radius"], layout=2, max_particles=cap[0],
                            max_beams=cap[1], collision_mode=mode, subticks=64, grid_min_particles=1)
        for i, b in enumerate(bufs):
            be.write_scene(b, i, 1)
        done = 0
        for n in c["checkpoints"]:
            be.step(n - done)
            done = n
            for i, b in enumerate(bufs):
                exp = (exp_off if i == 2 else exp_plain)[n]
                assert np.isfinite(exp.particles).all()
                bc.assert_same(be.load_scene(i, b.copy()), exp, "%s, batch mode %d, scene %d, %d substeps" % (name, mode, i, n))
        if mode == GRID:
            assert be.info("cell_substeps") + be.info("cell_overflow_substeps") == 4 * done
        be.destroy()
