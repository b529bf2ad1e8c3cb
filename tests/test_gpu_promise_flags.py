"""Parity across every transition of the per-tile promise flags ("zero accelerations", "never yielded"): every case
of tests/promise_cases.py, on every schedule of step() calls it names, on every kernel that reads or writes the flags -- the blocked
kernel at K = 2, 3, 5, the tiled single-substep kernel with tiles of 64 and 256, the atomic path as the flag-free control and, for
the floor cases, the default collision mode (hash on, blocked plan beside the tiling).  Against OracleEngine bit for bit
(test_gpu_parity.assert_same: particles, beams, mapping, metadata) after EVERY call, and the engine is asked for its flag counts
(info "acc_dirty_tiles" / "plastic_tiles") wherever the oracle's own state says what they must be.
tests/test_promise_cases_cpu.py shows on the oracle alone that every case walks through the transitions it is named for."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import promise_cases as pc  # noqa: E402
from test_gpu_parity import ATOMIC, GRID, OFF, TILED, assert_same  # noqa: E402

pytestmark = pytest.mark.gpu

_cases, _reference = {}, {}
# name -> (Engine options, collision mode, flags: which of the two flag arrays the engine keeps)
CONFIGS = {
    "blocked K=2": (dict(path=TILED, tile_particles=256, block_substeps=2), OFF, ("acc", "plastic")),
    "blocked K=3": (dict(path=TILED, tile_particles=256, block_substeps=3), OFF, ("acc", "plastic")),
    "blocked K=5": (dict(path=TILED, tile_particles=256, block_substeps=5), OFF, ("acc", "plastic")),
    "tiled 64": (dict(path=TILED, tile_particles=64, block_substeps=1), OFF, ("acc",)),
    "tiled 256": (dict(path=TILED, tile_particles=256, block_substeps=1), OFF, ("acc",)),
    "atomic": (dict(path=ATOMIC), OFF, ()),
    "hash on": (dict(tile_particles=256), GRID, ("acc",)),
}
FLAT = [k for k in CONFIGS if k != "hash on"]
FLOOR = ["A1 bounce", "A2 one corner"]
ONE_LAUNCH_SLACK = ("the flag of the buffer a launch writes is recomputed by that launch from what it stores, so it may be 1 over "
                    "zeros only until the first launch behind an upload (which marks every tile of its buffer)")


def the_case(sb, name):
    if not _cases:
        _cases.update((c["name"], c) for c in pc.all_cases(sb))
    return _cases[name]


def reference(oracle, c, label, mode, buf=None, key=None):
    """(states behind every call, per-substep trace) of the oracle; computed once per (case, schedule, scan), shared, never changed."""
    key = (key or c["name"], label, pc.ALLPAIRS if mode == GRID else mode)
    if key not in _reference:
        edit = pc.a4_edit(c) if "import_particle" in c else None
        _reference[key] = pc.oracle_run(oracle, c, c["schedules"][label], mode=mode, buf=buf, edit=edit)
    return _reference[key]


def make_engine(sb, c, config, buf=None):
    options, mode, flags = CONFIGS[config]
    buf = c["buf"] if buf is None else buf
    eng = sb.Engine(bounds_size=pc.BOUNDS, particle_radius=pc.RADIUS, subticks=64, layout=2, max_particles=buf.max_particles,
                    max_beams=buf.max_beams, collision_mode=mode, **options)
    eng.write_buffers(buf)
    if config.startswith("blocked"):
        assert eng.info("substeps_per_launch") == options["block_substeps"], config
    elif config.startswith("tiled"):
        assert eng.info("path") == TILED and eng.info("substeps_per_launch") == 1
    elif config == "atomic":
        assert eng.info("path") == ATOMIC and eng.info("tiles") == 0
    if config != "atomic":
        assert eng.info("tiles") >= 8, config
    return eng


def check_flags(eng, c, config, trace, states, i, done, what):
    """The flag counts behind call i (`done` substeps in all), wherever the oracle's state says what they must be."""
    flags = CONFIGS[config][2]
    dirty, plastic, tiles = eng.info("acc_dirty_tiles"), eng.info("plastic_tiles"), eng.info("tiles")
    if "acc" not in flags:
        assert dirty == 0, what + ": an engine without tiles has no acceleration flags"
    if "plastic" not in flags:
        assert plastic == 0, what + ": an engine without a blocked plan has no plastic flags"
    if "acc" in flags and c["kind"] == "acc" and done:
        st = states[i]
        now = len(pc.acc_set(st)) > 0
        before = done >= 2 and len(trace[done - 2][1]) > 0 and "import_particle" not in c
        if now:
            assert dirty > 0, what + ": nonzero accelerations in a buffer whose tiles all promise zeros"
            assert dirty < tiles or c["name"] == "A1 bounce", what + ": one corner touches, %d of %d tiles are dirty" % (dirty, tiles)
        elif not before:
            assert dirty == 0, what + ": %d tiles dirty over accelerations that have been zero for two substeps (%s)" % (dirty, ONE_LAUNCH_SLACK)
    if "plastic" in flags and c["kind"] == "plastic":
        st = states[i]
        yielded = len(pc.yielded(st))
        if "offender" in c and i < c["pass_of_call"]:
            return
        if c.get("survivors"):                              # removed and surviving yielded beams in ONE tile: what the variant is named for
            assert plastic == 1, what + ": the survivor's beams and the offender's lie in one tile of 256, %d tiles are plastic" % plastic
        if yielded:
            assert 1 <= plastic <= 2, what + ": %d yielded beams around one particle, %d plastic tiles" % (yielded, plastic)
        else:
            assert plastic == 0, what + (": %d plastic tiles and no live beam has yielded (a delete pass recomputes the flag over the "
                                         "beams it leaves; no slack is allowed here)" % plastic)


def run_calls(sb, oracle, c, config, label, eng=None, buf=None, key=None):
    calls = c["schedules"][label]
    states, trace = reference(oracle, c, label, CONFIGS[config][1], buf=buf, key=key)
    own = eng is None
    if own:
        eng = make_engine(sb, c, config, buf)
    base = c["buf"] if buf is None else buf
    if CONFIGS[config][0].get("path") == TILED and "cut_beam" in c:
        assert eng.info("beam_copies") > base.beam_count, "no beam is cut"
    done = 0
    for i, call in enumerate(calls):
        what = "%s, schedule %s, %s, call %d (%s): %d substeps" % (c["name"], label, config, i, call, done + pc.substeps(call))
        if call == "frame":
            eng.frame()
        elif call:
            eng.step(call)
        done += pc.substeps(call)
        if i == c.get("import_after_call", -1):             # A4: the first nonzero acceleration of a clean tile, through the import
            if CONFIGS[config][2]:
                assert eng.info("acc_dirty_tiles") == 0, what + ": before the import"
            t = eng.state_tensors()
            t["particles"][c["import_particle"], 4:6] = torch.tensor(c["import_acc"], dtype=torch.float32, device=t["particles"].device)
            eng.write_particles_device(t["particles"])
            if CONFIGS[config][2]:
                assert eng.info("acc_dirty_tiles") == 1, what + ": behind the import"
        assert np.isfinite(states[i].particles).all()
        assert_same(eng.load_buffers(base.copy()), states[i], what)
        if c["name"] == "A3 -0.0" and i == 0:
            if CONFIGS[config][2]:
                assert eng.info("acc_dirty_tiles") >= 2, what + ": two tiles hold nonzero acceleration bits"
        else:
            check_flags(eng, c, config, trace, states, i, done, what)
    info = {k: eng.info(k) for k in ("hybrid_substeps", "substeps_done")}
    if own:
        eng.destroy()
    return info


def test_the_names_are_the_cases(sb):
    assert sorted(pc.NAMES) == sorted(c["name"] for c in pc.all_cases(sb))


@pytest.mark.parametrize("config", FLAT)
@pytest.mark.parametrize("name", [n for n in pc.NAMES if not n.startswith("P4")])
def test_case(sb, oracle, name, config):
    c = the_case(sb, name)
    for label in c["schedules"]:
        if c["kind"] == "plastic" and "plastic" in CONFIGS[config][2]:      # before anything yields: the upload holds rest lengths only
            eng = make_engine(sb, c, config)
            assert eng.info("plastic_tiles") == 0, "%s, %s: plastic tiles behind an upload in which no beam has yielded" % (name, config)
            run_calls(sb, oracle, c, config, label, eng=eng)
            eng.destroy()
        else:
            run_calls(sb, oracle, c, config, label)


@pytest.mark.parametrize("name", FLOOR)
def test_floor_case_with_the_hash_on(sb, oracle, name):
    """The default collision mode: the lattice never comes within 2r of itself, so runs of tracked blocked launches and single
    substeps of k_substep_tiled_grid alternate while the floor contact comes and goes; both keep the same acceleration flags."""
    c = the_case(sb, name)
    blocked = 0
    for label in c["schedules"]:
        info = run_calls(sb, oracle, c, "hash on", label)
        total = sum(c["schedules"][label])
        assert info["substeps_done"] == total
        assert info["hybrid_substeps"] < total, "%s, schedule %s: no single substeps ran (%s)" % (name, label, info)
        blocked += info["hybrid_substeps"]
    assert blocked > 0, "%s: no blocked launches ran on either schedule" % name


@pytest.mark.parametrize("config", FLAT)
def test_upload_holds_yielded_beams(sb, oracle, config):
    """P4: P1's state after 37 substeps, read back and uploaded into a fresh engine and into the same engine (which keeps its plan),
    then schedule B."""
    c = the_case(sb, "P4 upload holds yielded beams")
    p1 = the_case(sb, "P1 one interior particle")
    states, _ = reference(oracle, p1, "A", OFF)
    mid = states[0]                                          # (schedule A's first call is 37 substeps)
    assert pc.SCHEDULE_A[0] == c["after"] and len(pc.yielded(mid)) == 2
    eng = make_engine(sb, c, config)
    eng.step(c["after"])
    got = eng.load_buffers(c["buf"].copy())
    assert_same(got, mid, "P4, %s: before the upload" % config)
    has = "plastic" in CONFIGS[config][2]
    fresh = make_engine(sb, c, config, buf=got)
    if has:
        assert 1 <= fresh.info("plastic_tiles") <= 2, "P4, %s: a fresh engine's upload holds yielded beams" % config
    run_calls(sb, oracle, c, config, "B", eng=fresh, buf=mid, key="P4 from P1's state")
    fresh.destroy()
    kept = eng.info("uploads_kept")
    eng.write_buffers(got)
    if CONFIGS[config][0].get("path") == TILED:
        assert eng.info("uploads_kept") == kept + 1, "P4, %s: the same scene again must keep the plan" % config
    if has:
        assert 1 <= eng.info("plastic_tiles") <= 2, "P4, %s: the same engine's upload holds yielded beams" % config
    run_calls(sb, oracle, c, config, "B", eng=eng, buf=mid, key="P4 from P1's state")
    eng.destroy()
