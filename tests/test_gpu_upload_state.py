"""An engine that has run, then gets a second upload, holds what a fresh engine holds behind that upload alone -- whether the upload
keeps the plan, plans again, or keeps and edits it (csrc/sb_api.hip: reset_run_state is the one writer of "just uploaded",
DESIGN.md 4.2).  tests/upload_state_cases.py has the scene and the uploads; five schedules x three uploads.

E1 uploads S, steps 37 substeps and runs a delete pass: acceleration and plastic flags written, break flags set, beams removed,
d_dead_gen and delete_gen counted up, and with the hash on a build (and, beside the tiling, the hybrid's look) behind it.  Then the
second upload.  BEFORE any step load_buffers of E1 equals, byte for byte, that of E2, a fresh engine that only got the second
upload; where E2 cannot plan differently ("same", "other") the flag counts agree as well.  Then calls of 1, 2 and 37 substeps,
each compared with the oracle bit for bit (test_gpu_parity.assert_same)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import promise_cases as pc  # noqa: E402
import upload_state_cases as uc  # noqa: E402
from test_gpu_parity import ALLPAIRS, ATOMIC, GRID, OFF, TILED, assert_same  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (Engine options, collision mode)
SCHEDULES = {
    "blocked K=3": (dict(path=TILED, tile_particles=256, block_substeps=3), OFF),
    "tiled": (dict(path=TILED, tile_particles=256, block_substeps=1), OFF),
    "tiled, hash, hybrid": (dict(tile_particles=256), GRID),
    "atomic, hash": (dict(path=ATOMIC), GRID),
    "atomic, all pairs": (dict(path=ATOMIC), ALLPAIRS),
}
_reference = {}


def reference(oracle, buf, kind, mode):
    """The oracle behind each of uc.CALLS on a fresh upload of `buf`; once per (upload, scan), shared, never changed."""
    key = (kind, ALLPAIRS if mode == GRID else mode)
    if key not in _reference:
        _reference[key] = uc.oracle_states(oracle, buf, mode, uc.CALLS)
    return _reference[key]


def engine(sb, buf, schedule):
    options, mode = SCHEDULES[schedule]
    eng = sb.Engine(bounds_size=pc.BOUNDS, particle_radius=pc.RADIUS, subticks=64, layout=2, max_particles=buf.max_particles,
                    max_beams=buf.max_beams, collision_mode=mode, **options)
    eng.write_buffers(buf)
    return eng


def same_bytes(a, b, what):
    for part in ("metadata", "mapping", "particles", "beams"):
        assert getattr(a, part).tobytes() == getattr(b, part).tobytes(), "%s: %s differs" % (what, part)


@pytest.mark.parametrize("kind", uc.UPLOADS)
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_second_upload_leaves_a_fresh_engines_state(sb, oracle, schedule, kind):
    options, mode = SCHEDULES[schedule]
    what = "%s, upload '%s'" % (schedule, kind)
    first, second = uc.scene(sb), uc.upload(sb, kind)
    e1 = engine(sb, first, schedule)
    if schedule == "blocked K=3":
        assert e1.info("substeps_per_launch") == 3
    if options.get("path") != ATOMIC:
        assert e1.info("path") == TILED and e1.info("tiles") >= 8, what
        assert e1.info("acc_dirty_tiles") >= 1, what + ": S uploads a nonzero acceleration"
    if schedule == "blocked K=3":
        assert e1.info("plastic_tiles") >= 1, what + ": S uploads a yielded beam"
    e1.step(uc.FIRST_RUN)
    e1.delete_pass()
    assert e1.counts()[1] < first.beam_count, what + ": the first run must break beams and its pass remove them"
    kept, edited = e1.info("uploads_kept"), e1.info("uploads_edited")
    e1.write_buffers(second)
    assert e1.info("uploads_kept") - kept == (0 if kind == "other" else 1), what
    assert e1.info("uploads_edited") - edited == (1 if kind == "cut" else 0), what
    e2 = engine(sb, second, schedule)
    same_bytes(e1.load_buffers(second.copy()), e2.load_buffers(second.copy()), what + ", before any step")
    if kind != "cut":                                       # (a cut scene: E2 may plan differently, only the state is compared)
        for key in ("acc_dirty_tiles", "plastic_tiles"):
            assert e1.info(key) == e2.info(key), "%s: %s" % (what, key)
    e2.destroy()
    states = reference(oracle, second, kind, mode)
    done = 0
    for call, exp in zip(uc.CALLS, states):
        e1.step(call)
        done += call
        assert_same(e1.load_buffers(second.copy()), exp, "%s: %d substeps behind the second upload" % (what, done))
    assert e1.info("substeps_done") == done, what
    e1.destroy()
