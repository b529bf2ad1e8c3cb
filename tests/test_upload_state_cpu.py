"""The conditions that keep tests/test_gpu_upload_state.py honest, on the ORACLE alone (no GPU): scene S of
tests/upload_state_cases.py breaks beams within the first run (so its delete pass removes some), holds a yielded beam and a nonzero
acceleration in the upload itself, yields more within the first substep, and -- with collisions on -- makes a contact within every
stretch the GPU test compares; the three second uploads are what they are named for.  Conditions, not measurements: a scene that
misses one is changed, not the assertion."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import promise_cases as pc  # noqa: E402
import upload_state_cases as uc  # noqa: E402


def test_the_uploads_are_what_they_are_named_for(sb):
    s = uc.scene(sb)
    B = s.beam_count
    assert s.particle_count == 1920 and len(pc.yielded(s)) == 1 and list(pc.acc_set(s)) == [uc.S_ACC]
    assert uc.upload(sb, "same").beams.tobytes() == s.beams.tobytes()
    other, cut = uc.upload(sb, "other"), uc.upload(sb, "cut")
    assert B - other.beam_count > B // 8, "more than an eighth of the beams gone: no edit, the upload plans again"
    assert B - cut.beam_count == len(uc.CUT) <= B // 8
    for b in (other, cut):                                  # the state that makes S bite survives both
        assert len(pc.yielded(b)) == 1 and list(pc.acc_set(b)) == [uc.S_ACC]
        for p in (uc.S_THROWN, uc.S_SHIFTED):
            assert len(pc.beams_at(b, p)) == len(pc.beams_at(s, p))


@pytest.mark.parametrize("mode", [pc.OFF, pc.ALLPAIRS])
def test_the_first_run_breaks_yields_and_touches(sb, oracle, mode):
    s = uc.scene(sb)
    one, run, swept = uc.oracle_states(oracle, s, mode, (1, uc.FIRST_RUN - 1, "pass"))
    assert len(pc.yielded(one)) >= 3, "the shifted particle's two beams yield in substep 1, on top of the uploaded one"
    assert len(pc.acc_set(one)) == 0 or mode != pc.OFF, "the uploaded acceleration is consumed by the first substep"
    assert run.beam_count == s.beam_count and swept.beam_count < s.beam_count, "beams break within the first run; its pass removes them"
    assert np.isfinite(swept.particles[:swept.particle_count]).all()
    print("mode %d: %d beams yielded after 1 substep, %d removed by the pass" % (mode, len(pc.yielded(one)), s.beam_count - swept.beam_count))


@pytest.mark.parametrize("kind", uc.UPLOADS)
def test_every_compared_stretch_bites(sb, oracle, kind):
    """Behind the second upload: beams yield in the first call, and each call's state differs between collisions on and off (somebody
    touched by then) -- so the hash schedules are compared on contacts, not on a lattice that never meets itself."""
    buf = uc.upload(sb, kind)
    off = uc.oracle_states(oracle, buf, pc.OFF, uc.CALLS)
    on = uc.oracle_states(oracle, buf, pc.ALLPAIRS, uc.CALLS)
    for i, (a, b) in enumerate(zip(off, on)):
        assert np.isfinite(a.particles[:a.particle_count]).all() and np.isfinite(b.particles[:b.particle_count]).all()
        assert len(pc.yielded(a)) >= 3 and len(pc.yielded(b)) >= 3, (kind, i)
        assert a.particles.tobytes() != b.particles.tobytes(), "%s: no contact within call %d" % (kind, i)
