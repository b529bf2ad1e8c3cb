"""The scene and the uploads of tests/test_gpu_upload_state.py: what an engine that has RUN holds behind a second upload must be
what a fresh engine holds behind that upload alone (DESIGN.md 4.2 "just uploaded"; csrc/sb_api.hip reset_run_state).

Scene S: the 48 x 40 lattice of tests/promise_cases.py (1920 particles, at least 8 tiles of 256) with strain limit 0.26, and
  - one beam uploaded with target != rest length (its tile starts as yielded),
  - one particle of another tile uploaded with a nonzero acceleration (its tile starts dirty),
  - one particle of the left edge thrown outwards at 300 per second: its beams break within a few substeps, collisions or not,
  - one interior particle shifted by 5.5 of 25: its two beams along the shift yield in substep 1, and it starts 19.5 < 2 r from
    its neighbour, so with collisions on there is a contact from substep 1 on.
An engine takes S, runs FIRST_RUN substeps and a delete pass, and then gets one of UPLOADS:
  same      S again (the plan is kept)
  other     S without every fourth beam: more than an eighth gone, another topology (the upload plans again)
  cut       S without five beams, the records that are left renumbered in order (the plan is kept and edited)
and steps CALLS.  tests/test_upload_state_cpu.py shows on the oracle that all of it bites within those steps."""
import numpy as np

import promise_cases as pc

F = np.float32
FIRST_RUN = 37
CALLS = (1, 2, 37)
UPLOADS = ("same", "other", "cut")
S_PLASTIC = (pc.pid(40, 30), pc.pid(41, 30))  # the beam uploaded 1 % longer than its rest length
S_ACC, S_ACC_VALUE = pc.pid(40, 8), (0.25, -0.75)
S_THROWN, S_THROWN_V = pc.pid(0, 10), (-300.0, 0.0)
S_SHIFTED = pc.P1_PARTICLE
CUT = ((10, 10), (11, 10)), ((10, 10), (10, 11)), ((30, 20), (31, 20)), ((44, 35), (44, 36)), ((2, 38), (3, 38))


def scene(sb):
    buf = pc.lattice(sb, origin=pc.P_ORIGIN, strain_limit=pc.P3_LIMIT, consts=pc.QUIET, slack=8)
    pc.shift(buf, S_THROWN, v=S_THROWN_V)
    pc.shift(buf, S_SHIFTED, dx=pc.P3_SHIFT)
    j = pc.beam_between(buf, *S_PLASTIC)
    buf.beams["target_length"][j] = buf.beams["length"][j] * F(1.01)
    buf.particles[S_ACC, 4:6] = S_ACC_VALUE
    return buf


def without(buf, keep):
    """`buf` with only the beams keep[] of its slots, renumbered in order (what an editor leaves of a scene after removeBeam calls)."""
    out = buf.copy()
    B, maxP = buf.beam_count, buf.max_particles
    recs = buf.beams[buf.mapping[maxP:maxP + B].astype(np.int64)][keep]
    n = len(recs)
    out.beams[:n] = recs
    out.mapping[maxP:maxP + n] = np.arange(n)
    out.beam_count = n
    return out


def upload(sb, kind):
    s = scene(sb)
    B = s.beam_count
    keep = np.ones(B, bool)
    if kind == "other":
        keep[::4] = False
        keep[pc.beams_at(s, S_THROWN)] = True               # (what makes S bite stays)
        keep[pc.beams_at(s, S_SHIFTED)] = True
        keep[pc.beam_between(s, *S_PLASTIC)] = True
    elif kind == "cut":
        for p, q in CUT:
            keep[pc.beam_between(s, pc.pid(*p), pc.pid(*q))] = False
    return s if kind == "same" else without(s, keep)


def oracle_states(orc, buf, mode, calls):
    """The oracle's state behind each of `calls` (a substep count; "pass": a delete pass) on a fresh engine that uploaded `buf`."""
    ref = orc.OracleEngine(pc.BOUNDS, pc.RADIUS, 64, 2, pc.ALLPAIRS if mode == pc.GRID else mode, threads=8)
    ref.write_buffers(buf)
    out = []
    for call in calls:
        if call == "pass":
            ref.delete_pass()
        else:
            ref.step(call)
        out.append(ref.load_buffers(buf.copy()))
    return out
