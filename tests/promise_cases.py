"""Hand-made scenes that walk the two per-tile promise flags of the single-scene engine through every transition (DESIGN.md 4.1:
"zero accelerations", d_acc_flag[buffer][tile]; "never yielded", d_plastic[buffer][tile] of the blocked plan).

Base scene: a 48 x 40 lattice, d = 25, no jitter, layout 2, bounds 2000, radius 10: 1920 particles (data index x * 40 + y), at
least 8 tiles of 256.  No random numbers.  A case is a dict:
  name, kind    "acc" / "plastic"
  buf           layout.Buffers with the physics constants in its metadata
  schedules     {label: calls}; a call is a substep count for step(n) (0: compare without stepping) or "frame" (64 substeps and
                a delete pass)
  ...           what the case promises (tests/test_promise_cases_cpu.py asserts it on the oracle alone)
An acceleration is nonzero only where a particle is clamped onto a wall while it moves along it in the negative direction
(compute.wgsl:191-198: a -= min(a, sign(v) * friction * ...)), so the acceleration scenes drift towards -x.

tests/test_promise_cases_cpu.py shows on the oracle that every case bites; tests/test_gpu_promise_flags.py runs them on every
kernel that reads or writes the flags, comparing bit for bit after EVERY call and asking the engine for its flag counts."""
import numpy as np

F = np.float32
OFF, ALLPAIRS, GRID = 0, 1, 2
W, H, D = 48, 40, 25.0
BOUNDS, RADIUS = 2000.0, 10.0
KS = (2, 3, 5)                                # depths of the blocked launches the GPU tests run
# every call length 1, 2, K - 1, K, K + 1 for K in KS, and 37 (odd, longer than any launch: a call of several launches and a
# remainder); A starts with a long call, B with single substeps, so every transition lands on both buffer parities and both
# inside a deep launch and at the edge of a call.  Calls end INSIDE A1's contact windows (substeps 2, 57-58, 111-112, 166-167) and
# in the clean stretches between them -- A after 58, 112 and 167 substeps, B after 2, 58, 111, 112 and 166 -- which
# tests/test_promise_cases_cpu.py asserts from the oracle's trace, so the flag assertions at those checkpoints cannot go vacuous.
SCHEDULE_A = (37, 1, 2, 3, 4, 5, 6, 37, 5, 4, 3, 5, 2, 1, 37, 6, 4, 5, 3, 37)
SCHEDULE_B = (1, 1, 2, 37, 6, 5, 4, 2, 3, 37, 6, 5, 2, 1, 2, 37, 4, 5, 6, 3, 37)
SCHEDULES = {"A": SCHEDULE_A, "B": SCHEDULE_B}
assert sum(SCHEDULE_A) == 207 and sum(SCHEDULE_B) == 206
QUIET = dict(gravity=(0.0, 0.0), border_elasticity=0.5, border_friction=0.2, elasticity=0.5, friction=0.1, drag_coeff=0.0, drag_exp=2.0)
NAMES = ["A1 bounce", "A2 one corner", "A3 -0.0", "A4 import", "P1 one interior particle", "P1 late", "P2 cut in x", "P2 cut in y",
         "P3 break and delete", "P3 break and delete, survivor", "P4 upload holds yielded beams"]


def pid(x, y):
    return x * H + y


def substeps(call):
    return 64 if call == "frame" else int(call)


def lattice(sb, *, origin, spring=50.0, damp=700.0, yield_strain=0.2, strain_limit=1.0e9, velocity=None, consts=None, slack=0):
    buf = sb.scenes.lattice_buffers(W, H, d=D, origin=origin, spring=spring, damp=damp, yield_strain=yield_strain,
                                    strain_limit=strain_limit, layout=2, velocity=velocity, slack=slack)
    if consts:
        buf.set_physics_constants(**consts)
    return buf


def beams_at(buf, p):
    """Indices of the beams with an endpoint at particle p."""
    B = buf.beam_count
    return np.nonzero((buf.beams["a"][:B] == p) | (buf.beams["b"][:B] == p))[0]


def beam_between(buf, p, q):
    B = buf.beam_count
    a, b = buf.beams["a"][:B], buf.beams["b"][:B]
    (j,) = np.nonzero(((a == p) & (b == q)) | ((a == q) & (b == p)))[0]
    return int(j)


def case(name, kind, buf, schedules=None, **more):
    return dict(name=name, kind=kind, buf=buf, schedules=dict(schedules or SCHEDULES), **more)


# ---------------------------------------------------------------- accelerations
A1_CONSTS = dict(gravity=(0.0, -0.5), border_elasticity=0.9, border_friction=0.2, elasticity=0.5, friction=0.1, drag_coeff=0.001, drag_exp=2.0)


def case_a1(sb):
    """Soft beams (spring 0.2, damp 2), thrown at the floor from half a unit above it at (-8, -30): the bottom rows touch, rebound
    (border elasticity 0.9), are pulled back by gravity and the rows above, and touch again every 55 substeps or so.  Yield strain
    1e9: nothing yields, the case moves the acceleration flag alone."""
    buf = lattice(sb, origin=(100.0, 10.5), spring=0.2, damp=2.0, yield_strain=1.0e9, velocity=(-8.0, -30.0), consts=A1_CONSTS)
    return case("A1 bounce", "acc", buf)


A2_SHEAR = 6.0                                # rise per column: column x starts 6 x above column 0
A2_CORNER = (6, 4)                            # columns and rows of the block that may touch


def case_a2(sb, name="A2 one corner"):
    """Stiff beams, thrown at (-8, -8) from two units above the floor, every column 6 units above the one to its left, border
    elasticity 0 (what touches stays down and keeps sliding towards -x): within 207 substeps only the bottom left corner touches."""
    buf = lattice(sb, origin=(100.0, 12.0), spring=50.0, damp=700.0, yield_strain=0.3, velocity=(-8.0, -8.0),
                  consts=dict(A1_CONSTS, border_elasticity=0.0))
    x = np.arange(W * H) // H
    buf.particles[:W * H, 1] += (x * A2_SHEAR).astype("f4")
    sb.scenes.rest_at_current_length(buf)     # (the sheared lattice is at rest)
    corner = np.array([pid(cx, cy) for cx in range(A2_CORNER[0]) for cy in range(A2_CORNER[1])])
    return case(name, "acc", buf, corner=corner)


A3_NEG0, A3_PLAIN = pid(6, 30), pid(40, 8)


def case_a3(sb):
    """At rest in mid-air under gravity; the upload carries acceleration bits 0x80000000 in x of one particle and (0.25, -0.75) on one
    particle of another tile.  Read back after 0, 1 and 2 substeps: both buffers are written once."""
    buf = lattice(sb, origin=(100.0, 300.0), consts=A1_CONSTS)
    buf.particles[A3_NEG0, 4] = F(-0.0)
    buf.particles[A3_PLAIN, 4:6] = (0.25, -0.75)
    return case("A3 -0.0", "acc", buf, schedules={"0-1-2": (0, 1, 1)})


A4_PARTICLE, A4_ACC, A4_AFTER_CALL = pid(40, 30), (0.5, -0.25), 1


def case_a4(sb):
    """A2's scene on schedule B; behind its call 1 (2 substeps: the corner touches in substep 16, every tile is clean) particle
    (40, 30), far from the corner, gets the acceleration (0.5, -0.25) through the device import."""
    c = case_a2(sb, "A4 import")
    c["schedules"] = {"B": SCHEDULE_B}
    c.update(import_particle=A4_PARTICLE, import_acc=A4_ACC, import_after_call=A4_AFTER_CALL)
    return c


# ---------------------------------------------------------------- plastic yield
P_ORIGIN = (400.0, 400.0)
P1_PARTICLE = pid(6, 10)                      # the middle of the bottom left 12 x 20 block, six columns from any bisection cut
P_SHIFT = 7.0                                 # of 25: the two beams along the shift are strained by 0.28 > yield 0.2, the others < 0.15


def shift(buf, p, dx=0.0, dy=0.0, v=(0.0, 0.0)):
    buf.particles[p, 0] += F(dx)
    buf.particles[p, 1] += F(dy)
    buf.particles[p, 2:4] = v


def case_p1(sb):
    buf = lattice(sb, origin=P_ORIGIN, consts=QUIET)
    shift(buf, P1_PARTICLE, dx=P_SHIFT)
    want = [beam_between(buf, pid(5, 10), pid(6, 10)), beam_between(buf, pid(6, 10), pid(7, 10))]
    return case("P1 one interior particle", "plastic", buf, yields=sorted(want), yield_within=(1, 1))


P1_LATE_SPRING, P1_LATE_DAMP, P1_LATE_V = 5.0, 5.0, (30.0, 0.0)


def case_p1_late(sb):
    """Soft beams (spring 5, damp 5), the particle in place but moving at 30 per second: the two beams along its way cross the yield
    strain in substep 14 -- in the third launch or later of schedule A's first call, and in schedule B's fourth call, behind its three
    single-launch calls."""
    buf = lattice(sb, origin=P_ORIGIN, spring=P1_LATE_SPRING, damp=P1_LATE_DAMP, consts=QUIET)
    shift(buf, P1_PARTICLE, v=P1_LATE_V)
    want = [beam_between(buf, pid(5, 10), pid(6, 10)), beam_between(buf, pid(6, 10), pid(7, 10))]
    return case("P1 late", "plastic", buf, yields=sorted(want), yield_within=(8, 30))


def case_p2(sb, axis):
    """The beam across the middle of the lattice (the first bisection cut of any tiling of it) and the one behind it."""
    buf = lattice(sb, origin=P_ORIGIN, consts=QUIET)
    if axis == "x":
        p, q, o = pid(W // 2 - 1, 10), pid(W // 2, 10), pid(W // 2 - 2, 10)
        shift(buf, p, dx=-P_SHIFT)
    else:
        p, q, o = pid(6, H // 2 - 1), pid(6, H // 2), pid(6, H // 2 - 2)
        shift(buf, p, dy=-P_SHIFT)
    want = [beam_between(buf, p, q), beam_between(buf, o, p)]
    return case("P2 cut in %s" % axis, "plastic", buf, yields=sorted(want), yield_within=(1, 1), cut_beam=beam_between(buf, p, q))


P3_LIMIT, P3_SHIFT, P3_V = 0.26, 5.5, (300.0, 0.0)
P3_SURVIVOR = pid(8, 14)                      # same block as P1's particle, no beam in common with it
P3_CALLS = ("frame", 1, 2, "frame", 5, "frame")


def case_p3(sb, survivor):
    """P1's particle shifted by 5.5 (strain 0.22: its two beams yield in substep 1) and thrown on at 300 per second, strain limit
    0.26: the two break within the first frame and that frame's pass removes them; nothing else ever yields.  Survivor variant:
    particle (8, 14) of the same tile shifted by 5.5 and left alone -- its two beams yield, never break, and keep their targets
    through the pass."""
    buf = lattice(sb, origin=P_ORIGIN, strain_limit=P3_LIMIT, consts=QUIET, slack=8)
    shift(buf, P1_PARTICLE, dx=P3_SHIFT, v=P3_V)
    keep = []
    if survivor:
        shift(buf, P3_SURVIVOR, dx=P3_SHIFT)
        keep = sorted([beam_between(buf, pid(7, 14), pid(8, 14)), beam_between(buf, pid(8, 14), pid(9, 14))])
    return case("P3 break and delete" + (", survivor" if survivor else ""), "plastic", buf, schedules={"frames": P3_CALLS},
                offender=sorted([beam_between(buf, pid(5, 10), pid(6, 10)), beam_between(buf, pid(6, 10), pid(7, 10))]), survivors=keep,
                pass_of_call=0)


P4_AFTER = 37                                 # substeps of P1 before its state is read back and uploaded again


def case_p4(sb):
    """P1 (the scene; the GPU test takes its state after 37 substeps -- schedule A's first call -- and uploads that into a fresh
    engine and into the same one, then runs schedule B on)."""
    c = case_p1(sb)
    c.update(name="P4 upload holds yielded beams", schedules={"B": SCHEDULE_B}, after=P4_AFTER)
    return c


def all_cases(sb):
    return [case_a1(sb), case_a2(sb), case_a3(sb), case_a4(sb), case_p1(sb), case_p1_late(sb), case_p2(sb, "x"), case_p2(sb, "y"),
            case_p3(sb, False), case_p3(sb, True), case_p4(sb)]


# ---------------------------------------------------------------- the oracle's side
def acc_set(st):
    """Data indices of the particles whose acceleration bits are not all zero (-0.0 counts)."""
    P = st.particle_count
    rows = st.mapping[:P].astype(np.int64)
    return rows[st.particles[rows, 4:6].view("<u4").any(axis=1)]


def yielded(st):
    """Data indices of the live beams whose target is not their rest length, bit for bit."""
    B, maxP = st.beam_count, st.max_particles
    rows = st.mapping[maxP:maxP + B].astype(np.int64)
    rec = st.beams[rows]
    return rows[rec["target_length"].view("<u4") != rec["length"].view("<u4")]


def live_beams(st):
    B, maxP = st.beam_count, st.max_particles
    return set(int(j) for j in st.mapping[maxP:maxP + B])


def oracle_run(orc, c, calls, mode=OFF, buf=None, every=True, edit=None):
    """The oracle over `calls`.  Returns (states, trace): states[i] = its state behind call i; trace = one row per substep
    (substep number, particles with a nonzero acceleration, yielded beams, live beams) when every=True, stepping one by one.
    edit(i, state) -> Buffers or None: a state to upload behind call i (the host's side of an import)."""
    buf = c["buf"] if buf is None else buf
    ref = orc.OracleEngine(BOUNDS, RADIUS, 64, 2, ALLPAIRS if mode == GRID else mode, threads=8)
    ref.write_buffers(buf)
    states, trace, done = [], [], 0
    for i, call in enumerate(calls):
        n = substeps(call)
        if every:
            for _ in range(n):
                ref.step(1)
                done += 1
                st = ref.load_buffers(buf.copy())
                trace.append((done, acc_set(st), yielded(st), st.beam_count))
        elif n:
            ref.step(n)
        if call == "frame":
            ref.delete_pass()
        st = ref.load_buffers(buf.copy())
        if edit is not None:
            new = edit(i, st)
            if new is not None:
                ref.write_buffers(new)
                st = new
        states.append(st)
    return states, trace


def a4_edit(c):
    def edit(i, st):
        if i != c["import_after_call"]:
            return None
        new = st.copy()
        new.particles[c["import_particle"], 4:6] = c["import_acc"]
        return new
    return edit
