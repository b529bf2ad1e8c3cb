"""Scenes, seeds and schedules of the batch tests.

tests/test_batch_cpu.py runs the ORACLE alone over every case here and asserts that it stays finite to the last
checkpoint; tests/test_gpu_batch.py runs the same cases through BatchEngine and compares bit for bit.  A case is a dict:
  bufs     one layout.Buffers per scene (None: the scene is never uploaded), all of the batch's capacity
  layout, cap = (max_particles, max_beams) per scene, mode (0 off / 1 collisions on), subticks
  program  what happens after the uploads, applied to the batch and to one oracle per scene alike:
             ("frame", n) ("step", n) ("delete",) ("consts", scene, c8) ("input", bytes32) ("inputs", [bytes32 per scene])
"""
import numpy as np

OFF, ALLPAIRS, GRID = 0, 1, 2


def fit(sb, src, max_particles, max_beams):
    """The (identity-mapped) scene of `src` in Buffers of another capacity, constants and user input included."""
    P, B = src.particle_count, src.beam_count
    out = sb.Buffers(src.layout, max_particles, max_beams)
    out.set_scene(src.particles[:P], src.beams[:B].copy())
    out.metadata[12:28] = src.metadata[12:28]
    return out


def two_particles(sb, layout, cap, x=500.0, y=300.0, vx=0.0):
    buf = sb.Buffers(layout, *cap)
    pts = np.zeros((2, 6), "f4")
    pts[:, 0] = (x, x + 25.0)
    pts[:, 1] = y
    pts[:, 2] = (vx, -vx)
    beams = np.zeros(1, sb.layout.BEAM_DTYPE[layout])
    beams[0]["a"], beams[0]["b"] = 0, 1
    for f, v in (("length", 30.0), ("target_length", 30.0), ("last_length", 30.0), ("spring", 50.0), ("damp", 700.0),
                 ("yield_strain", 0.2), ("strain_break_limit", 0.5)):
        beams[0][f] = v
    buf.set_scene(pts, beams)
    return buf


def empty_scene(sb, layout, cap):
    buf = sb.Buffers(layout, *cap)
    buf.set_scene(np.zeros((0, 6), "f4"), np.zeros(0, sb.layout.BEAM_DTYPE[layout]))
    return buf


def case_default(sb, layout):
    """The reference's default scene (119 / 299), collisions on, 3 frames; the GPU test replicates it over 64 scenes."""
    return dict(name="default v%d" % layout, layout=layout, cap=(128, 320), mode=ALLPAIRS,
                bufs=[sb.scenes.default_buffers(layout, 128, 320)], program=[("frame", 1)] * 3)


def case_hetero(sb):
    """Scenes of different sizes and topologies in one batch, different physics constants each, 2 frames + 7 substeps."""
    cap, L = (1024, 4096), 2
    lat12 = sb.scenes.lattice_buffers(12, 12, d=30.0, origin=(100.0, 300.0), strain_limit=0.5, layout=L, velocity=(3.0, -2.0))
    lat32 = sb.scenes.lattice_buffers(32, 32, d=25.0, origin=(100.0, 100.0), spring=50.0, damp=700.0, yield_strain=0.2,
                                      strain_limit=0.5, jitter=2.0, layout=L)
    assert lat32.particle_count == cap[0]
    bufs = [sb.scenes.default_buffers(L, *cap), fit(sb, lat12, *cap), fit(sb, lat32, *cap), two_particles(sb, L, cap, vx=4.0),
            empty_scene(sb, L, cap), None]
    consts = [[0.0, -0.5, 0.5, 0.2, 0.5, 0.1, 0.001, 2.0], [0.1, -0.8, 0.4, 0.3, 0.6, 0.2, 0.002, 2.0],
              [-0.05, -0.3, 0.6, 0.1, 0.4, 0.05, 0.0005, 3.0], [0.0, -1.0, 0.3, 0.25, 0.7, 0.15, 0.002, 2.5],   # 2.5: general pow
              [0.0, -0.5, 0.5, 0.2, 0.5, 0.1, 0.001, 2.0]]
    program = [("consts", i, np.array(c, "f4")) for i, c in enumerate(consts)] + [("frame", 2), ("step", 7)]
    return dict(name="heterogeneous", layout=L, cap=cap, mode=ALLPAIRS, bufs=bufs, program=program)


# 0.5 .. 1.5 is the range the feature was specified with.  The oracle removes beams at EVERY one of them (41, 107, 161, 234, 319
# of 385 after 3 frames), so a sixth, gentler throw (0.2: none removed; 0.3 already loses 4) is added for the scene that must
# stay whole beside them; the five are all kept.
BREAK_SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 0.2)


def case_break(sb):
    """test_yield_break_and_delete's lattice (12 x 12 thrown at the wall, v1, slack 8), initial velocities scaled per scene."""
    bufs = [sb.scenes.lattice_buffers(12, 12, d=30.0, origin=(30.0, 30.0), spring=50.0, damp=100.0, yield_strain=0.05,
                                      strain_limit=0.12, layout=1, velocity=(-40.0 * s, -35.0 * s), slack=8) for s in BREAK_SCALES]
    return dict(name="yield / break / delete", layout=1, cap=(bufs[0].max_particles, bufs[0].max_beams), mode=ALLPAIRS,
                bufs=bufs, program=[("frame", 1)] * 3)


def permuted_default(sb):
    """test_nonidentity_mapping's construction: slots need not equal data indices (engineMapping.ts:336-339)."""
    buf = sb.scenes.default_buffers(2, 256, 512)
    rng = np.random.default_rng(3)
    P, B = buf.particle_count, buf.beam_count
    pp, bp = rng.permutation(P), rng.permutation(B)
    newp = np.zeros_like(buf.particles)
    newp[pp + 50] = buf.particles[:P]
    newb = np.zeros_like(buf.beams)
    bb = buf.beams[:B].copy()
    bb["a"] = pp[bb["a"]] + 50
    bb["b"] = pp[bb["b"]] + 50
    newb[bp + 100] = bb
    buf.particles[:] = newp
    buf.beams[:] = newb
    buf.mapping[:P] = rng.permutation(pp + 50)
    buf.mapping[buf.max_particles:buf.max_particles + B] = rng.permutation(bp + 100)
    return buf


def coincident(sb):
    """Particles on one spot: compute.wgsl:151-154 separates them by the sign of (DATA index - other DATA index), which a
    mapping that is not the identity makes differ from the slot order."""
    buf = sb.Buffers(2, 256, 512)
    idx = np.array([40, 3, 17, 5, 29, 8])
    pos = [(300.0, 300.0), (300.0, 300.0), (500.0, 500.0), (500.0, 500.0), (500.0, 500.0), (700.0, 200.0)]
    for d, p in zip(idx, pos):
        buf.particles[d, :2] = p
    buf.mapping[:6] = idx
    rec = buf.beams[9]
    rec["a"], rec["b"] = 40, 8
    L = np.float32(np.sqrt(np.float32(400.0 ** 2 + 100.0 ** 2)))
    for f, v in (("length", L), ("target_length", L), ("last_length", L), ("spring", 3.0), ("damp", 50.0), ("yield_strain", 2.0),
                 ("strain_break_limit", 5.0)):
        rec[f] = v
    buf.mapping[buf.max_particles] = 9
    buf.particle_count, buf.beam_count = 6, 1
    return buf


def case_mapping(sb):
    return dict(name="permuted mapping + coincident particles", layout=2, cap=(256, 512), mode=ALLPAIRS,
                bufs=[permuted_default(sb), coincident(sb)], program=[("frame", 1)])


def user_inputs(sb, k):
    """Per-scene user input of round k for 4 scenes: different applied forces, scene 2 with the mouse grab active."""
    out = []
    for i in range(4):
        b = sb.Buffers(1, 4, 4)
        b.user_strength = 1.0 + 0.25 * i
        b.set_user_input(applied_force=(0.1 * i - 0.05 * k, 0.05 * i * (k + 1)), mouse_pos=(200.0 + 20.0 * k, 150.0),
                         mouse_vel=(4.0, 2.0 - k), mouse_active=(i == 2))
        out.append(b.user_input_bytes())
    return out


def case_inputs(sb):
    """Per-scene actions from a device tensor, changed between frames; then the host broadcast form."""
    buf = sb.scenes.default_buffers(1, 128, 320)
    return dict(name="user input", layout=1, cap=(128, 320), mode=ALLPAIRS, bufs=[buf.copy() for _ in range(4)],
                program=[("inputs", user_inputs(sb, 0)), ("frame", 1), ("inputs", user_inputs(sb, 1)), ("frame", 1),
                         ("input", user_inputs(sb, 2)[2]), ("frame", 1)])


def saturation_scene(sb):
    """test_force_saturation_and_nonfinite's scene: absurd springs push the fixed-point force past +-2^31, one beam has length 0."""
    P = [[100, 100, 0, 0, 0, 0], [220, 100, 0, 0, 0, 0], [100, 300, 0, 0, 0, 0], [100, 420, 0, 0, 0, 0],
         [400, 400, 0, 0, 0, 0], [400, 400, 0, 0, 0, 0]]
    buf = sb.Buffers(2, 8, 8)
    bb = np.zeros(3, sb.layout.BEAM_DTYPE[2])
    bb[0] = (0, 1, 100, 100, 100, 1e9, 0, 5, 50, 0, 0)
    bb[1] = (2, 3, 140, 140, 140, 3e8, 0, 5, 50, 0, 0)
    bb[2] = (4, 5, 50, 50, 50, 1e30, 0, 5, 50, 0, 0)
    buf.set_scene(np.array(P, "f4"), bb)
    buf.set_physics_constants(gravity=(0.0, 0.0), border_elasticity=0.5, border_friction=0.2, elasticity=0.5,
                              friction=0.1, drag_coeff=0.0, drag_exp=2.0)
    return buf


def case_saturation(sb):
    cap = (8, 8)
    return dict(name="force saturation", layout=2, cap=cap, mode=OFF,
                bufs=[two_particles(sb, 2, cap), saturation_scene(sb), two_particles(sb, 2, cap, vx=2.0)], program=[("step", 1)])


def case_reset(sb):
    """What the reset, state I/O, engine-agreement and independence tests run on the oracle's side: the default scene for 4
    frames (2 + 2), and 2 frames + 5 substeps."""
    return dict(name="default scene, 4 frames + 5 substeps", layout=1, cap=(128, 320), mode=ALLPAIRS,
                bufs=[sb.scenes.default_buffers(1, 128, 320)], program=[("frame", 1)] * 4 + [("step", 5)])


def all_cases(sb):
    return [case_default(sb, 1), case_default(sb, 2), case_hetero(sb), case_break(sb), case_mapping(sb), case_inputs(sb),
            case_saturation(sb), case_reset(sb)]


def make_oracle(orc, case, buf):
    ref = orc.OracleEngine(1000.0, 10.0, case.get("subticks", 64), case["layout"], ALLPAIRS if case["mode"] else OFF, threads=4)
    ref.write_buffers(buf)
    return ref


def apply_to_oracles(refs, op):
    """One op of a case's program on the per-scene oracles (None entries: never uploaded)."""
    for i, ref in enumerate(refs):
        if ref is None:
            continue
        if op[0] == "frame":
            for _ in range(op[1]):
                ref.frame()
        elif op[0] == "step":
            ref.step(op[1])
        elif op[0] == "delete":
            ref.delete_pass()
        elif op[0] == "consts":
            if op[1] == i:
                ref.set_physics_constants(op[2])
        elif op[0] == "input":
            ref.write_user_input(op[1])
        elif op[0] == "inputs":
            ref.write_user_input(op[1][i])
        else:
            raise ValueError(op)


def run_oracles(orc, case, checkpoint=None):
    """One oracle per uploaded scene through the whole program; checkpoint(refs, op_index) after every op."""
    refs = [None if b is None else make_oracle(orc, case, b) for b in case["bufs"]]
    for k, op in enumerate(case["program"]):
        apply_to_oracles(refs, op)
        if checkpoint:
            checkpoint(refs, k)
    return refs


def assert_same(got, exp, what=""):
    """tests/test_gpu_parity.py's comparison, restated: counts, metadata, mapping equal, every particle float and the whole
    beam buffer equal as bytes.  No tolerance."""
    P, B = exp.particle_count, exp.beam_count
    assert (got.particle_count, got.beam_count) == (P, B), what
    assert np.array_equal(got.metadata, exp.metadata), what
    assert np.array_equal(got.mapping, exp.mapping), what
    gp, ep = got.particles.view("<u4"), exp.particles.view("<u4")
    bad = np.nonzero((gp != ep).any(axis=1))[0]
    assert bad.size == 0, "%s: %d particles differ, first %d: %s vs %s" % (
        what, bad.size, bad[0], got.particles[bad[0]], exp.particles[bad[0]])
    assert got.beams.tobytes() == exp.beams.tobytes(), what + ": beam state differs"
