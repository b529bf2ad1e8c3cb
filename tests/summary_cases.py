"""Scenes and programs of the tests of Engine.summary() (sb_summary_device), shared by
tests/test_summary_cpu.py (the oracle side alone: no warnings, and that every case bites) and tests/test_gpu_summary.py.

A case is a dict: name, buf (the upload), bounds, mode (the ORACLE's collision mode: 0 off / 1 on), program -- ops applied to the
engine and to the oracle alike: ("frame", n) ("step", n) ("delete",) ("poke", [(data index, column, value)]) -- and compare_after:
the op indices after which the summary is compared with batch_summary_ref.summary_ref (-1: right after the upload)."""
import numpy as np

import batch_cases as bc
import batch_summary_ref as sr

OFF, ALLPAIRS = 0, 1


def case_default(sb, mode=ALLPAIRS):
    """119 / 299 at capacity 120 / 300: W = 128 / 512, below the narrowest cut, so levels are skipped."""
    return dict(name="default 120/300", buf=sb.scenes.default_buffers(1, 120, 300), bounds=1000.0, mode=mode,
                program=[("frame", 2), ("step", 5)], compare_after=[-1, 0, 1])


def case_cut(sb):
    """A 96 x 96 lattice at capacity 10000 / 30000 (W = 16384 / 32768: many leaves to a thread at the narrowest cut), every
    particle with a velocity of its own, of widely different magnitudes, so that no column is trivial; compared as uploaded (the
    magnitudes still apart) and after three substeps."""
    lat = sb.scenes.lattice_buffers(96, 96, d=25.0, origin=(100.0, 100.0), spring=50.0, damp=700.0, yield_strain=0.2, strain_limit=0.5,
                                    jitter=2.0, layout=2)
    buf = bc.fit(sb, lat, 10000, 30000)
    rng = np.random.default_rng(11)
    P = buf.particle_count
    # (magnitudes spread over forty binary orders: the double sums round, so their order shows -- tests/test_summary_cpu.py)
    buf.particles[:P, 2:4] = ((rng.standard_normal((P, 2)) * 3.0 + (0.7, -1.3)) * np.exp2(-rng.integers(0, 40, (P, 2)))).astype("f4")
    return dict(name="96x96 lattice", buf=buf, bounds=4000.0, mode=OFF, program=[("step", 3)], compare_after=[-1, 0])


def permuted(sb, src, max_particles, max_beams, p_off, b_off, seed=3):
    """bc.permuted_default's construction for any identity-mapped scene: records at shuffled data indices behind an offset, the
    mapping shuffled again, so slots, data indices and the engine's own order all differ."""
    buf = sb.Buffers(src.layout, max_particles, max_beams)
    buf.metadata[12:28] = src.metadata[12:28]
    rng = np.random.default_rng(seed)
    P, B = src.particle_count, src.beam_count
    pp, bp = rng.permutation(P), rng.permutation(B)
    buf.particles[pp + p_off] = src.particles[:P]
    bb = src.beams[:B].copy()
    bb["a"] = pp[bb["a"]] + p_off
    bb["b"] = pp[bb["b"]] + p_off
    buf.beams[bp + b_off] = bb
    buf.mapping[:P] = rng.permutation(pp + p_off)
    buf.mapping[max_particles:max_particles + B] = rng.permutation(bp + b_off)
    buf.particle_count, buf.beam_count = P, B
    return buf


def case_capacity(sb):
    """The 8 x 6 lattice at capacity 5000 / 70000 (W = 8192 / 131072), permuted: the tables end far below the capacity."""
    lat = sb.scenes.lattice_buffers(8, 6, d=30.0, origin=(200.0, 300.0), strain_limit=0.5, layout=2, velocity=(3.0, -2.0))
    return dict(name="8x6 in 5000/70000", buf=permuted(sb, lat, 5000, 70000, 50, 100), bounds=1000.0, mode=OFF,
                program=[("frame", 1)], compare_after=[-1, 0])


CLAMP_CAPACITY = (1 << 20) + 1


def case_clamp(sb):
    """The same lattice, permuted, at capacity 2^20 + 1 / 2^20 + 1: W = 2^21 for both trees, where the engine's own cut, W / 4
    clamped to SB_SUMMARY_MAX_PARTIALS = 262 144, is the clamp and no longer W / 4.  Every particle a velocity of its own, spread
    over forty binary orders (case_cut's), so the sums round."""
    lat = sb.scenes.lattice_buffers(8, 6, d=30.0, origin=(200.0, 300.0), strain_limit=0.5, layout=2, velocity=(3.0, -2.0))
    buf = permuted(sb, lat, CLAMP_CAPACITY, CLAMP_CAPACITY, 50, 100)
    rng = np.random.default_rng(12)
    idx = buf.mapping[:buf.particle_count].astype(np.int64)
    buf.particles[idx, 2:4] = ((rng.standard_normal((len(idx), 2)) * 3.0 + (0.7, -1.3)) * np.exp2(-rng.integers(0, 40, (len(idx), 2)))).astype("f4")
    return dict(name="8x6 in 2^20+1/2^20+1", buf=buf, bounds=1000.0, mode=OFF, program=[("frame", 1)], compare_after=[-1, 0])


def default_partials(W):
    """sbm_default_partials of sb_summary.hip: W / 4, at least 256, at most SB_SUMMARY_MAX_PARTIALS"""
    return min(max(W // 4, 256), 262144)


def free_particles(sb, cap, vx):
    """len(vx) free particles at data indices 0 .. in capacity cap / 4, x velocities vx"""
    buf = sb.Buffers(2, cap, 4)
    pts = np.zeros((len(vx), 6), "f4")
    pts[:, 0] = 100.0 + 50.0 * np.arange(len(vx))
    pts[:, 1] = 500.0
    pts[:, 2] = np.asarray(vx, "f4")
    buf.set_scene(pts, np.zeros(0, sb.layout.BEAM_DTYPE[2]))
    return buf


def witness_cases(sb):
    """Uploaded, not stepped.  W = 4: the tree adds leaf 0 to leaf 2 and leaf 1 to leaf 3 first."""
    big = float(2.0 ** 60)
    mk = lambda name, vx: dict(name=name, buf=free_particles(sb, 4, vx), bounds=1000.0, mode=OFF, program=[], compare_after=[-1])
    return [mk("tree order", [big, 1.0, -big]), mk("all -0.0", [-0.0] * 4), mk("-0.0 beside empty leaves", [-0.0, -0.0])]


def zero_sign_scenes(sb, cap=(1024, 0)):
    """Two scenes of two free particles at data indices 0 and 256 -- at capacity 1024 both leaves of thread 0 of the batch's kernel,
    which the tree visits in that order -- whose x, y, vx, vy are all zeros: A holds +0.0 at index 0 and -0.0 at index 256, B the
    signs swapped.  Either way a minimum is -0.0 and a maximum +0.0: the keys order -0.0 below +0.0."""
    out = []
    for first in (0.0, -0.0):
        buf = sb.Buffers(2, *cap)
        pts = np.zeros((2, 6), "f4")
        pts[0, :4], pts[1, :4] = first, -first
        buf.set_scene(pts, np.zeros(0, sb.layout.BEAM_DTYPE[2]))
        buf.particles[256], buf.particles[1] = buf.particles[1].copy(), 0.0
        buf.mapping[1] = 256
        out.append(dict(name="zeros %s first" % ("+0.0" if first == 0.0 and not np.signbit(first) else "-0.0"), buf=buf, bounds=1000.0,
                        mode=OFF, program=[], compare_after=[-1]))
    return out


def case_nonfinite(sb):
    """After a frame a NaN coordinate in one particle and an infinite velocity in another; one substep later the beams on them
    are not finite either."""
    c = case_default(sb, OFF)
    c.update(name="non-finite", program=[("frame", 1), ("poke", [(7, 0, np.nan), (40, 3, np.inf)]), ("step", 1)], compare_after=[2])
    return c


BREAK_STEPS = 40   # substeps into the throw at which flags are pending (asserted in tests/test_summary_cpu.py)


def case_break(sb):
    """batch_cases.case_break's lattice at scale 1.0: pending flags mid-frame, removed beams after the delete pass."""
    buf = bc.case_break(sb)["bufs"][2]
    return dict(name="breaking lattice", buf=buf, bounds=1000.0, mode=OFF,
                program=[("step", BREAK_STEPS), ("delete",), ("frame", 1)], compare_after=[0, 1, 2])


def all_cases(sb):
    return ([case_default(sb), case_default(sb, OFF), case_cut(sb), case_capacity(sb)] + witness_cases(sb) + [case_nonfinite(sb), case_break(sb)] +
            [case_clamp(sb)])


def make_oracle(orc, case):
    ref = orc.OracleEngine(case["bounds"], 10.0, 64, case["buf"].layout, case["mode"], threads=4)
    ref.write_buffers(case["buf"])
    return ref


def poke_records(particles, pokes):
    for d, col, v in pokes:
        particles[d, col] = v


def apply_to_oracle(ref, op):
    if op[0] == "poke":
        poke_records(ref.particles_b if ref.final_in_b else ref.particles_a, op[1])
    else:
        bc.apply_to_oracles([ref], op)


def apply_to_engine(eng, op):
    if op[0] == "frame":
        for _ in range(op[1]):
            eng.frame()
    elif op[0] == "step":
        eng.step(op[1])
    elif op[0] == "delete":
        eng.delete_pass()
    elif op[0] == "poke":
        t = eng.state_tensors()["particles"]
        for d, col, v in op[1]:
            t[d, col] = float(v)
        eng.write_particles_device(t)
    else:
        raise ValueError(op)


def expected_now(ref, case):
    """(row, counts) of the oracle's state now: the row is summary_ref's, the counts the same integers."""
    row = sr.summary_ref(ref.load_buffers(case["buf"].copy()), case["buf"], sr.pending_of(ref))
    counts = np.array([int(row[k]) for k in range(6)] + [1, 0], dtype=np.uint64)   # (scenes of the tests: all below 2^24)
    return row, counts


def expected(orc, case):
    """{op index: (row, counts)} and the oracle at the end."""
    ref, out = make_oracle(orc, case), {}
    if -1 in case["compare_after"]:
        out[-1] = expected_now(ref, case)
    for k, op in enumerate(case["program"]):
        apply_to_oracle(ref, op)
        if k in case["compare_after"]:
            out[k] = expected_now(ref, case)
    return out, ref
