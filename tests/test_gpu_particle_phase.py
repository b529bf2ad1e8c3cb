"""The particle phase of the blocked kernel (csrc/sb_blocked.hip) where its wave-level shortcuts can go wrong: the wall block
behind one ballot per wave, the drag chain with its at-rest lanes masked out, the force scale as a multiplication.

Every case runs the scene n = 1, 7 and 13 substeps in ONE call on a fresh blocked engine (13 = a launch of 7 and the launch that
ends the call, which also writes strain / stress) and compares, as uint32 views (test_gpu_parity.assert_same), with the same
scene stepped one substep per launch and with the oracle.  Scenes that hold a NaN or an infinity are compared with the
single-substep kernel only: which NaN an invalid operation returns (sign, payload) is the processor's choice, so the CPU oracle
is no reference for those bits -- the kernel that shares sb_particle_finish is.
Tiles of 64 particles: an 8 x 6 lattice is one tile, a 40 x 30 lattice nineteen with halo slots all around."""
import json
import os
import signal
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gate_cases as gc  # noqa: E402
from test_gpu_parity import GRID, OFF, TILED, assert_same  # noqa: E402

pytestmark = pytest.mark.gpu
LIMIT_S = 60                                  # per case, set-up included: a case takes a few seconds


@pytest.fixture(autouse=True)
def time_limit():
    """Every case under a time limit of its own: a hung launch fails the case instead of holding the suite."""
    def expired(signum, frame):
        raise TimeoutError("case exceeded %d s" % LIMIT_S)
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(LIMIT_S)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


F = np.float32
NS = (1, 7, 13)
K = 7
BOUNDS, RADIUS = 2000.0, 10.0   # (a 40 x 30 lattice at spacing 25 from (300, 300) lies well inside)
LO, HI = F(RADIUS), F(BOUNDS) - F(RADIUS)
CONSTS = dict(gravity=(0.0, -9.81), border_elasticity=0.5, border_friction=0.2, elasticity=0.5, friction=0.1, drag_coeff=0.002, drag_exp=2.0)


def lattice(sb, nx, ny, origin=(300.0, 300.0), jitter=1.0, consts=None, **kw):
    buf = sb.scenes.lattice_buffers(nx, ny, d=25.0, origin=origin, spring=50.0, damp=700.0, yield_strain=0.3, strain_limit=1.0e9,
                                    jitter=jitter, layout=2, seed=11, **kw)
    buf.set_physics_constants(**dict(CONSTS, **(consts or {})))
    return buf


def velocities(sb, buf, scale, seed=5):
    """Both signs in both components, a few units per second."""
    P = buf.particle_count
    buf.particles[:P, 2:4] = (sb.scenes.hash_uniform(seed, 2 * P).reshape(P, 2) * scale).astype("f4")


def engine(sb, buf, block, mode=OFF):
    eng = sb.Engine(bounds_size=BOUNDS, particle_radius=RADIUS, subticks=64, layout=2, max_particles=buf.max_particles,
                    max_beams=buf.max_beams, collision_mode=mode, path=TILED, tile_particles=64, block_substeps=block)
    eng.write_buffers(buf)
    return eng


def stepped(sb, buf, n, block, between=None, must_block=True):
    eng = engine(sb, buf, block)
    if block > 1 and must_block:
        assert eng.info("substeps_per_launch") == block, "the scene must run on the blocked kernel"
    eng.step(n)
    if between:
        between(eng)
        eng.step(n)
    out = eng.load_buffers(buf.copy())
    eng.destroy()
    return out


def check(sb, oracle, buf, what, with_oracle=True, between=None, must_block=True):
    """blocked == one substep per launch (== oracle) after n substeps (and n more behind `between`), for n in NS."""
    for n in NS:
        got = stepped(sb, buf, n, K, between, must_block)
        one = stepped(sb, buf, n, 1, between)
        assert_same(got, one, "%s: blocked vs single substeps, n = %d" % (what, n))
        if with_oracle:
            ref = oracle.OracleEngine(BOUNDS, RADIUS, 64, 2, OFF, threads=1)
            ref.write_buffers(buf)
            ref.step(n)
            if between:
                between(ref)
                ref.step(n)
            exp = ref.load_buffers(buf.copy())
            assert_same(got, exp, "%s: blocked vs oracle, n = %d" % (what, n))


# ---------------------------------------------------------------- walls
WALL_SPOTS = {
    "floor": lambda p: (p[0], LO),
    "below the floor": lambda p: (p[0], LO - F(3.0)),
    "side wall": lambda p: (HI, p[1]),
    "past the side wall": lambda p: (HI + F(0.5), p[1]),
    "corner": lambda p: (LO, LO),
    "past the corner": lambda p: (HI + F(2.0), LO - F(2.0)),
}


@pytest.mark.parametrize("elasticity", [0.0, 0.5])
@pytest.mark.parametrize("spot", sorted(WALL_SPOTS))
@pytest.mark.parametrize("size", [(8, 6), (40, 30)])
def test_one_lane_at_the_wall(sb, oracle, size, spot, elasticity):
    """One particle of an interior lattice put on, or past, a wall (its beams stretch: finite all the same), once for each sign
    of its velocity components; the other 63 lanes of its wave never see a wall.  8 x 6: the wave is the tile."""
    for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        buf = lattice(sb, *size, consts=dict(border_elasticity=elasticity))
        velocities(sb, buf, 2.0)
        i = buf.particle_count // 2 + 3
        buf.particles[i, :2] = WALL_SPOTS[spot](buf.particles[i, :2])
        buf.particles[i, 2:4] = (sx * 40.0, sy * 25.0)
        check(sb, oracle, buf, "%s, v signs %+d %+d, elasticity %g" % (spot, sx, sy, elasticity))


@pytest.mark.parametrize("elasticity", [0.0, 0.5])
@pytest.mark.parametrize("spot", sorted(WALL_SPOTS))
def test_one_particle_alone(sb, oracle, spot, elasticity):
    """A scene of ONE particle and no beam, on or past a wall, every sign pattern of its velocity: one lane, one wave, one tile
    (wherever the host routes a scene without beams: compared all the same)."""
    for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        buf = lattice(sb, 1, 1, consts=dict(border_elasticity=elasticity))
        assert (buf.particle_count, buf.beam_count) == (1, 0)
        buf.particles[0, :2] = WALL_SPOTS[spot](buf.particles[0, :2])
        buf.particles[0, 2:4] = (sx * 40.0, sy * 25.0)
        check(sb, oracle, buf, "one particle, %s, v signs %+d %+d, elasticity %g" % (spot, sx, sy, elasticity), must_block=False)


@pytest.mark.parametrize("elasticity", [0.0, 0.5])
def test_lattice_pressed_into_the_corner(sb, oracle, elasticity):
    """40 x 30 with its first column on the left wall and its first row on the floor, moving into both: wall particles in most
    tiles, each also a halo particle of the tiles next door (the redundant copies must be the owner's, or the beams between
    disagree a substep later), interior waves beside them."""
    buf = lattice(sb, 40, 30, origin=(10.0, 10.0), jitter=0.0, consts=dict(border_elasticity=elasticity))
    velocities(sb, buf, 30.0)
    buf.particles[:buf.particle_count, 2:4] += np.array([-20.0, -30.0], "f4")
    check(sb, oracle, buf, "corner lattice, elasticity %g" % elasticity)


# ---------------------------------------------------------------- drag gate
def drag_lattice(sb, drag_exp=2.0):
    buf = lattice(sb, 40, 30, consts=dict(gravity=(0.0, 0.0), drag_exp=drag_exp))
    velocities(sb, buf, 3.0)
    return buf


FINITE_V = [(0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (2.0 ** -46, 0.0), (-(2.0 ** -46), 2.0 ** -47), (1.0e-25, -3.0e-26),
            (1.0e-21, -3.0e-22), (1.0e-40, 0.0), (-1.0e-40, 1.0e-41)]   # (the last two: subnormal COMPONENTS)


def test_drag_gate_mixed_in_one_wave(sb, oracle):
    """Lanes at rest (+0, -0) and with |v|^2 below 2^-90 (zero after rounding, subnormal, ordinary), a few to every
    wave of ordinary lanes: the wave takes the IEEE branch, and in the waves around them the short forms run with lanes at rest."""
    buf = drag_lattice(sb)
    for k, v in enumerate(FINITE_V * 3):
        buf.particles[20 + 43 * k, 2:4] = v
    rest = np.arange(7, buf.particle_count, 64)   # one lane at rest in EVERY wave: the masked lanes of the short form
    buf.particles[rest, 2:4] = 0.0
    check(sb, oracle, buf, "drag gate, finite edges")


@pytest.mark.parametrize("v", [(2.0 ** 46, 0.0), (-(2.0 ** 45), 2.0 ** 45), (np.inf, 0.0), (1.0, -np.inf), (np.nan, 0.0), (0.0, np.nan)], ids=str)
def test_drag_gate_huge_or_nonfinite_velocity(sb, oracle, v):
    """|v|^2 above 2^90 (its drag overflows within a few substeps: infinities, then NaN), infinite and NaN velocities -- in ONE
    wave with every finite edge lane of the case above (particles 320 .. 383 are a wave of the 64-particle tiles) and ordinary lanes."""
    buf = drag_lattice(sb)
    buf.particles[333, 2:4] = v
    for k, fv in enumerate(FINITE_V):
        buf.particles[321 + 5 * k + (5 * k >= 12), 2:4] = fv
    buf.particles[np.arange(7, buf.particle_count, 64), 2:4] = 0.0
    check(sb, oracle, buf, "drag gate, v = %s" % (v,), with_oracle=False)


# ---------------------------------------------------------------- force scale
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def i32(x):
    """compute.wgsl's i32(f) as the device has it: truncation, saturating, NaN -> 0."""
    x = np.nan_to_num(np.asarray(x, dtype=np.float64), nan=0.0, posinf=1.0e300, neginf=-1.0e300)
    return np.clip(np.trunc(x), INT_MIN, INT_MAX).astype(np.int64)


def force_sums(buf):
    """The fixed-point force sums (x, y) every particle collects in the substep that READS `buf`, in binary32 and in the order of
    compute.wgsl:103-111, 127-130: B gets i32(f * 65536), A gets i32(-f * 65536)."""
    B, P = buf.beam_count, buf.particle_count
    rec = buf.beams[:B]
    a, b = rec["a"].astype(np.int64), rec["b"].astype(np.int64)
    with np.errstate(all="ignore"):
        dx, dy = buf.particles[b, 0] - buf.particles[a, 0], buf.particles[b, 1] - buf.particles[a, 1]
        ln = np.sqrt(dx * dx + dy * dy)
        assert (ln > 0).all()
        mag = (rec["target_length"] - ln) * rec["spring"] + (rec["last_length"] - ln) * rec["damp"]
        inv = F(1.0) / ln
        fx, fy = mag * (dx * inv) * F(65536.0), mag * (dy * inv) * F(65536.0)
    S = np.zeros((P, 2), np.int64)
    for k, f in enumerate((fx, fy)):
        np.add.at(S[:, k], b, i32(f))
        np.add.at(S[:, k], a, i32(-f.astype(np.float64)))
    return S


def force_scale_scene(sb):
    """An 8 x 6 lattice at rest (every beam at its rest length: every sum exactly 0) in which a few axis-parallel beams, no two
    sharing a particle across sites, are one unit off their targets, without damping:
      spring 1.5 / 65536                       sums of +1 and -1 at its ends
      spring 2e29, once longer, once shorter   i32 saturates: INT_MAX at one end, INT_MIN at the other, in both directions
      spring 256 into a particle that a beam of spring 1.5 / 65536 leaves: 2^24 and 1 on the same particle, in both signs --
                                               +-(2^24 + 1), the first integer its conversion to binary32 rounds"""
    buf = lattice(sb, 8, 6, jitter=0.0, consts=dict(gravity=(0.0, 0.0), drag_coeff=0.0))
    sb.scenes.rest_at_current_length(buf)
    B = buf.beam_count
    axis = [j for j in range(B) if buf.beams["length"][j] == 25.0]
    used = set()

    def ends(j):
        return int(buf.beams["a"][j]), int(buf.beams["b"][j])

    def take(candidates):
        """The first candidate (a tuple of beams) none of whose particles an earlier site uses."""
        for js in candidates:
            pts = set(p for j in js for p in ends(j))
            if not (pts & used):
                used.update(pts)
                return js
        raise AssertionError("no free site left")

    def off_target(j, spring, by):
        buf.beams["spring"][j], buf.beams["damp"][j] = spring, 0.0
        buf.beams["target_length"][j] = buf.beams["length"][j] + F(by)

    chains = [(j1, j2) for j1 in axis for j2 in axis if ends(j1)[1] == ends(j2)[0]]   # j1 ends where j2 starts
    for s in (1.0, -1.0):
        j1, j2 = take(chains)
        off_target(j1, 256.0, s)                  # into the shared particle as B: s * 2^24
        off_target(j2, 1.5 / 65536.0, -s)         # out of it as A: s * 1
    for spring, by in ((2.0e29, 1.0), (2.0e29, -1.0), (1.5 / 65536.0, 1.0), (1.5 / 65536.0, -1.0)):
        (j,) = take([(j,) for j in axis])
        off_target(j, spring, by)
    return buf


def test_force_sum_edges(sb, oracle):
    """The division by the force scale as a multiplication by 2^-16, over the edge integers: sums of exactly 0, +-1,
    +-(2^24 + 1), INT_MIN and INT_MAX all arise in the first substep of this scene (counted here from its READ state), and the
    state after it, and after 7 and 13, is the single-substep kernel's and the oracle's."""
    buf = force_scale_scene(sb)
    S = force_sums(buf)
    have = set(S.ravel().tolist())
    for want in (0, 1, -1, 2 ** 24 + 1, -(2 ** 24 + 1), INT_MIN, INT_MAX):
        assert want in have, (want, sorted(have))
    assert F(2 ** 24 + 1) == F(2 ** 24) and (S == 0).all(axis=1).sum() >= 24   # (rounded by the conversion; most particles at rest)
    check(sb, oracle, buf, "force sum edges")


@pytest.mark.parametrize("name", ["M2 spring 1200 stretched by 20, spread", "M2 spring 2e+29 stretched by 20"])
def test_force_sums_at_2_31(sb, oracle, name):
    """tests/gate_cases.py: components of force * 65536 in [2^30, 2^31) in every other wave; one beam whose share saturates."""
    c = [c for c in gc.all_cases(sb) if c["name"] == name][0]
    check(sb, oracle, c["buf"], name)


# ---------------------------------------------------------------- constants in the kernarg
def test_general_constants_change_between_calls(sb, oracle):
    """drag_exp 2.5, the mouse held over some particles, an applied force with user_strength: the general variant; then other
    values (and, in the second round, the plain variant's) behind the first call -- they travel in the kernarg of every launch."""
    def first(buf):
        buf.user_strength = 0.75
        buf.set_user_input(applied_force=(0.3, -0.2), mouse_pos=(560.0, 610.0), mouse_vel=(4.0, -3.0), mouse_active=True)

    def change(to_plain):
        def between(e):
            b = lattice(sb, 8, 6)
            b.user_strength = 0.75
            b.set_user_input(applied_force=(-0.1, 0.4), mouse_pos=(700.0, 500.0), mouse_vel=(-2.0, 1.0), mouse_active=not to_plain)
            e.write_user_input(b.user_input_bytes())
            e.set_physics_constants(np.array([0.05, -5.0, 0.3, 0.1, 0.5, 0.1, 0.004, 2.0 if to_plain else 3.0], "f4"))
        return between

    for to_plain in (False, True):
        buf = lattice(sb, 40, 30, consts=dict(drag_exp=2.5))
        velocities(sb, buf, 3.0)
        first(buf)
        check(sb, oracle, buf, "general constants, then %s" % ("plain" if to_plain else "general"), between=change(to_plain))


# ---------------------------------------------------------------- tracked launches under the spatial hash
TRACK_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "particle_phase_track.json")
TRACK_COUNTERS = ("hybrid_substeps", "hybrid_failed", "grid_builds", "hybrid_launches", "hybrid_validate_launches", "substeps_done")
GRID_CTL_WORDS = 32                           # SbGridCtl (sb_physics.h), word by word; 8 is the running displacement bound


def track_scene(sb):
    return sb.scenes.lattice_buffers(64, 48, d=30.0, origin=(300.0, 900.0), jitter=1.0, layout=2, velocity=(0.4, -1.0)), 3000.0


def track_record(sb, eng):
    return dict(grid_ctl=[int(eng.info("grid_ctl_%d" % i)) for i in range(GRID_CTL_WORDS)], **{k: int(eng.info(k)) for k in TRACK_COUNTERS})


def test_tracked_launches(sb, oracle):
    """A falling lattice with nothing within reach, default collision mode: after the hash is built the run goes to tracked
    blocked launches, whose displacement bound reads p_old and the new p of every own particle.  The hash's decision state after
    each of two calls of 100 substeps -- all 32 words of SbGridCtl, the running bound (word 8, the sums the tracked launches
    reported folded in), its drift and skin among them -- and the counters that follow from the bound (roll-backs, hash builds,
    launches, validations) equal, bit for bit, what the kernel recorded them as before the walls moved behind a ballot
    (tests/golden/particle_phase_track.json); the state equals the oracle's grid mode."""
    buf, bounds = track_scene(sb)
    golden = json.load(open(TRACK_GOLDEN))
    eng = sb.Engine(bounds_size=bounds, subticks=64, layout=2, max_particles=buf.max_particles, max_beams=buf.max_beams, collision_mode=GRID)
    ref = oracle.OracleEngine(bounds, 10.0, 64, 2, GRID, threads=16)
    eng.write_buffers(buf)
    ref.write_buffers(buf)
    seen = []
    for _ in range(2):
        eng.step(100)
        ref.step(100)
        seen.append(track_record(sb, eng))
    got, exp = eng.load_buffers(buf.copy()), ref.load_buffers(buf.copy())
    eng.destroy()
    print("tracked launches:", seen)
    assert seen[-1]["hybrid_substeps"] >= 100, seen
    assert seen == golden["after_each_call_of_100"], (seen, golden)
    assert_same(got, exp, "tracked blocked launches")


# ---------------------------------------------------------------- NaN position
@pytest.mark.parametrize("xy", [(np.nan, None), (None, np.nan), (np.nan, np.nan)], ids=str)
def test_nan_position_in_one_lane(sb, oracle, xy):
    """`p != clamp(p)` is true for a NaN coordinate, so that lane takes both wall branches -- the wave's ballot must say so.  The
    NaN reaches its beam neighbours a substep later; everything is the single-substep kernel's bits.  After ONE substep the
    other lanes of its wave are what they are without the NaN (beams only feed forces from the READ state of their endpoints:
    neighbours change, and only in velocity and position, not in being finite)."""
    buf = lattice(sb, 40, 30)
    velocities(sb, buf, 2.0)
    i = 64 * 9 + 21
    for k, val in enumerate(xy):
        if val is not None:
            buf.particles[i, k] = val
    check(sb, oracle, buf, "NaN position %s" % (xy,), with_oracle=False)
    after = stepped(sb, buf, 1, K)
    P = buf.particle_count
    nan_rows = np.nonzero(~np.isfinite(after.particles[:P]).all(axis=1))[0]
    nb = set([i])
    for a, b in zip(buf.beams["a"][:buf.beam_count], buf.beams["b"][:buf.beam_count]):
        if int(a) == i or int(b) == i:
            nb.update((int(a), int(b)))
    assert set(nan_rows.tolist()) <= nb and i in nan_rows, (nan_rows, sorted(nb))
