"""Scenes at the edges of the exact-arithmetic gates (csrc/sb_physics.h: sb_sqrt_gated / sb_rcp_gated and the wave-uniform
tests in front of them), hand-made so that ONE launch holds lanes on both sides of a gate.

tests/test_gate_cases_cpu.py runs the ORACLE alone over every case: finite at every checkpoint, and every case bites -- counted
in binary32 from the oracle's READ states, some beam / pair / particle lies outside the gate the case names, and in the mixed
cases at least 64 times as many lie inside it.  tests/test_gpu_gate_edges.py runs the same cases through every schedule that
contains the gate and compares bit for bit.  A case is a dict:
  name, gates   the rows of GATES whose device code the case reaches with lanes on both sides (or beyond an edge); a case with no
                gate of its own is a parity companion of the one beside it
  buf           layout.Buffers (layout 2, physics constants in its metadata), bounds, radius
  modes         collision modes of the single-engine runs; batch: also as scene 2 of a BatchEngine beside plain lattices
  checkpoints   substep counts after which states are compared
  blocked       None: not run on the blocked kernel; True / False: whether the host lets the scene into it
  mixed         one launch holds both sides of the gate (the 64 : 1 condition applies)
  bite(reads)   {gate: (inside, outside)} summed over the READ states of the compared substeps, over the population the gate
                ballots: beams, particles; for `contact dist` the pairs in contact (0 < dist < 2r), for `contact d2` the pairs whose
                root the list walk takes (d2 <= (2r)^2 * 1.001); plus "notes"
"""
import numpy as np

import batch_cases as bc

F = np.float32
OFF, ALLPAIRS, GRID = 0, 1, 2
GATES = ("beam len2", "blocked 1/length", "mirrored", "contact d2", "contact dist", "drag v2")
SEED = 7                                      # the base lattice's jitter
NAMES = ["M1 zero-length beam", "M1 zero-length beam, spread", "M2 spring 1200 stretched by 20", "M2 spring 1200 stretched by 20, spread",
         "M2 spring 2e+29 stretched by 20", "M3 drag exponent 2", "M3 drag exponent 2.5", "M4 two particles 1e-15 apart",
         "M5 rest length 1e-20, spring 1e-18, material mode 1", "M5 rest length 1e-20, spring 3e-15, material mode 1",
         "M5 rest length 1e-20, spring 1e-18, material mode 2", "M5 rest length 1e-20, spring 3e-15, material mode 2",
         "scaled world 2^-50", "scaled world 2^-47", "scaled world 2^40", "scaled world 2^44", "scaled world 2^46"]
SQRT_LO, SQRT_HI = F(2.0) ** -90, F(2.0) ** 90
RCP_LO, RCP_HI = F(2.0) ** -45, F(2.0) ** 45
QUIET = dict(gravity=(0.0, 0.0), border_elasticity=0.5, border_friction=0.2, elasticity=0.5, friction=0.1, drag_coeff=0.0, drag_exp=2.0)


# ---------------------------------------------------------------- what a substep's READ state puts in front of each gate
def beam_terms(st):
    """Per active beam, in binary32 and in the order of compute.wgsl:103-111: len2, the larger |component| of force * 65536,
    the rest length."""
    B, maxP = st.beam_count, st.max_particles
    rec = st.beams[st.mapping[maxP:maxP + B].astype(np.int64)]
    a, b = rec["a"].astype(np.int64), rec["b"].astype(np.int64)
    with np.errstate(all="ignore"):
        dx, dy = st.particles[b, 0] - st.particles[a, 0], st.particles[b, 1] - st.particles[a, 1]
        len2 = dx * dx + dy * dy
        ln = np.sqrt(len2)
        zero = ln == 0
        dx, dy, ln = np.where(zero, F(0.0), dx), np.where(zero, F(-1.0e-10), dy), np.where(zero, F(1.0e-10), ln)
        mag = (rec["target_length"] - ln) * rec["spring"] + (rec["last_length"] - ln) * rec["damp"]
        inv = F(1.0) / ln
        fx, fy = mag * (dx * inv) * F(65536.0), mag * (dy * inv) * F(65536.0)
        big = np.maximum(np.abs(fx), np.abs(fy))
    return len2, big, rec["length"]


def pair_terms(st, radius):
    """Every pair i < j of the collision scan: d2, dist, and whether it is a contact the reciprocal gate sees (0 < dist < 2r)."""
    P = st.particle_count
    p = st.particles[st.mapping[:P].astype(np.int64), :2]
    i, j = _triangle(P)
    with np.errstate(all="ignore"):
        dx, dy = p[j, 0] - p[i, 0], p[j, 1] - p[i, 1]
        d2 = dx * dx + dy * dy
        dist = np.sqrt(d2)
    return d2, dist, (dist > 0) & (dist < F(radius) * F(2.0))


_triangles = {}


def _triangle(P):
    if P not in _triangles:
        _triangles[P] = np.triu_indices(P, 1)
    return _triangles[P]


def in_range(x, lo, hi):
    return (x >= lo) & (x <= hi)


def split(ok, sel=None):
    ok = ok if sel is None else ok[sel]
    return int(ok.sum()), int((~ok).sum())


def make_bite(gates, radius):
    def bite(reads, contacts=True):
        tot = {g: [0, 0] for g in gates}
        notes = dict(f_30_31=0, f_sat=0, contacts_outside_dist=0, contacts_inside_dist=0, v2_subnormal=0, len2_zero=0)
        for st in reads:
            len2, big, rest = beam_terms(st)
            P = st.particle_count
            v = st.particles[st.mapping[:P].astype(np.int64), 2:4]
            v2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]
            notes["f_30_31"] += int(((big >= F(2.0) ** 30) & (big < F(2.0) ** 31)).sum())
            notes["f_sat"] += int((big >= F(2.0) ** 31).sum())
            notes["len2_zero"] += int((len2 == 0).sum())
            notes["v2_subnormal"] += int(((v2 > 0) & (v2 < F(2.0) ** -126)).sum())
            per = {"beam len2": split(in_range(len2, SQRT_LO, SQRT_HI)), "blocked 1/length": split(in_range(rest, RCP_LO, RCP_HI)),
                   "mirrored": split(big < F(2.0) ** 30), "drag v2": split(in_range(v2, SQRT_LO, SQRT_HI) | (v2 == 0))}
            if contacts and ("contact d2" in gates or "contact dist" in gates):
                d2, dist, contact = pair_terms(st, radius)
                # the list walk takes the root of every entry with d2 <= (2r)^2 * 1.001 (sb_collide_list), zero included
                near = d2 <= F(radius) * F(2.0) * (F(radius) * F(2.0)) * F(1.001)
                ok2, okd = in_range(d2, SQRT_LO, SQRT_HI), in_range(dist, RCP_LO, RCP_HI)
                per["contact d2"] = (int((ok2 & near).sum()), int((~ok2 & near).sum()))
                per["contact dist"] = (int((okd & contact).sum()), int((~okd & contact).sum()))
                notes["contacts_outside_dist"] += int((~okd & contact).sum())
                notes["contacts_inside_dist"] += int((okd & contact).sum())
            for g in gates:
                if g not in per:
                    continue
                tot[g][0] += per[g][0]
                tot[g][1] += per[g][1]
        out = {g: tuple(v) for g, v in tot.items()}
        out["notes"] = notes
        return out
    return bite


def case(name, gates, buf, *, modes, checkpoints=(1, 23), blocked=None, batch=True, mixed=True, bounds=1000.0, radius=10.0):
    return dict(name=name, gates=tuple(gates), buf=buf, modes=tuple(modes), checkpoints=tuple(checkpoints), blocked=blocked,
                batch=batch, mixed=mixed, bounds=float(bounds), radius=float(radius), bite=make_bite(gates, radius))


# ---------------------------------------------------------------- mixed-wave cases
def base_lattice(sb, extra_particles=0, consts=None):
    """24 x 20, d = 25, jitter 2, spring 50, damp 700, yield 0.3, strain limit 1e9: 480 particles, 1790 beams (bounds 1000, radius
    10): eight waves of particles, twenty-nine of beams, eight tiles of 64."""
    src = sb.scenes.lattice_buffers(24, 20, d=25.0, origin=(100.0, 100.0), spring=50.0, damp=700.0, yield_strain=0.3,
                                    strain_limit=1.0e9, anti_diagonal=True, jitter=2.0, layout=2, seed=SEED)
    buf = bc.fit(sb, src, src.particle_count + extra_particles, src.beam_count) if extra_particles else src
    if consts:
        buf.set_physics_constants(**consts)
    return buf


def disjoint_beams(buf, stride):
    """From the middle of every run of `stride` beams, the first axis-parallel beam (rest length 25: stretched by 20 under spring
    1200 its larger force component is 1.57e9 of 2^31 = 2.15e9; a diagonal's stays below 2^30) whose endpoints no earlier pick touches."""
    used, out = set(), []
    for first in range(stride // 2, buf.beam_count, stride):
        for j in range(first, min(first + stride // 2, buf.beam_count)):
            a, b = int(buf.beams["a"][j]), int(buf.beams["b"][j])
            if buf.beams["length"][j] == 25.0 and a not in used and b not in used:
                used.update((a, b))
                out.append(j)
                break
    return out


ONE_RUN = 12                                  # the single offender of M1, M2 and M5 sits in the middle of this run of 64 beams
SPREAD = 128                                  # "spread" variants: one offender in every run of 128 beams -- every other wave of the
                                              # beam kernel is mixed, the ones between are not (one per 64 cannot have 64 : 1 inside)


def offenders(buf, spread):
    return disjoint_beams(buf, SPREAD) if spread else [one_beam(buf)]


def one_beam(buf):
    return [j for j in disjoint_beams(buf, 64) if j // 64 == ONE_RUN][0]


def case_m1(sb, spread=False):
    """Zero-length beams: endpoint B moved onto endpoint A, so len2 == 0, the guard of compute.wgsl:104-107 fires and the beam
    points along (0, -1)."""
    buf = base_lattice(sb, consts=QUIET)
    for j in offenders(buf, spread):
        a, b = int(buf.beams["a"][j]), int(buf.beams["b"][j])
        buf.particles[b, :2] = buf.particles[a, :2]
    return case("M1 zero-length beam" + (", spread" if spread else ""), ["beam len2"], buf, modes=[OFF], blocked=True)


def stretch(buf, j, by):
    """Endpoint B of beam j moved `by` units away from A along the beam; last_length follows (it is the length the substep before
    would have left behind), so the force of the first substep is the spring term alone."""
    a, b = int(buf.beams["a"][j]), int(buf.beams["b"][j])
    d = buf.particles[b, :2].astype(np.float64) - buf.particles[a, :2].astype(np.float64)
    buf.particles[b, :2] = (buf.particles[b, :2] + d / np.hypot(*d) * by).astype("f4")
    dx, dy = buf.particles[b, 0] - buf.particles[a, 0], buf.particles[b, 1] - buf.particles[a, 1]
    buf.beams["last_length"][j] = np.sqrt(dx * dx + dy * dy)


def case_m2(sb, spring=1200.0, spread=False):
    """|f * 65536| in [2^30, 2^31): nothing saturates, and the blocked kernel's `mirrored` gate still refuses the wave.  Spring
    2e29 instead: that one lane saturates among ordinary ones."""
    buf = base_lattice(sb, consts=QUIET)
    for j in offenders(buf, spread):
        buf.beams["spring"][j] = spring
        stretch(buf, j, 20.0)
    what = "M2 spring %g stretched by 20" % spring + (", spread" if spread else "")
    return case(what, ["mirrored"], buf, modes=[OFF], blocked=True)


M3_TINY = (5, 70, 133, 200, 333)              # v = (1e-25, -3e-26): both squares round to 0 in binary32, v2 == 0 with v != 0
M3_SUBNORMAL = (17, 128, 191, 300, 479)       # v = (1e-21, -3e-22): v2 = 1.09e-42, subnormal
M3_REST = (9, 64, 190, 257, 400)              # v = 0


def case_m3(sb, drag_exp):
    """Drag 0.002, gravity 0, every particle moving at a few units per second except fifteen: five at rest, five so slow that v2
    underflows to zero, five whose v2 is subnormal (the drag gate's IEEE branch beside ordinary lanes)."""
    buf = base_lattice(sb, consts=dict(QUIET, drag_coeff=0.002, drag_exp=drag_exp))
    P = buf.particle_count
    buf.particles[:P, 2:4] = (sb.scenes.hash_uniform(SEED + 1, 2 * P).reshape(P, 2) * 3.0).astype("f4")
    buf.particles[list(M3_TINY), 2:4] = (1.0e-25, -3.0e-26)
    buf.particles[list(M3_SUBNORMAL), 2:4] = (1.0e-21, -3.0e-22)
    buf.particles[list(M3_REST), 2:4] = 0.0
    return case("M3 drag exponent %g" % drag_exp, ["drag v2"], buf, modes=[OFF, ALLPAIRS, GRID], blocked=True)


M4_NUDGE = 9.5                                # with jitter 2 the nudged neighbours end up 11.5 .. 19.5 apart in x, at most 4 in y: < 2r


def case_m4(sb):
    """Two free particles 1.1e-15 apart outside the box: 0 < dist < 2^-45 and d2 < 2^-90 on the first substep, coincident on the
    wall clamps (dist == 0) on the second.  Beside them ordinary contacts for the same ballots: in every other column of the
    lattice every other particle is nudged 9.5 towards its neighbour in the next column (120 pairs closer than 2r, in every wave of
    the particle kernel, the offenders' included)."""
    buf = base_lattice(sb, extra_particles=2, consts=QUIET)
    P = buf.particle_count
    for x in range(0, 24, 2):
        for y in range(1, 20, 2):
            buf.particles[x * 20 + y, 0] += F(M4_NUDGE)
    pts = buf.particles[:P + 2].copy()
    pts[P] = (1.0e-15, 1.0e-15, 1.0, 2.0, 0.0, 0.0)
    pts[P + 1] = (2.0e-15, 1.5e-15, -1.0, 0.0, 0.0, 0.0)
    consts = buf.metadata[12:28].copy()
    buf.set_scene(pts, buf.beams[:buf.beam_count].copy())
    buf.metadata[12:28] = consts
    return case("M4 two particles 1e-15 apart", ["contact dist", "contact d2"], buf, modes=[ALLPAIRS, GRID], checkpoints=(1, 2))


def case_m5(sb, mode, spring):
    """One beam whose rest length, target_length and last_length are 1e-20 between endpoints an ordinary distance apart.  Material
    mode 1: every beam rests at its present length (no two alike: more rows than the blocked plan's dictionary of 256 holds, so
    rest lengths travel per beam there).  Spring 1e-18 lies below the blocked kernel's range (2^-50) and
    takes the single-substep kernel; spring 3e-15 is inside it, and the blocked kernel's own 1/length gates run."""
    buf = base_lattice(sb, consts=QUIET)
    j = one_beam(buf)                             # (chosen before the rest lengths change)
    if mode == 1:
        sb.scenes.rest_at_current_length(buf)
    for f in ("length", "target_length", "last_length"):
        buf.beams[f][j] = 1.0e-20
    buf.beams["spring"][j] = spring
    blocked = bool(abs(spring) >= 2.0 ** -50)
    # the device's 1/length gates are compiled for per-beam rest lengths only (mode 2 reads the host's table) and sit in the blocked
    # kernel: one of the four reaches them, the others are its parity companions
    c = case("M5 rest length 1e-20, spring %g, material mode %d" % (spring, mode), ["blocked 1/length"] if blocked and mode == 1 else [],
             buf, modes=[OFF], blocked=blocked)
    c["material_mode"] = mode
    return c


# ---------------------------------------------------------------- whole-launch cases: the same small world, scaled by 2^k
def case_scaled(sb, k):
    """12 x 11 lattice (d = 25, jitter 2) whose first two columns and rows lie outside the box, everything with a length times
    2^k: positions, the three beam lengths, bounds, radius.  No gravity, no drag, at rest.  The first substep clamps the outer
    columns and rows onto the walls: beams between them shrink to the jitter or to nothing, the corner's four particles coincide.
      k = -50, -47   len2 straddles 2^-90 beam by beam; contacts closer than 2^-45
      k = +40        beside the upper edge: the axis-parallel beams (len2 up to 841 * 2^80) and every contact are inside the gates,
                     the diagonals (1250 * 2^80 > 2^90) already outside -- the upper edge straddled beam by beam
      k = +44, +46   len2 above 2^90 for every beam that is not degenerate, forces saturate, contacts farther than 2^45"""
    s = 2.0 ** k
    buf = sb.scenes.lattice_buffers(12, 11, d=25.0, origin=(-18.0, -18.0), spring=50.0, damp=700.0, yield_strain=0.3,
                                    strain_limit=1.0e9, jitter=2.0, layout=2, seed=SEED + 2)
    buf.set_physics_constants(**QUIET)
    buf.particles[:, :2] *= F(s)
    for f in ("length", "target_length", "last_length"):
        buf.beams[f] *= F(s)
    modes = [OFF, ALLPAIRS] + ([GRID] if k in (-47, 44) else [])
    gates = ["beam len2"] if k == 40 else ["beam len2", "contact dist", "contact d2"]
    return case("scaled world 2^%d" % k, gates, buf, modes=modes, checkpoints=(1, 20 if k >= 44 else 23), blocked=True, batch=False,
                mixed=False, bounds=1000.0 * s, radius=10.0 * s)


SCALES = (-50, -47, 40, 44, 46)


def all_cases(sb):
    out = [case_m1(sb), case_m1(sb, spread=True), case_m2(sb), case_m2(sb, spread=True), case_m2(sb, spring=2.0e29),
           case_m3(sb, 2.0), case_m3(sb, 2.5), case_m4(sb)]
    out += [case_m5(sb, mode, spring) for mode in (1, 2) for spring in (1.0e-18, 3.0e-15)]
    out += [case_scaled(sb, k) for k in SCALES]
    return out


def ref_mode(mode):
    """The oracle's collision scan for an engine mode: the spatial hash is compared with the all-pairs loop."""
    return ALLPAIRS if mode == GRID else mode


def make_oracle(orc, c, mode, buf=None):
    ref = orc.OracleEngine(c["bounds"], c["radius"], 64, 2, ref_mode(mode), threads=1)
    ref.write_buffers(c["buf"] if buf is None else buf)
    return ref


def oracle_states(orc, c, mode, buf=None, reads=False):
    """The oracle's state after each checkpoint ({substeps: Buffers}); reads=True: also the READ state of every substep."""
    buf = c["buf"] if buf is None else buf
    ref = make_oracle(orc, c, mode, buf)
    out, seen, done = {}, [], 0
    for n in c["checkpoints"]:
        while done < n:
            if reads:
                seen.append(ref.load_buffers(buf.copy()))
                ref.step(1)
                done += 1
            else:
                ref.step(n - done)
                done = n
        out[n] = ref.load_buffers(buf.copy())
    return (out, seen) if reads else out
