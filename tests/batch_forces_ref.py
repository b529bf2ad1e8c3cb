"""The outputs of sb_batch_forces_device (include/softbody.h) restated in plain numpy float32: the reference of
tests/test_gpu_batch_forces.py and, alone, of tests/test_batch_forces_cpu.py.  No grid, no LDS: beams in one vector expression,
contacts partner by partner in ascending slot order.

Every operator is np.float32 (one IEEE rounding each; np.sqrt and / are correctly rounded).  A scene is a layout.Buffers as
load_scene / OracleEngine.load_buffers return it: its beam slots are ALL evaluated -- a beam with a pending break flag is still in
the slot list until a delete pass, a removed one is not.  Results are indexed by DATA index.

Three deliberately wrong variants (tests/test_batch_forces_cpu.py shows that the cases tell them apart): descending=True sums the
contacts in descending slot order, saturate=False converts without saturation, skip_slots leaves beam slots out (as a model that
drops beams with a pending flag would)."""
import numpy as np

F = np.float32
WORDS, COUNT_WORDS = 8, 4
FIELDS = ("beam_x", "beam_y", "push_x", "push_y", "impulse_x", "impulse_y", "depth", "partners")
INT_MAX, INT_MIN = np.int32(2 ** 31 - 1), np.int32(-2 ** 31)
FORCE_SCALE = F(65536.0)            # compute.wgsl:70
STRESS_SCALE = F(1.0) / F(20.0)     # compute.wgsl:71


def f32_to_i32(x, saturate=True):
    """v_cvt_i32_f32: truncate toward zero, saturate, NaN -> 0.  saturate=False (a WRONG variant): wrap modulo 2^32 instead."""
    x = np.asarray(x, F)
    out = np.zeros(x.shape, np.int32)
    with np.errstate(invalid="ignore"):
        nan = np.isnan(x)
        big, small = x >= F(2147483648.0), x <= F(-2147483648.0)
    mid = ~(nan | big | small)
    out[mid] = np.trunc(x[mid]).astype(np.int64).astype(np.int32)
    if saturate:
        out[big], out[small] = INT_MAX, INT_MIN
    else:
        far = (big | small) & np.isfinite(x)
        out[far] = (np.fmod(np.trunc(x[far].astype(np.float64)), 2.0 ** 32).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    return out


def beam_eval(ax, ay, bx, by, target, last, spring, damp, saturate=True):
    """compute.wgsl:103-130 on arrays: (force_mag, i32 contributions [n, 4] = ax, ay, bx, by)."""
    ax, ay, bx, by, target, last, spring, damp = (np.asarray(v, F) for v in (ax, ay, bx, by, target, last, spring, damp))
    with np.errstate(all="ignore"):
        dx, dy = bx - ax, by - ay
        len0 = np.sqrt(dx * dx + dy * dy)
        degenerate = len0 == F(0.0)                                       # :104-107
        dx = np.where(degenerate, F(0.0), dx)
        dy = np.where(degenerate, F(-1.0e-10), dy)
        length = np.where(degenerate, np.sqrt(F(0.0) * F(0.0) + F(-1.0e-10) * F(-1.0e-10)), len0)
        inv_len = F(1.0) / length
        force_mag = (target - length) * spring + (last - length) * damp   # :110
        nx, ny = dx * inv_len, dy * inv_len
        fx, fy = force_mag * nx, force_mag * ny                           # :111
        sx, sy = fx * FORCE_SCALE, fy * FORCE_SCALE
        assert all(v.dtype == F for v in (len0, length, inv_len, force_mag, sx, sy))
    words = np.stack([f32_to_i32(-sx, saturate), f32_to_i32(-sy, saturate), f32_to_i32(sx, saturate), f32_to_i32(sy, saturate)], axis=-1)
    return force_mag.astype(F), words


def _clamp(x, lo, hi):
    """sb_clamp: min(max(x, lo), hi) with sb_max(a, b) = a < b ? b : a, sb_min(a, b) = b < a ? b : a"""
    m = np.where(x < lo, lo, x)
    return np.where(hi < m, hi, m)


def contact_terms(dx, dy, dist, ux, uy, two_r, friction, elasticity_coeff, inv_dt2, dt2):
    """What one partner at (dx, dy), dist > 0, subtracts: (push_x, push_y, impulse_x, impulse_y) of compute.wgsl:156-168, arrays."""
    with np.errstate(all="ignore"):
        inv_dist = F(1.0) / dist
        nx, ny = dx * inv_dist, dy * inv_dist
        tx, ty = -ny, nx
        impulse_normal = elasticity_coeff * (ux * nx + uy * ny)
        max_friction = impulse_normal * friction
        impulse_tangent = _clamp(ux * tx + uy * ty, -max_friction, max_friction)
        ix, iy = impulse_normal * nx + impulse_tangent * tx, impulse_normal * ny + impulse_tangent * ty
        overlap = two_r - dist
        csx, csy = nx * overlap * F(0.5), ny * overlap * F(0.5)
        if inv_dt2 != F(0.0):
            px, py = csx * inv_dt2, csy * inv_dt2
        else:
            px, py = csx / dt2, csy / dt2
    return px.astype(F), py.astype(F), ix.astype(F), iy.astype(F)


def inv_dt2_of(subticks):
    """(inv_dt2, dt2) as sb_batch_create makes them: time_step = 1 / subticks (subticks rounded up to even) in float32; inv_dt2 =
    1 / dt2 where dt2 is a power of two, else 0 ("divide")."""
    subticks = (int(subticks) + 1) // 2 * 2
    dt = F(1.0) / F(subticks)
    dt2 = F(dt * dt)
    bits = int(np.asarray(dt2).view(np.uint32))
    pow2 = (bits & 0x007FFFFF) == 0 and 1 < (bits >> 23) < 253
    return (F(1.0) / dt2 if pow2 else F(0.0)), dt2


def never_uploaded(max_particles, max_beams):
    return (np.zeros((max_particles, WORDS), F), np.zeros((max_particles, 2), np.int32), np.zeros(max_beams, F), np.zeros(COUNT_WORDS, np.int32))


def forces_ref(buf, radius=10.0, subticks=64, labels=None, other_body=False, descending=False, saturate=True, skip_slots=()):
    """(rows [maxP, 8] float32, beam_i32 [maxP, 2] int32, tension [maxB] float32, counts [4] int32) of one scene."""
    maxP, maxB, P, Bc = buf.max_particles, buf.max_beams, buf.particle_count, buf.beam_count
    rows, beam_i32, tension, counts = never_uploaded(maxP, maxB)
    if other_body and labels is None:
        raise ValueError("forces_ref: other_body needs labels")
    if P == 0:
        return rows, beam_i32, tension, counts
    idx = buf.mapping[:P].astype(np.int64)                                  # data index per particle slot
    pos, vel = buf.particles[idx, 0:2].astype(F), buf.particles[idx, 2:4].astype(F)
    # ---- beam part: every beam slot
    slots = np.array([j for j in range(Bc) if j not in set(skip_slots)], np.int64)
    bd = buf.mapping[maxP + slots].astype(np.int64)                         # data index per beam slot
    rec = buf.beams[bd]
    a, b = rec["a"].astype(np.int64), rec["b"].astype(np.int64)
    pa, pb = buf.particles[a, 0:2].astype(F), buf.particles[b, 0:2].astype(F)
    force_mag, words = beam_eval(pa[:, 0], pa[:, 1], pb[:, 0], pb[:, 1], rec["target_length"], rec["last_length"], rec["spring"], rec["damp"], saturate)
    acc = np.zeros((maxP, 2), np.uint32)                                    # wrapping 32-bit adds
    u = words.view(np.uint32)
    np.add.at(acc[:, 0], a, u[:, 0])
    np.add.at(acc[:, 1], a, u[:, 1])
    np.add.at(acc[:, 0], b, u[:, 2])
    np.add.at(acc[:, 1], b, u[:, 3])
    beam_i32[idx] = acc.view(np.int32)[idx]
    tension[bd] = force_mag
    rows[idx, 0:2] = beam_i32[idx].astype(F) * F(2.0 ** -16)                # sb_particle_integrate's exact product
    # ---- contact part: partners in ascending slot order
    two_r = F(radius) * F(2.0)
    c = buf.metadata.view("<f4")
    elasticity_coeff, friction = (F(c[16]) + F(1.0)) / F(2.0), F(c[17])
    inv_dt2, dt2 = inv_dt2_of(subticks)
    with np.errstate(all="ignore"):
        dx, dy = pos[None, :, 0] - pos[:, None, 0], pos[None, :, 1] - pos[:, None, 1]     # [s, o]: other - self
        dist = np.sqrt(dx * dx + dy * dy)
        assert dist.dtype == F
        t = (dist == F(0.0)) | (dist < two_r)
    t[np.arange(P), np.arange(P)] = False
    if other_body:
        lab = np.asarray(labels)[idx]
        t &= lab[None, :] != lab[:, None]
    n_partners = t.sum(axis=1)
    order = np.argsort(~t, axis=1, kind="stable")                           # partners first, ascending slot order
    push, impulse, depth = np.zeros((P, 2), F), np.zeros((P, 2), F), np.zeros(P, F)
    for k in range(int(n_partners.max()) if P else 0):
        s = np.nonzero(n_partners > k)[0]
        o = order[s, n_partners[s] - 1 - k] if descending else order[s, k]
        d = dist[s, o]
        with np.errstate(all="ignore"):
            overlap = two_r - d
            depth[s] = np.where(overlap > depth[s], overlap, depth[s])
            px, py, ix, iy = contact_terms(dx[s, o], dy[s, o], d, vel[s, 0] - vel[o, 0], vel[s, 1] - vel[o, 1], two_r, friction, elasticity_coeff,
                                           inv_dt2, dt2)
            on_spot = d == F(0.0)                                           # counts, depth 2r, adds nothing
            push[s, 0] = np.where(on_spot, push[s, 0], push[s, 0] - px)
            push[s, 1] = np.where(on_spot, push[s, 1], push[s, 1] - py)
            impulse[s, 0] = np.where(on_spot, impulse[s, 0], impulse[s, 0] - ix)
            impulse[s, 1] = np.where(on_spot, impulse[s, 1], impulse[s, 1] - iy)
    rows[idx, 2:4], rows[idx, 4:6], rows[idx, 6], rows[idx, 7] = push, impulse, depth, n_partners.astype(F)
    with np.errstate(invalid="ignore"):
        counts[:] = (P, len(slots), int((n_partners > 0).sum()), int((~np.isfinite(force_mag)).sum()))
    return rows, beam_i32, tension, counts


def partner_records(buf, radius=10.0):
    """Per particle slot the float32 rows {dx, dy, dist, ux, uy} of its partners in ascending slot order: what
    tests/batch_forces_check.cpp feeds to csrc/sb_batch_forces_math.h."""
    P = buf.particle_count
    idx = buf.mapping[:P].astype(np.int64)
    pos, vel = buf.particles[idx, 0:2].astype(F), buf.particles[idx, 2:4].astype(F)
    two_r = F(radius) * F(2.0)
    out = []
    with np.errstate(all="ignore"):
        for s in range(P):
            dx, dy = pos[:, 0] - pos[s, 0], pos[:, 1] - pos[s, 1]
            dist = np.sqrt(dx * dx + dy * dy)
            t = (dist == F(0.0)) | (dist < two_r)
            t[s] = False
            o = np.nonzero(t)[0]
            out.append(np.stack([dx[o], dy[o], dist[o], vel[s, 0] - vel[o, 0], vel[s, 1] - vel[o, 1]], axis=1).astype(F))
    return out


def stack(results):
    return tuple(np.stack([r[k] for r in results]) for k in range(4))


def forces_of(bufs_now, max_particles, max_beams, radius=10.0, subticks=64, labels=None, other_body=False):
    """The four arrays of a batch from one Buffers per scene (None: never uploaded); labels: int32 [n, maxP] or None."""
    out = []
    for i, b in enumerate(bufs_now):
        if b is None:
            out.append(never_uploaded(max_particles, max_beams))
        else:
            out.append(forces_ref(b, radius, subticks, None if labels is None else labels[i], other_body))
    return stack(out)


def words(a):
    """An output as uint32 words for the exact comparison, every NaN as one word: the payload and sign of a NaN an operation makes
    differ between the CPU and the GPU (as tests/batch_contacts_cases.py notes of the oracle), a NaN's being one does not."""
    a = np.ascontiguousarray(a)
    if a.dtype != F:
        return a.view(np.uint32)
    w = a.view(np.uint32).copy()
    w[np.isnan(a)] = 0x7FC00000
    return w
