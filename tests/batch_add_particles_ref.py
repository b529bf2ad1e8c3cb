"""sb_batch_add_particles_device's definition (include/softbody.h) restated in numpy float32 on layout.Buffers: the
scene as load_scene returned it in, the edited buffers, `result` and `counts` out.  It restates the rule row by row, not the kernel:
no bitmap, no ballot, no ranks -- a Python loop over the rows and a sorted list of free indices.  reset_ref is the reset rule on a
(current, reset, P0) triple."""
import numpy as np

F = np.float32
EMPTY, INVALID, BLOCKED, FULL = -1, -2, -3, -4
DRY_RUN, SKIP_TOUCHING = 1, 2
ROW_WORDS = 8


def pack(rows):
    """(tag, x, y[, vx, vy, ax, ay[, reserved]]) rows -> sb_batch_new_particle words, int32 [k, 8]"""
    out = np.zeros((len(rows), ROW_WORDS), dtype=np.int32)
    for i, r in enumerate(rows):
        r = tuple(r)
        out[i, 0] = int(r[0])
        f = np.zeros(6, F)
        f[:len(r[1:7])] = np.asarray(r[1:7], dtype=F)
        out[i, 1:7] = f.view(np.int32)
        out[i, 7] = int(r[7]) if len(r) > 7 else 0
    return out


def held(buf):
    """bool [max_particles] by DATA index: "a slot < P of the particle mapping names d" (the constant blob's byte)"""
    out = np.zeros(buf.max_particles, dtype=bool)
    out[buf.mapping[:buf.particle_count].astype(np.int64)] = True
    return out


def touch(p, q, radius):
    """the step's contact test on two positions: dist = sqrt(dx * dx + dy * dy) in float32, one rounding per operator; touching
    when dist == 0 or dist < 2 * radius (a NaN or infinite distance touches nothing)"""
    with np.errstate(all="ignore"):
        dx, dy = F(q[0]) - F(p[0]), F(q[1]) - F(p[1])
        dist = np.sqrt(F(F(dx * dx) + F(dy * dy)), dtype=F)
        return bool(dist == F(0.0) or dist < F(radius) * F(2.0))


def row_verdict(row, loaded):
    """steps 1 and 2 of the definition on one row (int32 [8]): EMPTY / INVALID / 0 = candidate"""
    if int(row[0]) < 0:
        return EMPTY
    xy = np.asarray(row[1:3], dtype=np.int32).view(F)
    if not loaded or int(row[7]) != 0 or not np.isfinite(xy).all():
        return INVALID
    return 0


def add_ref(buf, rows, flags=0, radius=10.0, holds=None):
    """buf: the scene as load_scene returned it (None: never uploaded); rows: int32 [k, 8]; holds: the "holds a particle" bytes
    where the caller keeps them itself (None: held(buf), which the invariant says they are).  Returns (edited copy of buf -- buf
    itself with DRY_RUN, None for None --, result int32 [k], counts [added, invalid, blocked, full])."""
    rows = np.ascontiguousarray(rows).view(np.int32).reshape(-1, ROW_WORDS)
    k = len(rows)
    result, counts = np.zeros(k, dtype=np.int32), [0, 0, 0, 0]
    verd = [row_verdict(rows[j], buf is not None) for j in range(k)]
    if buf is None:
        for j in range(k):
            result[j] = verd[j]
            counts[1] += int(verd[j] == INVALID)
        return None, result, counts
    maxP, P = buf.max_particles, buf.particle_count
    pos = rows[:, 1:3].copy().view(F)
    here = buf.particles[buf.mapping[:P].astype(np.int64), :2]
    E = [verd[j] == 0 and any(touch(pos[j], q, radius) for q in here) for j in range(k)]
    holds = held(buf) if holds is None else holds
    free = [d for d in range(maxP) if not holds[d]]
    out = buf.copy()
    added = 0
    for j in range(k):
        code = verd[j]
        if code == 0 and flags & SKIP_TOUCHING:
            if E[j] or any(verd[i] == 0 and not E[i] and touch(pos[j], pos[i], radius) for i in range(j)):
                code = BLOCKED
        if code == 0 and not (P + added < maxP and added < len(free)):
            code = FULL
        if code != 0:
            result[j] = code
            if code != EMPTY:
                counts[{INVALID: 1, BLOCKED: 2, FULL: 3}[code]] += 1
            continue
        d = free[added]
        out.particles[d] = rows[j, 1:7].view(F)
        out.mapping[P + added] = d
        added += 1
        result[j] = d
    counts[0] = added
    out.particle_count = P + added
    return (buf if flags & DRY_RUN else out), result, counts


def reset_ref(current, reset, p0):
    """The reset rule on a triple: `current` is the scene as load_scene returns it now, `reset` as it returned it when the reset
    state was made (upload, checkpoint, fork), p0 the particle count of that moment.  Returns (the scene after the reset, its
    "holds a particle" bytes): the reset state's particle rows, beams and beam mapping; the particle mapping stays the CURRENT one
    (it lives in the constant blob: entries at and past p0 are stale, never read); the slots p0 .. P - 1 give their data indices
    back; physics constants and user input stay.  (Beam records of indices that are not alive in the reset state are outside this
    restatement: an undone weld leaves its material there.)"""
    maxP = current.max_particles
    assert p0 <= current.particle_count and reset.particle_count == p0
    out = reset.copy()
    out.mapping[:maxP] = current.mapping[:maxP]
    out.metadata[12:28] = current.metadata[12:28]
    out.particle_count = p0
    return out, held(out)
