"""sb_batch_add_beams_device's definition (include/softbody.h) restated in numpy float32 on layout.Buffers: the
scene as load_scene returned it plus the reset state's alive set in, the edited buffers, `result` and `counts` out.  It restates the
rule row by row, not the kernel: no inverse table, no bitmap, no ranks -- a Python loop over the rows with a set of joined pairs
and a sorted list of free indices."""
import numpy as np

F = np.float32
EMPTY, INVALID, JOINED, FULL = -1, -2, -3, -4
DRY_RUN, LENGTH_CURRENT, SKIP_JOINED = 1, 2, 4
ROW_WORDS = 8


def pack(rows):
    """(a, b, length, spring, damp, yield_strain, strain_break_limit[, reserved]) rows -> sb_batch_new_beam words, int32 [k, 8]"""
    out = np.zeros((len(rows), ROW_WORDS), dtype=np.int32)
    for i, r in enumerate(rows):
        out[i, 0], out[i, 1] = int(r[0]), int(r[1])
        out[i, 2:7] = np.asarray(r[2:7], dtype=F).view(np.int32)
        out[i, 7] = int(r[7]) if len(r) > 7 else 0
    return out


def alive_set(buf):
    """bool [max_beams] by DATA index: the beams a live slot of `buf` (as uploaded or read back) names"""
    out = np.zeros(buf.max_beams, dtype=bool)
    out[buf.mapping[buf.max_particles:buf.max_particles + buf.beam_count].astype(np.int64)] = True
    return out


def distance(pa, pb):
    """the beam phase's sb_length(pb.x - pa.x, pb.y - pa.y): float32, one rounding per operator"""
    with np.errstate(all="ignore"):
        dx, dy = F(pb[0]) - F(pa[0]), F(pb[1]) - F(pa[1])
        return np.sqrt(F(F(dx * dx) + F(dy * dy)), dtype=F)


def row_verdict(row, flags, max_particles, loaded, holds, current):
    """steps 1 and 2 of the definition on one row (int32 [8]): (EMPTY / INVALID / 0 = candidate, resolved length).  holds: bool
    [max_particles] "the data index of a particle slot < P"; current: the endpoints' current distance (looked at when both hold)"""
    a, b = int(row[0]), int(row[1])
    if a < 0:
        return EMPTY, F(0)
    if not loaded or a >= max_particles or b >= max_particles or b < 0 or a == b or not holds[a] or not holds[b] or int(row[7]) != 0:
        return INVALID, F(0)
    length = F(current) if flags & LENGTH_CURRENT else np.asarray(row[2:3], dtype=np.int32).view(F)[0]
    if not (np.isfinite(length) and length > 0):
        return INVALID, F(0)
    return 0, length


def add_ref(buf, rows, flags=0, reset_alive=None):
    """buf: the scene as load_scene returned it (None: never uploaded); rows: int32 [k, 8]; reset_alive: bool [max_beams], the
    alive set of the scene's reset state (None: nothing but what is alive now).  Returns (edited copy of buf -- buf itself with
    DRY_RUN, None for None --, result int32 [k], counts [added, invalid, joined, full])."""
    rows = np.ascontiguousarray(rows).view(np.int32).reshape(-1, ROW_WORDS)
    k = len(rows)
    result, counts = np.zeros(k, dtype=np.int32), [0, 0, 0, 0]
    if buf is None:
        for j in range(k):
            result[j] = EMPTY if rows[j, 0] < 0 else INVALID
            counts[1] += int(rows[j, 0] >= 0)
        return None, result, counts
    maxP, maxB = buf.max_particles, buf.max_beams
    P, Bc = buf.particle_count, buf.beam_count
    holds = np.zeros(maxP, dtype=bool)
    holds[buf.mapping[:P].astype(np.int64)] = True
    live = buf.mapping[maxP:maxP + Bc].astype(np.int64)
    alive = alive_set(buf)
    free = [d for d in range(maxB) if not alive[d] and not (reset_alive is not None and reset_alive[d])]
    joined = {frozenset((int(buf.beams["a"][d]), int(buf.beams["b"][d]))) for d in live}
    out = buf.copy()
    added = 0
    for j in range(k):
        a, b = int(rows[j, 0]), int(rows[j, 1])
        both = 0 <= a < maxP and 0 <= b < maxP and holds[a] and holds[b]
        current = distance(buf.particles[a], buf.particles[b]) if both else F(0)
        code, length = row_verdict(rows[j], flags, maxP, True, holds, current)
        if code == 0 and flags & SKIP_JOINED:
            if frozenset((a, b)) in joined:
                code = JOINED
            else:
                joined.add(frozenset((a, b)))       # (a later row of the same pair is joined, whether this one finds room or not)
        if code == 0 and not (Bc + added < maxB and added < len(free)):
            code = FULL
        if code != 0:
            result[j] = code
            if code != EMPTY:
                counts[{INVALID: 1, JOINED: 2, FULL: 3}[code]] += 1
            continue
        d, slot = free[added], Bc + added
        added += 1
        result[j] = d
        f = rows[j, 2:7].view(F)
        for name, v in (("a", a), ("b", b), ("length", length), ("target_length", length), ("last_length", current), ("spring", f[1]),
                        ("damp", f[2]), ("yield_strain", f[3]), ("strain_break_limit", f[4]), ("strain", 0.0), ("stress", 0.0)):
            out.beams[name][d] = v
        out.mapping[maxP + slot] = d
    counts[0] = added
    out.beam_count = Bc + added
    return (buf if flags & DRY_RUN else out), result, counts
