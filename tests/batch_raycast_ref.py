"""The outputs of sb_batch_raycast_device (include/softbody.h) restated in numpy: the reference of
tests/test_gpu_batch_raycast*.py and, against csrc/sb_batch_ray_math.h on the host, of tests/test_batch_raycast_cpu.py.

Everything is float32 with one rounding per operator, in the order the definition writes them: numpy's float32 +, -, *, / and sqrt
are correctly rounded, and no expression here is fused.  The geometry of a scene is defined on what load_scene returns: the particle
slots 0 .. particle_count-1 of the mapping at their records' positions, the beam slots 0 .. beam_count-1 whatever their break flags
say (`drop`: data indices the caller wants left out -- the WRONG model that forgets that a pending beam still counts).  The winner
is the smallest 64-bit key (bits(t) << 32) | (kind << 16) | index; model="first" is the other WRONG model, which takes the first
meeting in slot order (particles, beams, walls) instead of the nearest."""
import collections

import numpy as np

F = np.float32
ROW_WORDS, HIT_WORDS, COUNT_WORDS, RAY_MAX = 8, 3, 4, 256
PARTICLES, BEAMS, WALLS = 1, 2, 4
MISS, PARTICLE, BEAM, WALL, EMPTY, INVALID = 0, 1, 2, 3, -1, -2
WALL_LEFT, WALL_RIGHT, WALL_LOW, WALL_HIGH = 1, 2, 4, 8
HIT_FIELDS = ("kind", "index", "label")
COUNT_FIELDS = ("valid", "particles", "beams", "walls")
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
INF = float("inf")

RayCast = collections.namedtuple("RayCast", "t hit counts")
Geometry = collections.namedtuple("Geometry", "pidx px py plab bidx ax ay bx by blab")


def pack(rows):
    """uint32 [k, 8] from tuples (mask, ox, oy, dx, dy, tmax[, skip_label[, reserved]])"""
    out = np.zeros((len(rows), ROW_WORDS), np.uint32)
    for i, r in enumerate(rows):
        r = tuple(r) + (-1, 0)[len(r) - 6:]
        out[i, 0] = r[0]
        out[i, 1:6] = np.asarray(r[1:6], F).view(np.uint32)
        out[i, 6] = np.int64(r[6]) & 0xFFFFFFFF
        out[i, 7] = r[7]
    return out


def geometry(buf, labels=None, drop=()):
    """what a ray can meet in one scene (None: never uploaded), in slot order; labels: int32 [max_particles] or None"""
    if buf is None:
        e, z = np.zeros(0, np.int64), np.zeros(0, F)
        return Geometry(e, z, z, e, e, z, z, z, z, e)
    maxP = buf.max_particles
    lab = np.full(maxP, -1, np.int64) if labels is None else np.asarray(labels, np.int64)
    pidx = buf.mapping[:buf.particle_count].astype(np.int64)
    live = buf.mapping[maxP:maxP + buf.beam_count].astype(np.int64)      # entries behind beam_count are stale: never met
    bidx = live[~np.isin(live, np.asarray(list(drop), np.int64))]
    a, b = buf.beams["a"][bidx].astype(np.int64), buf.beams["b"][bidx].astype(np.int64)
    pos = buf.particles.astype(F)
    return Geometry(pidx, pos[pidx, 0], pos[pidx, 1], lab[pidx], bidx, pos[a, 0], pos[a, 1], pos[b, 0], pos[b, 1], lab[a])


def verdict(w, has_labels):
    """MISS (the row is cast), EMPTY or INVALID, from the row's eight words"""
    w = np.asarray(w, np.uint32)
    if w[0] == 0:
        return EMPTY
    f = w.view(F)
    if w[0] & ~np.uint32(7) or not np.isfinite(f[1:5]).all() or not f[5] >= 0 or w[7] != 0:
        return INVALID
    if w.view(np.int32)[6] != -1 and not has_labels:
        return INVALID
    return MISS


def keys(t, tmax, kind, index):
    """the keys of candidates t (float32 array), NO_KEY where one is not kept"""
    t = t + F(0.0)
    keep = (t >= 0) & (t <= tmax)
    k = (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(kind << 16) | np.asarray(index, np.uint64)
    return np.where(keep, k, NO_KEY)


def candidates(g, w, bounds, radius):
    """every key of one valid row, in slot order: particles, beams, walls (NO_KEY where there is no meeting)"""
    f = w.view(F)
    mask, skip = int(w[0]), int(w.view(np.int32)[6])
    ox, oy, dx, dy, tmax = f[1], f[2], f[3], f[4], f[5]
    out = []
    with np.errstate(all="ignore"):
        if mask & PARTICLES and g.pidx.size:
            r2 = F(radius) * F(radius)
            wx, wy = g.px - ox, g.py - oy
            a = dx * dx + dy * dy
            b = wx * dx + wy * dy
            c = (wx * wx + wy * wy) - r2
            q = b * b - a * c
            far = (b - np.sqrt(np.where(q >= 0, q, F(0.0)))) / a
            inside = c <= 0
            hit = inside | ((b > 0) & (q >= 0))
            k = keys(np.where(inside, F(0.0), far), tmax, PARTICLE, g.pidx)
            seen = hit & ~((skip != -1) & (g.plab == skip))
            out.append(np.where(seen, k, NO_KEY))
        if mask & BEAMS and g.bidx.size:
            ex, ey, wx, wy = g.bx - g.ax, g.by - g.ay, g.ax - ox, g.ay - oy
            den, tn, un = dx * ey - dy * ex, wx * ey - wy * ex, wx * dy - wy * dx
            neg = den < 0
            den, tn, un = np.where(neg, -den, den), np.where(neg, -tn, tn), np.where(neg, -un, un)
            hit = ~(den == 0) & (0 <= un) & (un <= den) & (0 <= tn)
            k = keys(tn / den, tmax, BEAM, g.bidx)
            seen = hit & ~((skip != -1) & (g.blab == skip))
            out.append(np.where(seen, k, NO_KEY))
        if mask & WALLS:
            ts, ws = [], []
            for o, d, lo, hi in ((ox, dx, WALL_LEFT, WALL_RIGHT), (oy, dy, WALL_LOW, WALL_HIGH)):
                if d < 0:
                    ts.append((F(0.0) - o) / d), ws.append(lo)
                if d > 0:
                    ts.append((F(bounds) - o) / d), ws.append(hi)
            if ts:
                out.append(keys(np.asarray(ts, F), tmax, WALL, np.asarray(ws)))
    return np.concatenate(out) if out else np.zeros(0, np.uint64)


def raycast_ref(buf, rows, bounds=1000.0, radius=10.0, labels=None, model="nearest", drop=(), ties=None):
    """(t as uint32 bits [k], hit int32 [k, 3], counts int32 [4]) of one scene.  rows: uint32 [k, 8].  ties: a list that gets, per
    valid row, the number of candidates that share the winner's t bits."""
    rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, ROW_WORDS)
    g = geometry(buf, labels, drop)
    lab = None if labels is None else np.asarray(labels, np.int64)
    t, hit, counts = np.zeros(len(rows), np.uint32), np.zeros((len(rows), HIT_WORDS), np.int32), np.zeros(COUNT_WORDS, np.int32)
    for j, w in enumerate(rows):
        v = verdict(w, labels is not None)
        if v != MISS:
            hit[j] = (v, -1, -1)
            continue
        counts[0] += 1
        k = candidates(g, w, bounds, radius)
        kept = k[k != NO_KEY]
        if kept.size == 0:
            t[j], hit[j] = w[5], (MISS, -1, -1)
            continue
        best = kept[0] if model == "first" else kept.min()
        if ties is not None:
            ties.append(int(((kept >> np.uint64(32)) == (best >> np.uint64(32))).sum()))
        kind, index = int(best >> np.uint64(16)) & 0xFFFF, int(best) & 0xFFFF
        label = -1
        if lab is not None and kind == PARTICLE:
            label = int(lab[index])
        elif lab is not None and kind == BEAM:
            label = int(lab[int(buf.beams["a"][index])])
        t[j], hit[j] = int(best >> np.uint64(32)), (kind, index, label)
        counts[kind] += 1
    return t, hit, counts


def raycast_of(bufs_now, rows, bounds=1000.0, radius=10.0, labels=None, **kw):
    """The three arrays of a batch, stacked (t as float32), from one Buffers per scene (None: never uploaded), rows uint32
    [N, k, 8] and labels int32 [N, max_particles] or None."""
    got = [raycast_ref(b, rows[i], bounds, radius, None if labels is None else labels[i], **kw) for i, b in enumerate(bufs_now)]
    return RayCast(np.stack([x[0] for x in got]).view(F), np.stack([x[1] for x in got]), np.stack([x[2] for x in got]))


def same(got, want):
    """the names of the arrays of two RayCasts that differ, by their bits"""
    bad = []
    for name, x, y in zip(RayCast._fields, got, want):
        if x is None:
            continue
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype == F:
            x, y = x.view(np.uint32), y.astype(F).view(np.uint32) if y.dtype != F else y.view(np.uint32)
        if x.shape != y.shape or not np.array_equal(x, y):
            bad.append(name)
    return bad


def bodies_labels(buf):
    """bodies()'s labels of one scene on the host: at a particle's data index the smallest data index of its body, -1 elsewhere"""
    maxP = buf.max_particles
    lab = np.full(maxP, -1, np.int32)
    pidx = buf.mapping[:buf.particle_count].astype(np.int64)
    lab[pidx] = pidx
    live = buf.mapping[maxP:maxP + buf.beam_count].astype(np.int64)
    a, b = buf.beams["a"][live].astype(np.int64), buf.beams["b"][live].astype(np.int64)
    changed = True
    while changed:
        m = np.minimum(lab[a], lab[b])
        changed = bool((lab[a] != m).any() or (lab[b] != m).any())
        np.minimum.at(lab, a, m)
        np.minimum.at(lab, b, m)
    return lab
