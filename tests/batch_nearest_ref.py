"""The outputs of sb_batch_nearest_device (include/softbody.h) restated in numpy: the reference of
tests/test_gpu_batch_nearest*.py and, against csrc/sb_batch_near_math.h on the host, of tests/test_batch_nearest_cpu.py.

Everything is float32 with one rounding per operator, in the order the definition writes them: numpy's float32 +, -, *, / and sqrt
are correctly rounded, and no expression here is fused.  The geometry of a scene is the ray cast's (batch_raycast_ref.geometry), on
what load_scene returns: the particle slots 0 .. particle_count-1 of the mapping at their records' positions, the beam slots
0 .. beam_count-1 whatever their break flags say (`drop`: data indices the caller wants left out -- the WRONG model that forgets
that a pending beam still counts).  The winner is the smallest 64-bit key (bits(d2) << 32) | (kind << 16) | index; model="first" is
the other WRONG model, which takes the first kept primitive in slot order (particles, beams, walls) instead of the nearest."""
import collections

import numpy as np

from batch_raycast_ref import bodies_labels, geometry  # noqa: F401  (the same geometry and labels as the ray cast's)

F = np.float32
ROW_WORDS, HIT_WORDS, COUNT_WORDS, NEAR_MAX = 8, 3, 4, 256
PARTICLES, BEAMS, WALLS = 1, 2, 4
MISS, PARTICLE, BEAM, WALL, EMPTY, INVALID = 0, 1, 2, 3, -1, -2
WALL_LEFT, WALL_RIGHT, WALL_LOW, WALL_HIGH = 1, 2, 4, 8
AT_A, AT_B, INSIDE = 0, 1, 2
HIT_FIELDS = ("kind", "index", "label")
WITHIN_FIELDS = ("particles", "beams")
COUNT_FIELDS = ("valid", "particles", "beams", "walls")
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
INF = float("inf")

Nearest = collections.namedtuple("Nearest", "d hit point within counts")


def pack(rows):
    """uint32 [k, 8] from tuples (mask, px, py, rmax[, skip_label[, reserved 0[, reserved 1[, reserved 2]]]])"""
    out = np.zeros((len(rows), ROW_WORDS), np.uint32)
    for i, r in enumerate(rows):
        r = tuple(r) + (-1, 0, 0, 0)[len(r) - 4:]
        out[i, 0] = r[0]
        out[i, 1:4] = np.asarray(r[1:4], F).view(np.uint32)
        out[i, 4] = np.int64(r[4]) & 0xFFFFFFFF
        out[i, 5:8] = r[5:8]
    return out


def verdict(w, has_labels):
    """MISS (the row is asked), EMPTY or INVALID, from the row's eight words"""
    w = np.asarray(w, np.uint32)
    if w[0] == 0:
        return EMPTY
    f = w.view(F)
    if w[0] & ~np.uint32(7) or not np.isfinite(f[1:3]).all() or not f[3] >= 0 or w[5:8].any():
        return INVALID
    if w.view(np.int32)[4] != -1 and not has_labels:
        return INVALID
    return MISS


def keys(d2, rmax2, kind, index):
    """the keys of squared distances d2 (float32 array), NO_KEY where one is not kept"""
    d2 = np.asarray(d2, F)
    k = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(kind << 16) | np.asarray(index, np.uint64)
    return np.where(d2 <= rmax2, k, NO_KEY)


def d2_to(qx, qy, px, py):
    vx, vy = qx - px, qy - py
    return vx * vx + vy * vy


def segment_q(ax, ay, bx, by, px, py):
    """(qx, qy, branch) of segments A -> B (float32 arrays) for one point: the clamped projection, the division only inside"""
    ex, ey, wx, wy = bx - ax, by - ay, px - ax, py - ay
    ee, we = ex * ex + ey * ey, wx * ex + wy * ey
    at_a = ~(we > 0)
    at_b = ~at_a & ~(we < ee)
    inside = ~at_a & ~at_b
    u = we / np.where(inside, ee, F(1.0))
    qx = np.where(at_a, ax, np.where(at_b, bx, ax + u * ex))
    qy = np.where(at_a, ay, np.where(at_b, by, ay + u * ey))
    return qx.astype(F), qy.astype(F), np.where(at_a, AT_A, np.where(at_b, AT_B, INSIDE))


def wall_q(px, py, bounds):
    """per wall word: (qx, qy, d2)"""
    b = F(bounds)
    out = {}
    for wall, q, v in ((WALL_LEFT, (F(0.0), py), F(0.0) - px), (WALL_RIGHT, (b, py), b - px), (WALL_LOW, (px, F(0.0)), F(0.0) - py),
                       (WALL_HIGH, (px, b), b - py)):
        out[wall] = (q[0], q[1], v * v)
    return out


def candidates(g, w, bounds, branches=None):
    """(every key of one valid row in slot order: particles, beams, walls -- NO_KEY where one is not kept or is skipped --, particles
    kept, beams kept).  branches: a set that gets the branch of every beam that is looked at."""
    f = w.view(F)
    mask, skip = int(w[0]), int(w.view(np.int32)[4])
    px, py, rmax = f[1], f[2], f[3]
    out, n_p, n_b = [], 0, 0
    with np.errstate(all="ignore"):
        rmax2 = rmax * rmax
        if mask & PARTICLES and g.pidx.size:
            k = keys(d2_to(g.px, g.py, px, py), rmax2, PARTICLE, g.pidx)
            k = np.where((skip != -1) & (g.plab == skip), NO_KEY, k)
            n_p = int((k != NO_KEY).sum())
            out.append(k)
        if mask & BEAMS and g.bidx.size:
            qx, qy, br = segment_q(g.ax, g.ay, g.bx, g.by, px, py)
            k = keys(d2_to(qx, qy, px, py), rmax2, BEAM, g.bidx)
            seen = ~((skip != -1) & (g.blab == skip))
            if branches is not None:
                branches |= set(br[seen].tolist())
            k = np.where(seen, k, NO_KEY)
            n_b = int((k != NO_KEY).sum())
            out.append(k)
        if mask & WALLS:
            q = wall_q(px, py, bounds)
            out.append(keys(np.asarray([q[wall][2] for wall in (1, 2, 4, 8)], F), rmax2, WALL, np.asarray([1, 2, 4, 8])))
    return (np.concatenate(out) if out else np.zeros(0, np.uint64)), n_p, n_b


def nearest_ref(buf, rows, bounds=1000.0, labels=None, model="nearest", drop=(), ties=None, branches=None, d2_bits=None):
    """(d as uint32 bits [k], hit int32 [k, 3], point as uint32 bits [k, 2], within int32 [k, 2], counts int32 [4]) of one scene.
    rows: uint32 [k, 8].  ties: a list that gets, per row with a winner, the number of kept primitives that share its d2 bits;
    d2_bits: a list that gets, per row, the winner's d2 bits (0 where there is none)."""
    rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, ROW_WORDS)
    g = geometry(buf, labels, drop)
    lab = None if labels is None else np.asarray(labels, np.int64)
    n = len(rows)
    d, hit, point = np.zeros(n, np.uint32), np.zeros((n, HIT_WORDS), np.int32), np.zeros((n, 2), np.uint32)
    within, counts = np.zeros((n, 2), np.int32), np.zeros(COUNT_WORDS, np.int32)
    pos = None if buf is None else buf.particles.astype(F)
    for j, w in enumerate(rows):
        v = verdict(w, labels is not None)
        if d2_bits is not None:
            d2_bits.append(0)
        if v != MISS:
            hit[j] = (v, -1, -1)
            continue
        counts[0] += 1
        k, within[j, 0], within[j, 1] = candidates(g, w, bounds, branches)
        kept = k[k != NO_KEY]
        if kept.size == 0:
            d[j], hit[j], point[j] = w[3], (MISS, -1, -1), w[1:3]
            continue
        best = kept[0] if model == "first" else kept.min()
        if ties is not None:
            ties.append(int(((kept >> np.uint64(32)) == (best >> np.uint64(32))).sum()))
        kind, index = int(best >> np.uint64(16)) & 0xFFFF, int(best) & 0xFFFF
        if d2_bits is not None:
            d2_bits[-1] = int(best >> np.uint64(32))
        px, py = w.view(F)[1], w.view(F)[2]
        label = -1
        with np.errstate(all="ignore"):
            if kind == PARTICLE:
                q = pos[index, :2]
                label = -1 if lab is None else int(lab[index])
            elif kind == BEAM:
                a, b = int(buf.beams["a"][index]), int(buf.beams["b"][index])
                qx, qy, _ = segment_q(*(np.asarray([x], F) for x in (pos[a, 0], pos[a, 1], pos[b, 0], pos[b, 1])), px, py)
                q = np.asarray([qx[0], qy[0]], F)
                label = -1 if lab is None else int(lab[a])
            else:
                q = np.asarray(wall_q(px, py, bounds)[index][:2], F)
            d[j] = np.sqrt(np.asarray([int(best >> np.uint64(32))], np.uint32).view(F))[0].view(np.uint32)
        hit[j], point[j] = (kind, index, label), np.asarray(q, F).view(np.uint32)
        counts[kind] += 1
    return d, hit, point, within, counts


def nearest_of(bufs_now, rows, bounds=1000.0, labels=None, **kw):
    """The five arrays of a batch, stacked (d and point as float32), from one Buffers per scene (None: never uploaded), rows uint32
    [N, k, 8] and labels int32 [N, max_particles] or None."""
    got = [nearest_ref(b, rows[i], bounds, None if labels is None else labels[i], **kw) for i, b in enumerate(bufs_now)]
    s = lambda i: np.stack([x[i] for x in got])
    return Nearest(s(0).view(F), s(1), s(2).view(F), s(3), s(4))


def same(got, want):
    """the names of the arrays of two Nearests that differ, by their bits"""
    bad = []
    for name, x, y in zip(Nearest._fields, got, want):
        if x is None:
            continue
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype == F:
            x, y = x.view(np.uint32), y.view(np.uint32)
        if x.shape != y.shape or not np.array_equal(x, y):
            bad.append(name)
    return bad
