"""The outputs of sb_batch_raycast_device (include/softbody.h) restated in numpy: the reference of
tests/test_gpu_batch_raycast*.py and, against csrc/sb_batch_ray_math.h on the host, of tests/test_batch_raycast_cpu.py.

Everything is float32 with one rounding per operator, in the order the definition writes them: numpy's float32 +, -, *, / and sqrt
are correctly rounded, and no expression here is fused.  The geometry of a scene, the key (bits(t) << 32) | (kind << 16) | index whose
minimum wins, the loop over the rows and the two WRONG models (`drop`, model="first") are tests/batch_query_ref.py's; this file holds
the row, the meetings of a ray and its t word."""
import collections

import numpy as np

import batch_query_ref as query
from batch_query_ref import (BEAM, BEAMS, COUNT_FIELDS, COUNT_WORDS, EMPTY, F, HIT_FIELDS, HIT_WORDS, INF, INVALID, MISS, NO_KEY,  # noqa: F401
                             PARTICLE, PARTICLES, ROW_WORDS, WALL, WALLS, WALL_HIGH, WALL_LEFT, WALL_LOW, WALL_RIGHT, Geometry,
                             bodies_labels, geometry)

RAY_MAX = query.ROWS_MAX

RayCast = collections.namedtuple("RayCast", "t hit counts")


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


def verdict(w, has_labels):
    """MISS (the row is cast), EMPTY or INVALID, from the row's eight words"""
    return query.row_verdict(w, has_labels, slice(1, 5), 5, 6, slice(7, 8))


def keys(t, tmax, kind, index):
    """the keys of candidates t (float32 array), NO_KEY where one is not kept"""
    t = t + F(0.0)
    return query.keys(t, (t >= 0) & (t <= tmax), kind, index)


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
    row with a hit, the number of candidates that share the winner's t bits."""
    rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, ROW_WORDS)
    t = np.zeros(len(rows), np.uint32)

    def answer(j, w, best, kind, index):
        if kind >= MISS:
            t[j] = w[5] if best is None else int(best >> np.uint64(32))
    hit, counts = query.answers(buf, rows, labels, verdict, lambda g, w, j: candidates(g, w, bounds, radius), answer, model, drop, ties)
    return t, hit, counts


def raycast_of(bufs_now, rows, bounds=1000.0, radius=10.0, labels=None, **kw):
    """The three arrays of a batch, stacked (t as float32), from one Buffers per scene (None: never uploaded), rows uint32
    [N, k, 8] and labels int32 [N, max_particles] or None."""
    return query.stacked(RayCast, ("t",), [raycast_ref(b, rows[i], bounds, radius, None if labels is None else labels[i], **kw)
                                          for i, b in enumerate(bufs_now)])


def same(got, want):
    """the names of the arrays of two RayCasts that differ, by their bits"""
    return query.same(RayCast._fields, got, want)
