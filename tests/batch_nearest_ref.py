"""The outputs of sb_batch_nearest_device (include/softbody.h) restated in numpy: the reference of
tests/test_gpu_batch_nearest*.py and, against csrc/sb_batch_near_math.h on the host, of tests/test_batch_nearest_cpu.py.

Everything is float32 with one rounding per operator, in the order the definition writes them: numpy's float32 +, -, *, / and sqrt
are correctly rounded, and no expression here is fused.  The geometry of a scene, the key (bits(d2) << 32) | (kind << 16) | index
whose minimum wins, the loop over the rows and the two WRONG models (`drop`, model="first") are tests/batch_query_ref.py's; this file
holds the row, the distances of a point, its `within` counts, its d word and its closest point."""
import collections

import numpy as np

import batch_query_ref as query
from batch_query_ref import (BEAM, BEAMS, COUNT_FIELDS, COUNT_WORDS, EMPTY, F, HIT_FIELDS, HIT_WORDS, INF, INVALID, MISS, NO_KEY,  # noqa: F401
                             PARTICLE, PARTICLES, ROW_WORDS, WALL, WALLS, WALL_HIGH, WALL_LEFT, WALL_LOW, WALL_RIGHT, bodies_labels,
                             geometry)

NEAR_MAX = query.ROWS_MAX
AT_A, AT_B, INSIDE = 0, 1, 2
WITHIN_FIELDS = ("particles", "beams")

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
    return query.row_verdict(w, has_labels, slice(1, 3), 3, 4, slice(5, 8))


def keys(d2, rmax2, kind, index):
    """the keys of squared distances d2 (float32 array), NO_KEY where one is not kept"""
    d2 = np.asarray(d2, F)
    return query.keys(d2, d2 <= rmax2, kind, index)


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
    n = len(rows)
    d, point, within = np.zeros(n, np.uint32), np.zeros((n, 2), np.uint32), np.zeros((n, 2), np.int32)
    pos = None if buf is None else buf.particles.astype(F)

    def kept(g, w, j):
        k, within[j, 0], within[j, 1] = candidates(g, w, bounds, branches)
        return k

    def answer(j, w, best, kind, index):
        if d2_bits is not None:
            d2_bits.append(0 if best is None else int(best >> np.uint64(32)))
        if best is None:
            if kind == MISS:
                d[j], point[j] = w[3], w[1:3]
            return
        px, py = w.view(F)[1], w.view(F)[2]
        with np.errstate(all="ignore"):
            if kind == PARTICLE:
                q = pos[index, :2]
            elif kind == BEAM:
                a, b = int(buf.beams["a"][index]), int(buf.beams["b"][index])
                qx, qy, _ = segment_q(*(np.asarray([x], F) for x in (pos[a, 0], pos[a, 1], pos[b, 0], pos[b, 1])), px, py)
                q = np.asarray([qx[0], qy[0]], F)
            else:
                q = np.asarray(wall_q(px, py, bounds)[index][:2], F)
            d[j] = np.sqrt(np.asarray([int(best >> np.uint64(32))], np.uint32).view(F))[0].view(np.uint32)
        point[j] = np.asarray(q, F).view(np.uint32)
    hit, counts = query.answers(buf, rows, labels, verdict, kept, answer, model, drop, ties)
    return d, hit, point, within, counts


def nearest_of(bufs_now, rows, bounds=1000.0, labels=None, **kw):
    """The five arrays of a batch, stacked (d and point as float32), from one Buffers per scene (None: never uploaded), rows uint32
    [N, k, 8] and labels int32 [N, max_particles] or None."""
    return query.stacked(Nearest, ("d", "point"), [nearest_ref(b, rows[i], bounds, None if labels is None else labels[i], **kw)
                                                  for i, b in enumerate(bufs_now)])


def same(got, want):
    """the names of the arrays of two Nearests that differ, by their bits"""
    return query.same(Nearest._fields, got, want)
