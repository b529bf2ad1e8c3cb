"""The cut predicate of include/softbody.h (sb_cut_device; csrc/sb_cut_math.h) restated in numpy float32 -- one rounding per
operator, in the order the header writes them -- and, for coordinates on which every float operation is exact, in Python fractions
from the geometry (closed segments meet; the distance from a point to a closed segment).  Scene helpers: the endpoints of a
Buffers' beams, the reference's hit bytes and counts."""
from fractions import Fraction

import numpy as np

NONE, SEGMENT, DISC = 0, 1, 2
F = np.float32


def _orient(ux, uy, vx, vy, wx, wy):
    return (vx - ux) * (wy - uy) - (vy - uy) * (wx - ux)


def _inbox(ux, uy, vx, vy, wx, wy):
    return (np.minimum(ux, vx) <= wx) & (wx <= np.maximum(ux, vx)) & (np.minimum(uy, vy) <= wy) & (wy <= np.maximum(uy, vy))


def segment_hits(px, py, qx, qy, A, B):
    ax, ay, bx, by = A[:, 0], A[:, 1], B[:, 0], B[:, 1]
    px, py, qx, qy = (np.full_like(ax, v) for v in (px, py, qx, qy))
    d1, d2 = _orient(px, py, qx, qy, ax, ay), _orient(px, py, qx, qy, bx, by)
    d3, d4 = _orient(ax, ay, bx, by, px, py), _orient(ax, ay, bx, by, qx, qy)
    proper = (((d1 > 0) & (d2 < 0)) | ((d1 < 0) & (d2 > 0))) & (((d3 > 0) & (d4 < 0)) | ((d3 < 0) & (d4 > 0)))
    return (proper | ((d1 == 0) & _inbox(px, py, qx, qy, ax, ay)) | ((d2 == 0) & _inbox(px, py, qx, qy, bx, by))
            | ((d3 == 0) & _inbox(ax, ay, bx, by, px, py)) | ((d4 == 0) & _inbox(ax, ay, bx, by, qx, qy)))


def disc_hits(cx, cy, r, A, B):
    ax, ay, bx, by = A[:, 0], A[:, 1], B[:, 0], B[:, 1]
    cx, cy, r = (np.full_like(ax, v) for v in (cx, cy, r))
    dx, dy, wx, wy = bx - ax, by - ay, cx - ax, cy - ay
    L2, t, r2 = dx * dx + dy * dy, wx * dx + wy * dy, r * r
    ux, uy = cx - bx, cy - by
    c = dx * wy - dy * wx
    near_a, near_b, side = wx * wx + wy * wy <= r2, ux * ux + uy * uy <= r2, c * c <= r2 * L2
    return (r >= 0) & np.where(~(t > 0), near_a, np.where(t >= L2, near_b, side))


def shape_words(shapes):
    """uint32 [n, 8] -> (kind uint32 [n], coordinates float32 [n, 4])"""
    w = np.ascontiguousarray(np.asarray(shapes).reshape(-1, 8)).view(np.uint32)
    return w[:, 0].copy(), w[:, 1:5].copy().view(np.float32)


def hits(shapes, A, B):
    """bool [m]: beam i (endpoints A[i], B[i], float32 [m, 2]) is hit by any of `shapes` (sb_cut_shape words, uint32 [n, 8])"""
    A, B = np.asarray(A, dtype=F).reshape(-1, 2), np.asarray(B, dtype=F).reshape(-1, 2)
    kind, xy = shape_words(shapes)
    out = np.zeros(len(A), dtype=bool)
    with np.errstate(all="ignore"):
        for k, (x0, y0, x1, y1) in zip(kind, xy):
            if k == SEGMENT:
                out |= segment_hits(x0, y0, x1, y1, A, B)
            elif k == DISC and y1 == 0:
                out |= disc_hits(x0, y0, x1, A, B)
    return out


# ---- the exact predicate, from the geometry

def exact_segment(P, Q, A, B):
    """closed segments PQ and AB share a point"""
    P, Q, A, B = ([Fraction(float(v)) for v in p] for p in (P, Q, A, B))

    def orient(u, v, w):
        return (v[0] - u[0]) * (w[1] - u[1]) - (v[1] - u[1]) * (w[0] - u[0])

    def on(u, v, w):  # w collinear with uv: inside its box
        return min(u[0], v[0]) <= w[0] <= max(u[0], v[0]) and min(u[1], v[1]) <= w[1] <= max(u[1], v[1])

    d1, d2, d3, d4 = orient(P, Q, A), orient(P, Q, B), orient(A, B, P), orient(A, B, Q)
    if d1 * d2 < 0 and d3 * d4 < 0:
        return True
    return (d1 == 0 and on(P, Q, A)) or (d2 == 0 and on(P, Q, B)) or (d3 == 0 and on(A, B, P)) or (d4 == 0 and on(A, B, Q))


def exact_disc(C, r, A, B):
    """the closed disc of radius r >= 0 around C touches the closed segment AB: the squared distance, with the one division"""
    C, A, B = ([Fraction(float(v)) for v in p] for p in (C, A, B))
    r = Fraction(float(r))
    if r < 0:
        return False
    d, w = (B[0] - A[0], B[1] - A[1]), (C[0] - A[0], C[1] - A[1])
    L2, t = d[0] * d[0] + d[1] * d[1], w[0] * d[0] + w[1] * d[1]
    if L2 == 0 or t <= 0:
        dist2 = w[0] * w[0] + w[1] * w[1]
    elif t >= L2:
        dist2 = (C[0] - B[0]) ** 2 + (C[1] - B[1]) ** 2
    else:
        s = t / L2
        fx, fy = A[0] + s * d[0], A[1] + s * d[1]
        dist2 = (C[0] - fx) ** 2 + (C[1] - fy) ** 2
    return dist2 <= r * r


def exact_hit(shape, A, B):
    """shape: (kind, x0, y0, x1, y1) of finite numbers"""
    k, x0, y0, x1, y1 = shape
    if k == SEGMENT:
        return exact_segment((x0, y0), (x1, y1), A, B)
    if k == DISC:
        return exact_disc((x0, y0), x1, A, B)
    return False


# ---- scenes

def pack(rows):
    """(kind, x0, y0, x1, y1) rows -> sb_cut_shape words, uint32 [n, 8]"""
    out = np.zeros((len(rows), 8), dtype=np.uint32)
    for i, (k, *xy) in enumerate(rows):
        out[i, 0] = int(k)
        out[i, 1:5] = np.asarray(xy, dtype=F).view(np.uint32)
    return out


def beam_ends(buf, particles=None):
    """(data index [B], A float32 [B, 2], B float32 [B, 2]) of the beam slots of `buf` (a layout.Buffers as loaded or uploaded),
    the positions from `particles` (records at particle data indices; None: buf's own)"""
    maxP, nb = buf.max_particles, buf.beam_count
    d = buf.mapping[maxP:maxP + nb].astype(np.int64)
    pos = (buf.particles if particles is None else particles)[:, :2].astype(F)
    rec = buf.beams[d]
    return d, pos[rec["a"].astype(np.int64)], pos[rec["b"].astype(np.int64)]


def scene_ref(buf, shapes, pending=None, dry=False):
    """(hit uint8 [max_beams], counts [tested, hit, flagged, already_flagged]) for the LIVE beams of `buf` (a read-back: its beam
    slots are the live ones); pending: bool [max_beams] by data index, the flags pending before the call"""
    d, A, B = beam_ends(buf)
    h = hits(shapes, A, B)
    out = np.zeros(buf.max_beams, dtype=np.uint8)
    out[d[h]] = 1
    already = int(pending[d[h]].sum()) if pending is not None else 0
    n_hit = int(h.sum())
    return out, [len(d), n_hit, 0 if dry else n_hit - already, already]
