"""The outputs of sb_raycast_device (include/softbody.h) restated in numpy: the brute-force definition with the WIDE
key (bits(t) << 32 | kind << 30 | index), and the rules behind the cost words -- the cells' rule, in-grid / short / long, the
walkable gate.  Geometry, verdicts and packing are tests/batch_raycast_ref.py's (the definition is the batch's, word for word); its
16-bit `keys` is not used.  Everything is float32 with one rounding per operator, in the order the header writes them."""
import collections

import numpy as np

import batch_raycast_ref as bref
from batch_raycast_ref import (BEAM, BEAMS, EMPTY, HIT_WORDS, INF, INVALID, MISS, PARTICLE, PARTICLES, ROW_WORDS, WALL, WALLS,  # noqa: F401
                               WALL_HIGH, WALL_LEFT, WALL_LOW, WALL_RIGHT, bodies_labels, geometry, pack, verdict)

F = np.float32
COUNT_WORDS = 8
COUNT_FIELDS = ("valid", "particles", "beams", "walls", "swept_rows", "particles_outside_grid", "long_beams", "reserved_7")
INDEX_BITS = 30
MAX_CELLS_PER_SIDE = 8192
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)

RayCast = collections.namedtuple("RayCast", "t hit counts")


def wide_keys(t, tmax, kind, index):
    """the wide keys of candidates t (float32 array), NO_KEY where one is not kept"""
    t = t + F(0.0)
    keep = (t >= 0) & (t <= tmax)
    k = (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(kind << INDEX_BITS) | np.asarray(index, np.uint64)
    return np.where(keep, k, NO_KEY)


def candidates(g, w, bounds, radius):
    """every wide key of one valid row: particles, beams, walls (NO_KEY where there is no meeting)"""
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
            k = wide_keys(np.where(inside, F(0.0), far), tmax, PARTICLE, g.pidx)
            out.append(np.where(hit & ~((skip != -1) & (g.plab == skip)), k, NO_KEY))
        if mask & BEAMS and g.bidx.size:
            ex, ey, wx, wy = g.bx - g.ax, g.by - g.ay, g.ax - ox, g.ay - oy
            den, tn, un = dx * ey - dy * ex, wx * ey - wy * ex, wx * dy - wy * dx
            neg = den < 0
            den, tn, un = np.where(neg, -den, den), np.where(neg, -tn, tn), np.where(neg, -un, un)
            hit = ~(den == 0) & (0 <= un) & (un <= den) & (0 <= tn)
            k = wide_keys(tn / den, tmax, BEAM, g.bidx)
            out.append(np.where(hit & ~((skip != -1) & (g.blab == skip)), k, NO_KEY))
        if mask & WALLS:
            ts, ws = [], []
            for o, d, lo, hi in ((ox, dx, WALL_LEFT, WALL_RIGHT), (oy, dy, WALL_LOW, WALL_HIGH)):
                if d < 0:
                    ts.append((F(0.0) - o) / d), ws.append(lo)
                if d > 0:
                    ts.append((F(bounds) - o) / d), ws.append(hi)
            if ts:
                out.append(wide_keys(np.asarray(ts, F), tmax, WALL, np.asarray(ws)))
    return np.concatenate(out) if out else np.zeros(0, np.uint64)


# ---- the rules behind the cost words

def default_cap(particles):
    """the largest G with G * G <= particles / 2, at least 1, at most 8192"""
    g = 1
    while (g + 1) * (g + 1) <= particles // 2 and g < MAX_CELLS_PER_SIDE:
        g += 1
    return g


def grid(particles, bounds, radius, cells_per_side=0):
    """(G, cell as float32): sb_batch_cell_geometry under the cap; one cell where radius or bounds are outside [2^-20, 2^30]"""
    bounds, radius = F(bounds), F(radius)
    cap = cells_per_side or default_cap(particles)
    lo, hi = F(2.0 ** -20), F(2.0 ** 30)
    cell_min = (radius * F(2.0)) * (F(1.0) + F(1.0) / F(64.0))
    if not (lo <= radius <= hi and lo <= bounds <= hi):
        return 1, bounds
    per_side = bounds / cell_min
    g = cap if per_side >= F(cap) else (int(per_side) if per_side >= 1 else 1)
    return g, max(cell_min, bounds / F(g))


def coord(x, cell, G):
    with np.errstate(all="ignore"):
        q = np.asarray(x, F) / F(cell)
        return np.where(~(q > 0), 0, np.where(q >= F(G), G - 1, np.minimum(q, F(G)).astype(np.int64))).astype(np.int64)


def in_grid(x, y, bounds):
    with np.errstate(all="ignore"):
        return np.isfinite(x) & np.isfinite(y) & (x >= 0) & (x <= F(bounds)) & (y >= 0) & (y <= F(bounds))


def leftovers(g, bounds, G, cell):
    """(particles outside the grid, long beams) of a Geometry"""
    outside = int((~in_grid(g.px, g.py, bounds)).sum())
    ends = in_grid(g.ax, g.ay, bounds) & in_grid(g.bx, g.by, bounds)
    span = (np.abs(coord(g.ax, cell, G) - coord(g.bx, cell, G)) <= 1) & (np.abs(coord(g.ay, cell, G) - coord(g.by, cell, G)) <= 1)
    return outside, int((~(ends & span)).sum())


def walkable(w, bounds):
    f = np.asarray(w, np.uint32).view(F)
    with np.errstate(all="ignore"):
        a = f[3] * f[3] + f[4] * f[4]
        lo, hi = -F(bounds), F(2.0) * F(bounds)
        return bool(lo <= f[1] <= hi and lo <= f[2] <= hi and F(2.0 ** -40) <= a <= F(2.0 ** 40))


def raycast_ref(buf, rows, bounds=1000.0, radius=10.0, labels=None, cells_per_side=0):
    """RayCast(t as uint32 bits [n], hit int32 [n, 3], counts int64 [8]) of one engine's scene.  rows: uint32 [n, 8]."""
    rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, ROW_WORDS)
    g = geometry(buf, labels)
    lab = None if labels is None else np.asarray(labels, np.int64)
    t, hit, counts = np.zeros(len(rows), np.uint32), np.zeros((len(rows), HIT_WORDS), np.int32), np.zeros(COUNT_WORDS, np.int64)
    for j, w in enumerate(rows):
        v = verdict(w, labels is not None)
        if v != MISS:
            hit[j] = (v, -1, -1)
            continue
        counts[0] += 1
        counts[4] += not walkable(w, bounds)
        k = candidates(g, w, bounds, radius)
        kept = k[k != NO_KEY]
        if kept.size == 0:
            t[j], hit[j] = w[5], (MISS, -1, -1)
            continue
        best = kept.min()
        kind, index = int(best >> np.uint64(INDEX_BITS)) & 3, int(best) & ((1 << INDEX_BITS) - 1)
        label = -1
        if lab is not None and kind == PARTICLE:
            label = int(lab[index])
        elif lab is not None and kind == BEAM:
            label = int(lab[int(buf.beams["a"][index])])
        t[j], hit[j] = int(best >> np.uint64(32)), (kind, index, label)
        counts[kind] += 1
    G, cell = grid(g.pidx.size, bounds, radius, cells_per_side)
    counts[5], counts[6] = leftovers(g, bounds, G, cell)
    return RayCast(t, hit, counts)


def same(got, want):
    """the names of the arrays of two RayCasts that differ, by their bits (t: float32 or its uint32 bits)"""
    bad = []
    for name, x, y in zip(RayCast._fields, got, want):
        if x is None:
            continue
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if name == "t":
            x, y = x.view(np.uint32), y.view(np.uint32)
        if x.shape != y.shape or not np.array_equal(x, y):
            bad.append(name)
    return bad
