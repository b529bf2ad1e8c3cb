"""The outputs of sb_nearest_device (include/softbody.h) restated in numpy: the brute-force definition with the WIDE
key (bits(d2) << 32 | kind << 30 | index), and the rules behind the cost words -- the ray casts' grid and leftovers
(tests/raycast_ref.py), the local gate, the ring in which a row's walk sees each record, the stop rule and so the rows the sweep
answers under a given max_rings.  Geometry, verdicts, distances and closest points are tests/batch_nearest_ref.py's (the definition
is the batch's, word for word); its 16-bit `keys` is not used.  Everything is float32 with one rounding per operator."""
import collections

import numpy as np

import batch_nearest_ref as bref
import raycast_ref as rref
from batch_nearest_ref import (BEAM, BEAMS, EMPTY, HIT_WORDS, INF, INVALID, MISS, PARTICLE, PARTICLES, ROW_WORDS, WALL, WALLS,  # noqa: F401
                               bodies_labels, geometry, pack, verdict)

F = np.float32
COUNT_WORDS = 8
COUNT_FIELDS = rref.COUNT_FIELDS
INDEX_BITS = 30
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
DEFAULT_RINGS, MAX_RINGS = 8, 8192

Nearest = collections.namedtuple("Nearest", "d hit point within counts")


def wide_keys(d2, rmax2, kind, index):
    """the wide keys of squared distances d2 (float32 array), NO_KEY where one is not kept"""
    d2 = np.asarray(d2, F)
    k = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(kind << INDEX_BITS) | np.asarray(index, np.uint64)
    return np.where(d2 <= rmax2, k, NO_KEY)


def candidates(g, w, bounds):
    """(particle keys, beam keys, wall keys) of one valid row, in slot order, NO_KEY where one is not kept, skipped or masked off"""
    f = w.view(F)
    mask, skip = int(w[0]), int(w.view(np.int32)[4])
    px, py, rmax = f[1], f[2], f[3]
    with np.errstate(all="ignore"):
        rmax2 = rmax * rmax
        kp = np.full(g.pidx.size, NO_KEY)
        if mask & PARTICLES and g.pidx.size:
            kp = np.where((skip != -1) & (g.plab == skip), NO_KEY, wide_keys(bref.d2_to(g.px, g.py, px, py), rmax2, PARTICLE, g.pidx))
        kb = np.full(g.bidx.size, NO_KEY)
        if mask & BEAMS and g.bidx.size:
            qx, qy, _ = bref.segment_q(g.ax, g.ay, g.bx, g.by, px, py)
            kb = np.where((skip != -1) & (g.blab == skip), NO_KEY, wide_keys(bref.d2_to(qx, qy, px, py), rmax2, BEAM, g.bidx))
        kw = np.zeros(0, np.uint64)
        if mask & WALLS:
            q = bref.wall_q(px, py, bounds)
            kw = wide_keys(np.asarray([q[wall][2] for wall in (1, 2, 4, 8)], F), rmax2, WALL, np.asarray([1, 2, 4, 8]))
    return kp, kb, kw


# ---- the rules behind the cost words

def local(w, bounds):
    f = np.asarray(w, np.uint32).view(F)
    lo, hi = -F(bounds), F(2.0) * F(bounds)
    return bool(lo <= f[1] <= hi and lo <= f[2] <= hi)


def record_cells(g, bounds, G, cell):
    """per particle and per beam (ix, iy) of the cell it is recorded in, (-1, -1) for the leftover list"""
    def cells(x0, y0, ok):
        return np.where(ok, x0, -1), np.where(ok, y0, -1)
    pin = rref.in_grid(g.px, g.py, bounds)
    p = cells(rref.coord(g.px, cell, G), rref.coord(g.py, cell, G), pin)
    xa, xb, ya, yb = (rref.coord(v, cell, G) for v in (g.ax, g.bx, g.ay, g.by))
    short = rref.in_grid(g.ax, g.ay, bounds) & rref.in_grid(g.bx, g.by, bounds) & (np.abs(xa - xb) <= 1) & (np.abs(ya - yb) <= 1)
    return p, cells(np.minimum(xa, xb), np.minimum(ya, yb), short)


def ring_of(k):
    """the ring in which a walk sees column (row) k of cells, relative to its virtual cell: the extra column towards lower x"""
    return np.where(k >= 0, k, -k - 1)


def bound2(h, cell, bounds):
    """L(h)^2 in binary64, -1 while there is no bound"""
    l = (float(h) * float(F(cell)) - 2.0 ** -20 * float(F(bounds))) * (1.0 - 2.0 ** -20)
    return l * l if l > 0.0 else -1.0


def rings_needed(w, keys, wall_key, rec_cells, bounds, G, cell, within, max_rings=MAX_RINGS):
    """the rings a LOCAL row's walk takes before it is complete, or None where it is not complete after max_rings.  keys: per record
    its key; rec_cells: (ix, iy) per record, -1 for leftovers."""
    mask = int(w[0])
    if not mask & (PARTICLES | BEAMS):
        return 0
    if G == 1:
        return 1
    f = np.asarray(w, np.uint32).view(F)
    cx, cy = (int(np.floor(float(v) / float(F(cell)))) for v in (f[1], f[2]))
    nearest = lambda c: 0 if 0 <= c < G else int(min(ring_of(np.int64(0 - c)), ring_of(np.int64(G - 1 - c))))
    h0 = max(nearest(cx), nearest(cy))
    cover = int(max(ring_of(np.int64(0 - cx)), ring_of(np.int64(G - 1 - cx)), ring_of(np.int64(0 - cy)), ring_of(np.int64(G - 1 - cy))))
    ix, iy = rec_cells
    ring = np.where(ix >= 0, np.maximum(ring_of(ix - cx), ring_of(iy - cy)), np.iinfo(np.int64).max)
    with np.errstate(all="ignore"):
        rmax2 = float(f[3] * f[3])
    for taken, h in enumerate(range(h0, h0 + max_rings), 1):
        if h >= cover:
            return taken
        l2 = bound2(h, cell, bounds)
        if rmax2 < l2:
            return taken
        if not within:
            seen = keys[ring <= h]
            best = min([wall_key] + ([seen.min()] if seen.size else []))
            if best != NO_KEY and float(np.asarray([int(best) >> 32], np.uint32).view(F)[0]) < l2:
                return taken
    return None


def nearest_ref(buf, rows, bounds=1000.0, radius=10.0, labels=None, cells_per_side=0, max_rings=0, within=True, rings=None, swept=None):
    """Nearest(d as uint32 bits [n], hit int32 [n, 3], point as uint32 bits [n, 2], within int32 [n, 2], counts int64 [8]) of one
    engine's scene.  rows: uint32 [n, 8].  within: whether the call asks for it (word 4 depends on it).  rings: a list that gets, per
    valid local row, the rings its walk takes (None: the sweep answers it); swept: a list that gets, per row, whether the sweep answers it."""
    rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, ROW_WORDS)
    n = len(rows)
    g = geometry(buf, labels)
    lab = None if labels is None else np.asarray(labels, np.int64)
    pos = buf.particles.astype(F)
    d, hit, point = np.zeros(n, np.uint32), np.zeros((n, HIT_WORDS), np.int32), np.zeros((n, 2), np.uint32)
    inside, counts = np.zeros((n, 2), np.int32), np.zeros(COUNT_WORDS, np.int64)
    G, cell = rref.grid(g.pidx.size, bounds, radius, cells_per_side)
    pc, bc = record_cells(g, bounds, G, cell)
    rec_cells = (np.concatenate([pc[0], bc[0]]), np.concatenate([pc[1], bc[1]]))
    for j, w in enumerate(rows):
        v = verdict(w, labels is not None)
        before = counts[4]
        if swept is not None:
            swept.append(False)
        if v != MISS:
            hit[j] = (v, -1, -1)
            continue
        counts[0] += 1
        kp, kb, kw = candidates(g, w, bounds)
        inside[j] = ((kp != NO_KEY).sum(), (kb != NO_KEY).sum())
        wall_key = kw.min() if kw.size else NO_KEY
        if not local(w, bounds):
            counts[4] += 1
        else:
            took = rings_needed(w, np.concatenate([kp, kb]), wall_key, rec_cells, bounds, G, cell, within, max_rings or DEFAULT_RINGS)
            counts[4] += took is None
            if rings is not None:
                rings.append(took)
        if swept is not None:
            swept[-1] = bool(counts[4] > before)
        k = np.concatenate([kp, kb, kw])
        kept = k[k != NO_KEY]
        if kept.size == 0:
            d[j], hit[j], point[j] = w[3], (MISS, -1, -1), w[1:3]
            continue
        best = kept.min()
        kind, index = int(best >> np.uint64(INDEX_BITS)) & 3, int(best) & ((1 << INDEX_BITS) - 1)
        label = -1
        px, py = w.view(F)[1], w.view(F)[2]
        with np.errstate(all="ignore"):
            if kind == PARTICLE:
                q = pos[index, :2]
                label = -1 if lab is None else int(lab[index])
            elif kind == BEAM:
                a, b = int(buf.beams["a"][index]), int(buf.beams["b"][index])
                qx, qy, _ = bref.segment_q(*(np.asarray([x], F) for x in (pos[a, 0], pos[a, 1], pos[b, 0], pos[b, 1])), px, py)
                q = np.asarray([qx[0], qy[0]], F)
                label = -1 if lab is None else int(lab[a])
            else:
                q = np.asarray(bref.wall_q(px, py, bounds)[index][:2], F)
            d[j] = np.sqrt(np.asarray([int(best >> np.uint64(32))], np.uint32).view(F))[0].view(np.uint32)
        hit[j], point[j] = (kind, index, label), np.asarray(q, F).view(np.uint32)
        counts[kind] += 1
    counts[5], counts[6] = rref.leftovers(g, bounds, G, cell)
    return Nearest(d, hit, point, inside, counts)


def same(got, want, skip=()):
    """the names of the arrays of two Nearests that differ, by their bits (None in got, or a name in skip: not compared)"""
    bad = []
    for name, x, y in zip(Nearest._fields, got, want):
        if x is None or name in skip:
            continue
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.shape != y.shape or x.itemsize != y.itemsize or x.tobytes() != y.tobytes():
            bad.append(name)
    return bad
