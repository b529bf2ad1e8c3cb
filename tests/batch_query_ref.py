"""What the numpy restatements of the batch's queries share (tests/batch_raycast_ref.py, tests/batch_nearest_ref.py):
the words of a row and of a hit row, the geometry of a scene, bodies()'s labels on the host, the 64-bit key
(bits(float) << 32) | (kind << 16) | index, and the loop over a scene's rows -- verdict, candidates, winner, ties, label, counts --
around the query's own arithmetic.

The geometry of a scene is defined on what load_scene returns: the particle slots 0 .. particle_count-1 of the mapping at their
records' positions, the beam slots 0 .. beam_count-1 whatever their break flags say (`drop`: data indices the caller wants left out
-- the WRONG model that forgets that a pending beam still counts).  The winner is the smallest key; model="first" is the other WRONG
model, which takes the first kept candidate in slot order (particles, beams, walls) instead."""
import collections

import numpy as np

F = np.float32
ROW_WORDS, HIT_WORDS, COUNT_WORDS, ROWS_MAX = 8, 3, 4, 256
PARTICLES, BEAMS, WALLS = 1, 2, 4
MISS, PARTICLE, BEAM, WALL, EMPTY, INVALID = 0, 1, 2, 3, -1, -2
WALL_LEFT, WALL_RIGHT, WALL_LOW, WALL_HIGH = 1, 2, 4, 8
HIT_FIELDS = ("kind", "index", "label")
COUNT_FIELDS = ("valid", "particles", "beams", "walls")
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
INF = float("inf")

Geometry = collections.namedtuple("Geometry", "pidx px py plab bidx ax ay bx by blab")


def geometry(buf, labels=None, drop=()):
    """what a query can meet in one scene (None: never uploaded), in slot order; labels: int32 [max_particles] or None"""
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


def row_verdict(w, has_labels, finite, bound, skip, zero):
    """MISS (the row is asked), EMPTY or INVALID, from the row's eight words: those of the slice `finite` must be finite floats,
    word `bound` a float >= 0, those of the slice `zero` 0; word `skip` is the skip label, which only a call with labels may set"""
    w = np.asarray(w, np.uint32)
    if w[0] == 0:
        return EMPTY
    f = w.view(F)
    if w[0] & ~np.uint32(7) or not np.isfinite(f[finite]).all() or not f[bound] >= 0 or w[zero].any():
        return INVALID
    if w.view(np.int32)[skip] != -1 and not has_labels:
        return INVALID
    return MISS


def keys(f, keep, kind, index):
    """the keys of float32 candidates f (non-negative, never -0), NO_KEY where `keep` is False"""
    k = (f.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(kind << 16) | np.asarray(index, np.uint64)
    return np.where(keep, k, NO_KEY)


def answers(buf, rows, labels, verdict, candidates, answer, model="nearest", drop=(), ties=None):
    """(hit int32 [k, 3], counts int32 [4]) of one scene's rows (uint32 [k, 8]).  verdict(w, has_labels) and candidates(g, w, j) --
    every key of valid row j in slot order, NO_KEY where there is none -- are the query's; answer(j, w, best, kind, index) is
    called for every row with its winner's key (None: no winner) and lets the query fill its own outputs.  ties: a list that
    gets, per row with a winner, the number of candidates that share the winner's float bits."""
    g = geometry(buf, labels, drop)
    lab = None if labels is None else np.asarray(labels, np.int64)
    hit, counts = np.zeros((len(rows), HIT_WORDS), np.int32), np.zeros(COUNT_WORDS, np.int32)
    for j, w in enumerate(rows):
        best, kind, index, label = None, verdict(w, labels is not None), -1, -1
        if kind == MISS:
            counts[0] += 1
            k = candidates(g, w, j)
            kept = k[k != NO_KEY]
            if kept.size:
                best = kept[0] if model == "first" else kept.min()
                if ties is not None:
                    ties.append(int(((kept >> np.uint64(32)) == (best >> np.uint64(32))).sum()))
                kind, index = int(best >> np.uint64(16)) & 0xFFFF, int(best) & 0xFFFF
                if lab is not None and kind == PARTICLE:
                    label = int(lab[index])
                elif lab is not None and kind == BEAM:
                    label = int(lab[int(buf.beams["a"][index])])
                counts[kind] += 1
        hit[j] = (kind, index, label)
        answer(j, w, best, kind, index)
    return hit, counts


def stacked(result, floats, got):
    """the arrays of a batch, stacked into the named tuple `result` from one tuple of arrays per scene; those of the fields `floats`
    are uint32 bits and become float32"""
    s = lambda i: np.stack([x[i] for x in got])
    return result(*(s(i).view(F) if name in floats else s(i) for i, name in enumerate(result._fields)))


def same(fields, got, want):
    """the names among `fields` of the arrays of two results that differ, by their bits (None in got: not asked for)"""
    bad = []
    for name, x, y in zip(fields, got, want):
        if x is None:
            continue
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype == F:
            x, y = x.view(np.uint32), (y if y.dtype == F else y.astype(F)).view(np.uint32)
        if x.shape != y.shape or not np.array_equal(x, y):
            bad.append(name)
    return bad
