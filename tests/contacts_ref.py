"""The outputs of sb_contacts_device (include/softbody.h) restated in numpy float32: the definition of
tests/batch_contacts_ref.py's contacts_ref -- two distinct particles touch iff dist == 0 or dist < radius * 2, dist = sqrt(dx * dx +
dy * dy), every operator in np.float32, everything at particle DATA indices -- but row-chunked: no P x P array is ever held whole,
so a scene of 20 000 particles fits in memory.  No grid.  counts are int64, as sb_contacts' are.  tests/test_contacts_cpu.py
asserts that it equals batch_contacts_ref.contacts_ref on every scene of batch_contacts_cases.all_cases.

prune=True is for scenes of tens of thousands of particles: the rows are taken in the order of their x, and a chunk of rows meets
only the columns whose x lies within PRUNE_REACH of the chunk's own x-range.  A pair that is left out is farther than 2r * 1.01
apart in x alone, so its float32 dist is above 2r whatever y is (a part in a hundred against a rounding of a part in 2^23); a
coordinate that is not finite touches nothing and sorts behind everything.  Every pair that is kept goes through the same float32
expressions.  This knows nothing of the kernel's cells; tests/test_contacts_cpu.py asserts that it changes no output on any scene
of contacts_cases.BIG and batch_scenes."""
import numpy as np

import batch_contacts_ref as cr

F = np.float32
WORDS = 4
CHUNK = 512      # rows of the distance matrix held at a time
PRUNE_REACH = 1.01   # times 2r: how far in x beyond a chunk's x-range a column may still hold a partner (prune=True)


def contacts_ref(buf, radius=10.0, bounds=1000.0, labels=None, max_pairs=0, other_body=False, prune=False):
    """(touch int32 [maxP, 4], pairs int32 [max_pairs, 2], counts int64 [4]) of one scene.  buf: a layout.Buffers as
    load_buffers returns it (or as it was uploaded); labels: int32 [maxP] at data indices, or None; prune: see above."""
    maxP, P = buf.max_particles, buf.particle_count
    if other_body and labels is None:
        raise ValueError("contacts_ref: other_body needs labels")
    none = 0 if labels is not None else -1
    touch = np.tile(np.array([0, none, 0, -1], np.int32), (maxP, 1))
    pairs = np.full((max_pairs, 2), -1, np.int32)
    counts = np.array([0, none, 0, 0], np.int64)
    if P == 0:
        return touch, pairs, counts
    slots = buf.mapping[:P].astype(np.int64)
    _, wall = cr.wall_bits(buf, radius, bounds)
    two_r = F(radius) * F(2.0)
    idx = slots
    if prune:       # the rows by x; what is not finite behind everything (it touches nothing)
        xkey = buf.particles[slots, 0].astype(np.float64)
        xkey = np.where(np.isfinite(xkey), xkey, np.inf)
        by_x = np.argsort(xkey, kind="stable")
        idx, xkey = slots[by_x], xkey[by_x]
        reach = abs(float(two_r)) * PRUNE_REACH
    x, y = buf.particles[idx, 0].astype(F), buf.particles[idx, 1].astype(F)
    lab = np.zeros(P, np.int64) if labels is None else np.asarray(labels)[idx].astype(np.int64)
    big = np.iinfo(np.int64).max
    listed_i, listed_j, listed_d = [], [], []
    n_touching = 0
    for a0 in range(0, P, CHUNK):
        a1 = min(a0 + CHUNK, P)
        c0, c1 = 0, P       # the columns the chunk meets
        if prune:
            c0 = min(a0, int(np.searchsorted(xkey, xkey[a0] - reach, "left")))
            c1 = max(a1, int(np.searchsorted(xkey, xkey[a1 - 1] + reach, "right")))
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy = x[None, c0:c1] - x[a0:a1, None], y[None, c0:c1] - y[a0:a1, None]      # [i, j]: xj - xi
            dist = np.sqrt(dx * dx + dy * dy)
            assert dist.dtype == F
            t = (dist == F(0.0)) | (dist < two_r)
        t[np.arange(a1 - a0), np.arange(a0, a1) - c0] = False
        differ = t & (lab[None, c0:c1] != lab[a0:a1, None])
        rows = idx[a0:a1]
        touch[rows, 0] = t.sum(axis=1)
        touch[rows, 1] = differ.sum(axis=1) if labels is not None else -1
        partner = np.where(t, idx[None, c0:c1], big).min(axis=1)
        touch[rows, 3] = np.where(t.any(axis=1), partner, -1)
        n_touching += int(t.any(axis=1).sum())
        a, b = np.nonzero(t)
        i, j = rows[a], idx[c0 + b]
        keep = i < j
        listed_i.append(i[keep]), listed_j.append(j[keep]), listed_d.append(differ[a, b][keep])
    touch[slots, 2] = wall
    i, j, d = np.concatenate(listed_i), np.concatenate(listed_j), np.concatenate(listed_d)
    order = np.lexsort((j, i))
    i, j, d = i[order], j[order], d[order]
    counts[:] = (len(i), int(d.sum()) if labels is not None else -1, int((wall != 0).sum()), n_touching)
    if other_body:
        i, j = i[d], j[d]
    n = min(len(i), max_pairs)
    pairs[:n, 0], pairs[:n, 1] = i[:n], j[:n]
    return touch, pairs, counts
