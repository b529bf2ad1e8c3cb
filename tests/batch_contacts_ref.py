"""The outputs of sb_batch_contacts_device (include/softbody.h) restated as a plain numpy float32 all-pairs test: the reference
of tests/test_gpu_batch_contacts.py and, alone, of tests/test_batch_contacts_cpu.py.  No grid.

Two distinct particles touch iff dist == 0 or dist < radius * 2, dist = sqrt(dx * dx + dy * dy), every operator in np.float32.
Everything is indexed by particle DATA index."""
import numpy as np

F = np.float32
WORDS = 4
LEFT, RIGHT, LOW, HIGH = 1, 2, 4, 8


def never_uploaded(max_particles, max_pairs=0, with_labels=False):
    """(touch, pairs, counts) of a scene never uploaded -- and of one without particles."""
    none = 0 if with_labels else -1
    touch = np.tile(np.array([0, none, 0, -1], np.int32), (max_particles, 1))
    return touch, np.full((max_pairs, 2), -1, np.int32), np.array([0, none, 0, 0], np.int32)


def touching(buf, radius):
    """(data index per slot, bool [P, P]: slot a touches slot b) of one scene."""
    P = buf.particle_count
    idx = buf.mapping[:P].astype(np.int64)
    x, y = buf.particles[idx, 0].astype(F), buf.particles[idx, 1].astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = x[None, :] - x[:, None], y[None, :] - y[:, None]          # [i, j]: xj - xi
        dist = np.sqrt(dx * dx + dy * dy)
        assert dist.dtype == F
        t = (dist == F(0.0)) | (dist < F(radius) * F(2.0))
    t[np.arange(P), np.arange(P)] = False
    return idx, t


def wall_bits(buf, radius, bounds):
    """(data index per slot, wall word per slot)."""
    P = buf.particle_count
    idx = buf.mapping[:P].astype(np.int64)
    x, y = buf.particles[idx, 0].astype(F), buf.particles[idx, 1].astype(F)
    lo, hi = F(radius), F(bounds) - F(radius)
    with np.errstate(invalid="ignore"):
        w = (x <= lo) * LEFT + (x >= hi) * RIGHT + (y <= lo) * LOW + (y >= hi) * HIGH
    return idx, w.astype(np.int32)


def contacts_ref(buf, radius=10.0, bounds=1000.0, labels=None, max_pairs=0, other_body=False):
    """(touch [maxP, 4], pairs [max_pairs, 2], counts [4]) int32 of one scene.  buf: a layout.Buffers as load_scene /
    OracleEngine.load_buffers return it (or as it was uploaded); labels: int32 [maxP] at data indices, or None."""
    maxP, P = buf.max_particles, buf.particle_count
    touch, pairs, counts = never_uploaded(maxP, max_pairs, labels is not None)
    if other_body and labels is None:
        raise ValueError("contacts_ref: other_body needs labels")
    if P == 0:
        return touch, pairs, counts
    idx, t = touching(buf, radius)
    _, wall = wall_bits(buf, radius, bounds)
    lab = np.zeros(P, np.int64) if labels is None else np.asarray(labels)[idx].astype(np.int64)
    differ = t & (lab[None, :] != lab[:, None])
    touch[idx, 0] = t.sum(axis=1)
    touch[idx, 1] = differ.sum(axis=1) if labels is not None else -1
    touch[idx, 2] = wall
    partner = np.where(t, idx[None, :], np.iinfo(np.int64).max).min(axis=1)
    touch[idx, 3] = np.where(t.any(axis=1), partner, -1)
    a, b = np.nonzero(t)
    keep = idx[a] < idx[b]
    every = sorted(zip(idx[a][keep].tolist(), idx[b][keep].tolist(), differ[a, b][keep].tolist()))
    listed = [(i, j) for i, j, d in every if d or not other_body][:max_pairs]
    if listed:
        pairs[:len(listed)] = np.array(listed, np.int32)
    counts[:] = (len(every), sum(1 for e in every if e[2]) if labels is not None else -1, int((wall != 0).sum()), int(t.any(axis=1).sum()))
    return touch, pairs, counts


def stack(results):
    return tuple(np.stack([r[k] for r in results]) for k in range(3))


def contacts_of(bufs_now, max_particles, radius=10.0, bounds=1000.0, labels=None, max_pairs=0, other_body=False):
    """The three arrays of a batch from one Buffers per scene (None: never uploaded); labels: int32 [n, maxP] or None."""
    out = []
    for i, b in enumerate(bufs_now):
        if b is None:
            out.append(never_uploaded(max_particles, max_pairs, labels is not None))
        else:
            out.append(contacts_ref(b, radius, bounds, None if labels is None else labels[i], max_pairs, other_body))
    return stack(out)


def all_pairs(buf, radius=10.0):
    """Every touching pair (i, j), i < j as data indices, ascending."""
    idx, t = touching(buf, radius)
    a, b = np.nonzero(t)
    return sorted((int(i), int(j)) for i, j in zip(idx[a], idx[b]) if i < j)
