"""The outputs of sb_batch_bodies_device (include/softbody.h) restated as a plain union-find: the reference of
tests/test_gpu_batch_bodies.py and, on the oracle alone, of tests/test_batch_bodies_cpu.py.

A body is a connected component of the scene's particles under its LIVE beams: the beam slots 0 .. beam_count-1 of the mapping,
whatever their break flags say.  Everything is indexed by particle DATA index."""
import numpy as np

WORDS = 4
EMPTY_COUNTS = (0, 0, 0, -1)


def never_uploaded(max_particles):
    """(labels, sizes, counts) of a scene never uploaded -- and of one without particles."""
    return (np.full(max_particles, -1, np.int32), np.zeros((max_particles, 2), np.int32), np.array(EMPTY_COUNTS, np.int32))


def bodies_ref(buf):
    """(labels [maxP], sizes [maxP, 2], counts [4]) int32 of one scene.  buf: a layout.Buffers as load_scene /
    OracleEngine.load_buffers return it (or as it was uploaded); None: never uploaded."""
    if buf is None:
        raise ValueError("bodies_ref: a never-uploaded scene has no buffers; use never_uploaded(max_particles)")
    maxP, P, B = buf.max_particles, buf.particle_count, buf.beam_count
    labels, sizes, counts = never_uploaded(maxP)
    pidx = [int(d) for d in buf.mapping[:P]]
    live = [int(d) for d in buf.mapping[maxP:maxP + B]]   # entries behind B are stale after a compaction: never edges
    parent = {d: d for d in pidx}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for d in live:
        a, b = find(int(buf.beams["a"][d])), find(int(buf.beams["b"][d]))
        if a != b:
            parent[max(a, b)] = min(a, b)     # the root is always the smallest data index of its tree
    for d in pidx:
        r = find(d)
        labels[d] = r
        sizes[r, 0] += 1
    for d in live:
        sizes[labels[int(buf.beams["a"][d])], 1] += 1
    roots = sorted(set(labels[pidx].tolist()))
    if roots:
        largest = max(roots, key=lambda r: (sizes[r, 0], -r))
        counts[:] = (len(roots), sizes[largest, 0], sum(1 for r in roots if sizes[r, 0] == 1), largest)
    return labels, sizes, counts


def stack(results):
    """[(labels, sizes, counts) per scene] -> (labels [n, maxP], sizes [n, maxP, 2], counts [n, 4])."""
    return tuple(np.stack([r[k] for r in results]) for k in range(3))


def bodies_of(bufs_now, max_particles):
    """The three arrays of a batch from one Buffers per scene (None: never uploaded)."""
    return stack([never_uploaded(max_particles) if b is None else bodies_ref(b) for b in bufs_now])


def brief(counts):
    """counts [n, 4] -> [(bodies, largest, singles) per scene], for assertions that read like the issue."""
    return [tuple(int(x) for x in row[:3]) for row in np.asarray(counts)]
