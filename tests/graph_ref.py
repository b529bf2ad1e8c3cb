"""The outputs of sb_batch_graph_device (include/softbody.h) restated in numpy, with sorts on integers only: the
reference of tests/test_gpu_batch_graph.py and, on hand-built graphs, of tests/test_graph_cpu.py.

The graph of a scene is defined on what load_scene returns: nodes are its particles at particle DATA indices, edges its LISTED
beams at beam DATA indices -- the beam slots 0 .. beam_count-1 of the mapping, whatever their break flags say (`drop`: data indices
the caller knows to carry a pending flag, for SKIP_PENDING).  A listed beam d with the record's pair (a, b) has the half-edges
(a, d, side 0) with neighbour b and (b, d, side 1) with neighbour a; nbr is the half-edges in ascending (particle, beam, side)."""
import collections

import numpy as np

COUNT_WORDS, MATERIAL_WORDS = 4, 5
MATERIAL_FIELDS = ("length", "spring", "damp", "yield_strain", "strain_break_limit")
EMPTY_COUNTS = (0, 0, 0, -1)

Graph = collections.namedtuple("Graph", "ends material row_ptr nbr counts")


def never_uploaded(max_particles, max_beams):
    """the five arrays of a scene never uploaded -- and of one without beams"""
    return Graph(np.full((max_beams, 2), -1, np.int32), np.zeros((max_beams, MATERIAL_WORDS), np.float32),
                 np.zeros(max_particles + 1, np.int32), np.full((2 * max_beams, 2), -1, np.int32), np.array(EMPTY_COUNTS, np.int32))


def graph_ref(buf, drop=()):
    """Graph(ends [maxB, 2], material [maxB, 5] float32, row_ptr [maxP + 1], nbr [2 maxB, 2], counts [4]) of one scene, int32
    unless said.  buf: a layout.Buffers as load_scene returns it (or as it was uploaded).  drop: beam data indices not to list."""
    maxP, maxB, B = buf.max_particles, buf.max_beams, buf.beam_count
    g = never_uploaded(maxP, maxB)
    live = np.asarray(buf.mapping[maxP:maxP + B], np.int64)   # entries behind B are stale after a compaction: never edges
    d = np.sort(live[~np.isin(live, np.asarray(list(drop), np.int64))])
    if d.size == 0:
        return g
    a, b = buf.beams["a"][d].astype(np.int64), buf.beams["b"][d].astype(np.int64)
    g.ends[d, 0], g.ends[d, 1] = a, b
    for q, name in enumerate(MATERIAL_FIELDS):
        g.material[d, q] = buf.beams[name][d]
    # half-edges (particle, beam, side, neighbour), sorted by the first three
    part = np.concatenate([a, b])
    beam = np.concatenate([d, d])
    side = np.concatenate([np.zeros_like(d), np.ones_like(d)])
    other = np.concatenate([b, a])
    order = np.lexsort((side, beam, part))
    n = order.size
    g.nbr[:n, 0], g.nbr[:n, 1] = other[order], beam[order]
    degree = np.bincount(part, minlength=maxP)[:maxP]
    g.row_ptr[1:] = np.cumsum(degree)
    top = int(degree.max())
    g.counts[:] = (d.size, int((degree > 0).sum()), top, int(np.flatnonzero(degree == top)[0]))
    return g


def graph_of(bufs_now, max_particles, max_beams, drop=None):
    """The five arrays of a batch, stacked, from one Buffers per scene (None: never uploaded).  drop: per scene, or None."""
    rows = [never_uploaded(max_particles, max_beams) if b is None else graph_ref(b, () if drop is None else drop[i])
            for i, b in enumerate(bufs_now)]
    return Graph(*(np.stack([r[k] for r in rows]) for k in range(5)))


def same(got, want):
    """the names of the arrays of two Graphs that differ, by their bits (material: as words)"""
    bad = []
    for name, x, y in zip(Graph._fields, got, want):
        if x is None:
            continue
        x, y = np.asarray(x), np.asarray(y)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), np.ascontiguousarray(y, np.float32).view(np.uint32)
        if x.shape != y.shape or not np.array_equal(x, y):
            bad.append(name)
    return bad
