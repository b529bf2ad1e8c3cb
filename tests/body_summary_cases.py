"""Scenes and label sets of the tests of Engine.body_summary() (sb_body_summary_device), shared by
tests/test_body_summary_cpu.py (the reference alone: what every scene must show) and tests/test_gpu_body_summary.py.

The block sizes the scenes are cut for are the kernels': SORT_KEYS keys to a block of the radix sort (which sorts Wn member keys
and, with their number read on the device, the groups), SCAN_WORDS words to a block of the scans; the scan of the block sums
itself takes SCAN_SUMS_BLOCK sums an iteration, so its second iteration needs more than 2^20 data indices."""
import numpy as np

import batch_bodies_ref as br
import bodies_cases as bc
import summary_cases as sc
from batch_bodies_cases import path_edges

SORT_KEYS = 1024        # SBY_SORT
SCAN_WORDS = 1024       # SBY_SCAN
SCAN_SUMS_BLOCK = 256   # SBY_BLOCK
INT32_MIN = -2 ** 31


def with_velocities(buf, seed):
    """every particle a velocity of its own, magnitudes spread over forty binary orders (summary_cases.case_cut's): the double
    sums round, so the order of the additions shows"""
    rng = np.random.default_rng(seed)
    idx = buf.mapping[:buf.particle_count].astype(np.int64)
    n = len(idx)
    buf.particles[idx, 2:4] = ((rng.standard_normal((n, 2)) * 3.0 + (0.7, -1.3)) * np.exp2(-rng.integers(0, 40, (n, 2)))).astype("f4")
    return buf


def graph(sb, cap, n, edges, seed, **kw):
    buf, D = bc.graph_scene(sb, cap, n, edges, seed, **kw)
    return with_velocities(buf, seed + 100)


def singles(sb, n, cap=None, seed=21):
    """n free particles, each a group of its own under bodies' labels: n keys for the group sort"""
    return graph(sb, cap or (n + 7, 4), n, [], seed)


SMALL = {
    "path 8 in 8/8": lambda sb: graph(sb, (8, 8), 8, path_edges(8), 31),
    "two pairs in 65/64": lambda sb: graph(sb, (65, 64), 4, [(0, 1), (2, 3)], 32),
    "path 65 in 65/64": lambda sb: graph(sb, (65, 64), 65, path_edges(65), 33),
    "two particles": lambda sb: graph(sb, (2, 4), 2, [(0, 1)], 34),
    "no particles": lambda sb: sb.Buffers(2, 16, 16),
}

BIG = {
    "path 4097": lambda sb: graph(sb, (5000, 5000), 4097, path_edges(4097), 2),
    "16 pieces of 256": lambda sb: graph(sb, (4096, 4096), 4096, path_edges(4096, 256), 4),
    "512 pairs": lambda sb: graph(sb, (1024, 1024), 1024, [(2 * k, 2 * k + 1) for k in range(512)], 5),
    "star 1024": lambda sb: graph(sb, (1100, 1100), 1024, [(1023, k) for k in range(1023)], 7, top=1023),
    "shuffled 65536, many bodies": lambda sb: graph(sb, (bc.N, bc.N), bc.N, path_edges(bc.N, 3), 8),
}

# groups one less than, exactly, and one more than the keys of a sort block (= the words of a scan block)
EDGES = {"%d singles" % n: (lambda sb, n=n: singles(sb, n)) for n in (SORT_KEYS - 1, SORT_KEYS, SORT_KEYS + 1)}

_cache = {}


def scene(sb, name):
    """built once per process; not to be written to"""
    if name not in _cache:
        table = SMALL if name in SMALL else BIG if name in BIG else EDGES
        _cache[name] = table[name](sb)
    return _cache[name]


def body_labels(buf):
    return br.bodies_ref(buf)[0]


def sparse_in_big_capacity(sb, cap=1 << 20):
    """(wide, tight): a 32 x 31 lattice (992 particles) permuted behind an offset in capacity 2^20 -- the tables end near data
    index 1050, so ten of twenty levels run -- and the same records at capacity 1100 (W = 2048)"""
    lat = with_velocities(sb.scenes.lattice_buffers(32, 31, d=30.0, origin=(100.0, 100.0), strain_limit=0.5, layout=2), 9)
    nb = lat.beam_count
    return sc.permuted(sb, lat, cap, nb + 200, 50, 100), sc.permuted(sb, lat, 1100, nb + 200, 50, 100)


def caller_labels(buf, which):
    """label sets of the caller's own at data indices"""
    maxP = buf.max_particles
    d = np.arange(maxP, dtype=np.int64)
    if which == "stripes":          # five interleaved groups, labels far apart
        lab = (d % 5) * (maxP // 5)
    elif which == "outside":        # -1, max_particles and INT32_MIN put a particle into no group; the rest is one group
        lab = np.full(maxP, maxP - 1, np.int64)
        lab[d % 4 == 0], lab[d % 4 == 1], lab[d % 7 == 3] = -1, maxP, INT32_MIN
    elif which == "split":          # a connected body split into halves by data index: the beams between them belong to nobody
        lab = np.where(d < maxP // 2, 3, 0)
    else:
        raise ValueError(which)
    return lab.astype(np.int32)
