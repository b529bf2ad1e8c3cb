"""Scenes and programs of the tests of Engine.bodies() (sb_bodies_device), shared by tests/test_bodies_cpu.py (the
oracle side alone: what every case must show) and tests/test_gpu_bodies.py.

A case is tests/summary_cases.py's dict -- name, buf, bounds, mode, program, compare_after -- run with its apply_to_engine /
apply_to_oracle; the reference is tests/batch_bodies_ref.py's bodies_ref on what the oracle's load_buffers returns at each compare
point.  The graph scenes are built for the search itself: far more nodes than a workgroup holds, every mapping shuffled, uploaded
and not stepped."""
import numpy as np

import batch_bodies_ref as br
import summary_cases as sc
from batch_bodies_cases import path_edges

OFF = sc.OFF
ROW = 256   # particles per row of the serpentine the graph scenes lie on


def graph_scene(sb, cap, n, edges, seed, top=None):
    """batch_bodies_cases.graph_scene for any capacity, layout v2: n particles numbered 0 .. n-1 and one beam per entry of `edges`
    (pairs of particle numbers; repeats are parallel beams).  Particle k lives at data index D[k] in slot S[k], beam e at data
    index E[e] in slot T[e]: four independent random draws.  top: the particle number that gets the LARGEST data index.
    Particle NUMBER k sits at step k of a serpentine of spacing 30 (radius 10: nothing touches), so the beams of a path really
    are 30 long; every beam rests at the distance of its endpoints.  Returns (Buffers, D)."""
    maxP, maxB = cap
    m = len(edges)
    assert n <= maxP and m <= maxB
    rng = np.random.default_rng(seed)
    D, S = rng.permutation(maxP)[:n], rng.permutation(n)
    E, T = rng.permutation(maxB)[:m], rng.permutation(m)
    if top is not None:
        j = int(np.argmax(D))
        D[top], D[j] = D[j], D[top]
    k = np.arange(n)
    row, col = k // ROW, k % ROW
    col = np.where(row % 2 == 1, ROW - 1 - col, col)
    buf = sb.Buffers(2, maxP, maxB)
    buf.particles[D, 0] = (20.0 + 30.0 * col).astype("f4")
    buf.particles[D, 1] = (20.0 + 30.0 * row).astype("f4")
    buf.mapping[S] = D
    e = np.asarray(edges, dtype=np.int64).reshape(m, 2)
    a, b = D[e[:, 0]], D[e[:, 1]]
    dx, dy = buf.particles[b, 0] - buf.particles[a, 0], buf.particles[b, 1] - buf.particles[a, 1]
    dist = np.sqrt(dx * dx + dy * dy, dtype=np.float32)
    rec = buf.beams[E]
    rec["a"], rec["b"] = a, b
    for f in ("length", "target_length", "last_length"):
        rec[f] = dist
    for f, v in (("spring", 50.0), ("damp", 700.0), ("yield_strain", 0.2), ("strain_break_limit", 0.5)):
        rec[f] = v
    buf.beams[E] = rec
    buf.mapping[maxP + T] = E
    buf.particle_count, buf.beam_count = n, m
    return buf, D


def bounds_of(n):
    return float(max(1000, 40 + 30 * max(ROW, (n + ROW - 1) // ROW)))


N = 65536
PARALLEL_EDGES = [(0, 1), (1, 2), (5, 6), (4000, 3)]


def _path(sb):
    buf, D = graph_scene(sb, (70000, 70000), N, path_edges(N), seed=1)
    return buf, D, (1, N, 0, int(D.min()))


def _path4097(sb):
    buf, D = graph_scene(sb, (5000, 5000), 4097, path_edges(4097), seed=2)
    return buf, D, (1, 4097, 0, int(D.min()))


def _cycle(sb):
    buf, D = graph_scene(sb, (N, N), N, path_edges(N) + [(N - 1, 0)], seed=3)
    return buf, D, (1, N, 0, 0)


def _pieces(sb):
    buf, D = graph_scene(sb, (N, N), N, path_edges(N, 4096), seed=4)
    return buf, D, (16, 4096, 0, 0)      # 16 bodies of 4096: the tie goes to the smallest label, and every data index is in use


def _pairs(sb):
    buf, D = graph_scene(sb, (N, N), N, [(2 * k, 2 * k + 1) for k in range(N // 2)], seed=5)
    return buf, D, (N // 2, 2, 0, 0)


def _parallel(sb):
    n = 4097
    buf, D = graph_scene(sb, (5000, 70000), n, PARALLEL_EDGES * 16384, seed=6)
    lab3, lab2 = int(min(D[[0, 1, 2]])), int(min(D[[4000, 3]]))    # bodies {0, 1, 2}, {5, 6}, {4000, 3}; n - 7 single particles
    assert lab3 != lab2
    return buf, D, (n - 4, 3, n - 7, lab3)


def _star(sb):
    n = 2049
    buf, D = graph_scene(sb, (2100, 2100), n, [(n - 1, k) for k in range(n - 1)], seed=7, top=n - 1)
    assert D[n - 1] == D.max()
    return buf, D, (1, n, 0, int(D.min()))


GRAPHS = {"path 65536 in 70000": _path, "path 4097": _path4097, "cycle 65536": _cycle, "16 pieces of 4096": _pieces,
          "32768 pairs": _pairs, "4 edges x 16384": _parallel, "star 2049": _star}
_graph_cache = {}


def graph_case(sb, name):
    """The case of one graph (built once per process): uploaded, not stepped, compared as uploaded; `counts` is what the
    construction says the four words are, D the data index of every particle number."""
    if name not in _graph_cache:
        buf, D, counts = GRAPHS[name](sb)
        _graph_cache[name] = dict(name=name, buf=buf, D=D, counts=counts, bounds=bounds_of(buf.particle_count), mode=OFF, program=[],
                                  compare_after=[-1])
    return _graph_cache[name]


# ---------------------------------------------------------------- stepped cases (tests/summary_cases.py's)
def case_default(sb, mode=sc.ALLPAIRS):
    return sc.case_default(sb, mode)


def case_break(sb):
    """summary_cases.case_break as it stands.  On the oracle: after 40 substeps 12 flags are pending and the lattice is ONE body of
    385 live beams; the delete pass removes those 12 and it is STILL one body (of 373); the frame after leaves 3 bodies."""
    return sc.case_break(sb)


APART_STEPS = 100


def case_break_apart(sb):
    """The same lattice 100 substeps into the throw with no delete pass yet: 34 flags pending, ONE body; the delete pass alone
    leaves 4 bodies (141 particles, three single ones)."""
    return dict(sc.case_break(sb), name="breaking lattice, apart", program=[("step", APART_STEPS), ("delete",)], compare_after=[0, 1])


def case_capacity(sb):
    return sc.case_capacity(sb)


def without(buf, keep):
    """`buf` with only the beams keep[] of its beam slots, renumbered in order (what an editor's cut leaves)."""
    out = buf.copy()
    B, maxP = buf.beam_count, buf.max_particles
    recs = buf.beams[buf.mapping[maxP:maxP + B].astype(np.int64)][keep]
    n = len(recs)
    out.beams[:n] = recs
    out.mapping[maxP:maxP + n] = np.arange(n)
    out.beam_count = n
    return out


def cut_lattice(sb):
    """(whole, cut): a 24 x 12 lattice and the same scene without the beams that cross between its columns 11 and 12 -- an upload
    that only removes beams (less than an eighth of them), after which the lattice is two bodies of 144."""
    whole = sb.scenes.lattice_buffers(24, 12, d=30.0, origin=(100.0, 100.0), strain_limit=0.5, layout=2)
    B, maxP = whole.beam_count, whole.max_particles
    rec = whole.beams[whole.mapping[maxP:maxP + B].astype(np.int64)]
    left = whole.particles[:, 0] < np.float32(100.0 + 30.0 * 11.5)
    keep = left[rec["a"].astype(np.int64)] == left[rec["b"].astype(np.int64)]
    assert 0 < B - keep.sum() < B // 8
    return whole, without(whole, keep)


def stepped_cases(sb):
    return [case_default(sb), case_default(sb, OFF), case_break(sb), case_break_apart(sb), case_capacity(sb)]


# ---------------------------------------------------------------- the reference
def counts64(counts):
    return np.asarray(counts).astype(np.int64)


def expected_now(ref, case):
    """(labels, sizes, counts) of the oracle's state now; counts as the same four integers in int64"""
    labels, sizes, counts = br.bodies_ref(ref.load_buffers(case["buf"].copy()))
    return labels, sizes, counts64(counts)


def expected(orc, case):
    """{op index: (labels, sizes, counts)} (-1: as uploaded)."""
    ref, out = sc.make_oracle(orc, case), {}
    if -1 in case["compare_after"]:
        out[-1] = expected_now(ref, case)
    for k, op in enumerate(case["program"]):
        sc.apply_to_oracle(ref, op)
        if k in case["compare_after"]:
            out[k] = expected_now(ref, case)
    return out


_expected_cache = {}


def expected_cached(orc, case):
    """expected() once per process for the cases that several tests share (graphs, the stepped cases by name and mode); the arrays
    are not to be written to."""
    key = (case["name"], case["mode"])
    if key not in _expected_cache:
        out = expected(orc, case)
        for arrs in out.values():
            for a in arrs:
                a.setflags(write=False)
        _expected_cache[key] = out
    return _expected_cache[key]
