"""Scenes and programs of the bodies tests (sb_batch_bodies_device).  The stepped cases are
tests/batch_summary_cases.py's (a case is tests/batch_cases.py's dict plus `compare_after`: the indices of the program's ops after
which the bodies are compared); the graph scenes below are built for the component search and need no stepping.
tests/test_batch_bodies_cpu.py runs the oracle side alone and shows that the cases bite, tests/test_gpu_batch_bodies.py both sides."""
import numpy as np

import batch_cases as bc
import batch_summary_cases as sc
import batch_bodies_ref as br

LATTICE = 1   # case_hetero's 12 x 12 lattice


# ---------------------------------------------------------------- stepped cases
def case_break(sb):
    """The thrown lattices after 2 frames (removed beams, a compacted mapping with stale entries behind the live slots) and
    mid-frame (flags pending)."""
    return sc.case_break(sb)


def case_hetero(sb):
    """batch_summary_cases.case_hetero (capacity 1024 / 4096; an empty and a never-uploaded scene; after the grab and step(5) 129
    break flags are pending in the lattice and it is still ONE body of 144), then the delete pass that removes those beams.
    On the oracle that delete pass leaves the lattice in 9 bodies -- the largest of 110 particles, 3 single particles -- and the
    32 x 32 lattice beside it in 58 (967, 57 single): the plain grab of 500 is strong enough, no more substeps are needed."""
    c = sc.case_hetero(sb)
    n = len(c["program"])
    c["program"] = c["program"] + [("delete",)]
    c["compare_after"] = [c["compare_after"][0], n - 1, n]
    return c


def case_mapping(sb):
    return sc.case_mapping(sb)


def case_default(sb):
    """The default scene at capacity 128 / 320: 9 bodies before and after 3 frames."""
    return dict(name="default scene, 3 frames", layout=1, cap=(128, 320), mode=bc.ALLPAIRS,
                bufs=[sb.scenes.default_buffers(1, 128, 320)], program=[("frame", 3)], compare_after=[0])


def case_default_120_300(sb):
    return sc.case_default_120_300(sb)


def case_saturation(sb):
    return sc.case_saturation(sb)


def case_pile(sb):
    """256 free discs, max_beams = 0: 256 bodies of one particle each."""
    return sc.case_pile(sb)


def stepped_cases(sb):
    return [case_hetero(sb), case_break(sb), case_mapping(sb), case_default(sb), case_default_120_300(sb), case_saturation(sb),
            case_pile(sb)]


def expected_bodies(orc, case, before=False):
    """{op index: (labels, sizes, counts) of the batch} of the case on one oracle per scene (-1: before the program, with
    before=True), and the oracles at the end."""
    refs, out = sc.make_oracles(orc, case), {}
    maxP = case["cap"][0]

    def now():
        return br.bodies_of([None if r is None else r.load_buffers(b.copy()) for r, b in zip(refs, case["bufs"])], maxP)

    if before:
        out[-1] = now()
    for k, op in enumerate(case["program"]):
        bc.apply_to_oracles(refs, op)
        if k in case["compare_after"]:
            out[k] = now()
    return out, refs


# ---------------------------------------------------------------- graphs built for the algorithm
def graph_scene(sb, cap, n, edges, seed=None, top=None, layout=2):
    """n particles numbered 0 .. n-1 and one beam per entry of `edges` (pairs of particle numbers; repeats are parallel beams).
    seed=None: identity mappings.  Otherwise particle k lives at data index D[k] in slot S[k] and beam e at data index E[e] in
    slot T[e], with D, S, E, T independent random draws; top: the particle number that gets the LARGEST data index.
    Positions: data index d sits on a lattice of spacing 30 (radius 10: nothing touches).  Returns (Buffers, D)."""
    maxP, maxB = cap
    m = len(edges)
    assert n <= maxP and m <= maxB and maxP <= 1024
    if seed is None:
        D, S, E, T = np.arange(n), np.arange(n), np.arange(m), np.arange(m)
    else:
        rng = np.random.default_rng(seed)
        D, S = rng.permutation(maxP)[:n], rng.permutation(n)
        E, T = rng.permutation(maxB)[:m], rng.permutation(m)
    if top is not None:
        j = int(np.argmax(D))
        D[top], D[j] = D[j], D[top]
    buf = sb.Buffers(layout, maxP, maxB)
    buf.particles[D, 0] = 20.0 + 30.0 * (D % 32)
    buf.particles[D, 1] = 20.0 + 30.0 * (D // 32)
    buf.mapping[S] = D
    e = np.asarray(edges, dtype=np.int64).reshape(m, 2)
    rec = buf.beams[E]
    rec["a"], rec["b"] = D[e[:, 0]], D[e[:, 1]]
    for f, v in (("length", 30.0), ("target_length", 30.0), ("last_length", 30.0), ("spring", 50.0), ("damp", 700.0),
                 ("yield_strain", 0.2), ("strain_break_limit", 0.5)):
        rec[f] = v
    buf.beams[E] = rec
    buf.mapping[maxP + T] = E
    buf.particle_count, buf.beam_count = n, m
    return buf, D


def path_edges(n, leave_out_every=None):
    return [(k, k + 1) for k in range(n - 1) if not (leave_out_every and k % leave_out_every == leave_out_every - 1)]


BIG = (1024, 4096)
PARALLEL_EDGES = [(0, 1), (1, 2), (5, 6), (1000, 3)]


def big_graphs(sb):
    """{name: (Buffers, D, expected counts)} at capacity 1024 / 4096; every mapping shuffled."""
    n = 1024
    out = {}
    buf, D = graph_scene(sb, BIG, n, path_edges(n), seed=1)
    out["path"] = (buf, D, (1, n, 0, 0))                    # the deepest component the capacity allows
    buf, D = graph_scene(sb, BIG, n, path_edges(n) + [(n - 1, 0)], seed=2)
    out["cycle"] = (buf, D, (1, n, 0, 0))
    buf, D = graph_scene(sb, BIG, n, [(n - 1, k) for k in range(n - 1)], seed=3, top=n - 1)
    out["star"] = (buf, D, (1, n, 0, 0))                    # the hub at the largest data index
    buf, D = graph_scene(sb, BIG, n, path_edges(n, 64), seed=4)
    out["pieces"] = (buf, D, (16, 64, 0, 0))                # 16 bodies of 64: the tie goes to the smallest label, 0
    buf, D = graph_scene(sb, BIG, n, [(2 * k, 2 * k + 1) for k in range(n // 2)], seed=5)
    out["pairs"] = (buf, D, (512, 2, 0, 0))
    buf, D = graph_scene(sb, BIG, n, PARALLEL_EDGES * 1024, seed=6)
    lab3, lab4 = int(min(D[[0, 1, 2]])), int(min(D[[1000, 3]]))   # bodies {0, 1, 2}, {5, 6}, {1000, 3}; 1017 single particles
    assert lab3 != lab4
    out["parallel"] = (buf, D, (1020, 3, 1017, lab3))
    return out


def case_big_graphs(sb):
    """One batch: the path in three scenes, the other graphs and a two-particle scene between them."""
    g = big_graphs(sb)
    order = ["path", "cycle", "path", "star", "pieces", "pairs", "parallel", None, "path"]
    bufs = [bc.two_particles(sb, 2, BIG) if k is None else g[k][0] for k in order]
    counts = [(1, 2, 0, 0) if k is None else g[k][2] for k in order]
    return dict(name="graphs at 1024 / 4096", layout=2, cap=BIG, mode=bc.ALLPAIRS, bufs=bufs, program=[], counts=counts, order=order)


def case_small_path(sb, cap):
    """The shuffled path filling capacity 8 / 8 (7 beams) or 65 / 64 (one particle more than a wave), in three scenes beside an
    empty one."""
    n = cap[0]
    assert cap[1] >= n - 1
    buf, _ = graph_scene(sb, cap, n, path_edges(n), seed=7 + n)
    return dict(name="path at %d / %d" % cap, layout=2, cap=cap, mode=bc.ALLPAIRS, bufs=[buf, buf.copy(), bc.empty_scene(sb, 2, cap), buf.copy()],
                program=[], counts=[(1, n, 0, 0)] * 2 + [br.EMPTY_COUNTS] + [(1, n, 0, 0)])


def graph_cases(sb):
    return [case_big_graphs(sb), case_small_path(sb, (8, 8)), case_small_path(sb, (65, 64))]
