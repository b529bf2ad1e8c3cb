"""Scenes, programs and label sets of the body-summary tests (sb_batch_body_summary_device).  The stepped cases are
those of tests/batch_summary_cases.py and tests/batch_bodies_cases.py (a case is tests/batch_cases.py's dict plus `compare_after`);
the graphs are tests/batch_bodies_cases.py's.  tests/test_batch_body_summary_cpu.py runs the oracle side alone and pins the
figures, tests/test_gpu_batch_body_summary.py runs both sides."""
import numpy as np

import batch_cases as bc
import batch_bodies_cases as cs
import batch_body_summary_ref as qr
import batch_summary_cases as sc

LATTICE = cs.LATTICE


# ---------------------------------------------------------------- stepped cases
def case_default_120_300(sb):
    """The default scene at capacity 120 / 300 (W = 128: leaves 120 .. 127 are never members) after 2 frames: 9 bodies."""
    c = sc.case_default_120_300(sb)
    c["program"], c["compare_after"] = [("frame", 2)], [0]
    return c


def case_break(sb):
    """The thrown lattices after 2 frames (1, 6, 21, 38, 56 and 1 bodies) and 5 substeps later, with flags pending."""
    return sc.case_break(sb)


def case_hetero(sb):
    """Capacity 1024 / 4096: in front of the delete pass the grabbed 12 x 12 lattice is one body with 129 flags pending; behind it
    it is 9 bodies and no flag is pending."""
    c = cs.case_hetero(sb)
    c["compare_after"] = c["compare_after"][1:]
    return c


def case_mapping(sb):
    return sc.case_mapping(sb)


def case_saturation(sb):
    """Capacity 8 / 8; scene NONFINITE_SCENE holds a NaN coordinate (data index 1) and an infinite velocity (data index 5)."""
    return sc.case_saturation(sb)


def stepped_cases(sb):
    return [case_default_120_300(sb), case_break(sb), case_hetero(sb), case_mapping(sb), case_saturation(sb)]


def expected(orc, case):
    """{op index: (bufs_now, body labels [n, maxP], pending slots per scene)} of the case on one oracle per scene, and the oracles
    at the end.  What body_summary_of needs; the rows themselves depend on max_rows and on the labels a test passes."""
    refs, out = sc.make_oracles(orc, case), {}
    maxP = case["cap"][0]
    for k, op in enumerate(case["program"]):
        bc.apply_to_oracles(refs, op)
        if k in case["compare_after"]:
            now = [None if r is None else r.load_buffers(b.copy()) for r, b in zip(refs, case["bufs"])]
            pending = [None if r is None else qr.pending_slots_of(r, b) for r, b in zip(refs, case["bufs"])]
            out[k] = (now, qr.body_labels_of(now, maxP), pending)
    return out, refs


# ---------------------------------------------------------------- graphs (no stepping: the positions alone make the sums)
def with_velocities(buf, seed):
    """The scene with random velocities at its particles' data indices, so that every sum has something to round."""
    buf = buf.copy()
    rng = np.random.default_rng(seed)
    d = buf.mapping[:buf.particle_count].astype(np.int64)
    buf.particles[d, 2:4] = rng.uniform(-50.0, 50.0, (len(d), 2)).astype(np.float32)
    return buf


def case_limit(sb):
    """One batch at 1024 / 4096: the shuffled path of 1024 (one group of all W leaves, the data indices permuted), 16 pieces of 64
    (a ranking tie that the label resolves), 512 pairs, a star, a scene of 2 particles, an empty and a never-uploaded scene."""
    g = cs.big_graphs(sb)
    order = ["path", "pieces", "pairs", "star", None]
    bufs = [bc.two_particles(sb, 2, cs.BIG, vx=4.0) if k is None else with_velocities(g[k][0], 11 + i) for i, k in enumerate(order)]
    bufs += [bc.empty_scene(sb, 2, cs.BIG), None]
    return dict(name="graphs at 1024 / 4096", layout=2, cap=cs.BIG, mode=bc.ALLPAIRS, bufs=bufs, program=[],
                groups=[1, 16, 512, 1, 1, 0, 0])


def case_small(sb, cap):
    """Capacity 8 / 8 (W = 8) or 65 / 64 (W = 128): the shuffled path filling the capacity, two pairs, an empty scene, the path."""
    n = cap[0]
    path, _ = cs.graph_scene(sb, cap, n, cs.path_edges(n), seed=7 + n)
    pairs, _ = cs.graph_scene(sb, cap, 4, [(0, 1), (2, 3)], seed=3)
    bufs = [with_velocities(path, 1), with_velocities(pairs, 2), bc.empty_scene(sb, 2, cap), with_velocities(path, 3)]
    return dict(name="path and two pairs at %d / %d" % cap, layout=2, cap=cap, mode=bc.ALLPAIRS, bufs=bufs, program=[],
                groups=[1, 2, 0, 1])


def graph_cases(sb):
    return [case_limit(sb), case_small(sb, (8, 8)), case_small(sb, (65, 64))]


# ---------------------------------------------------------------- labels of the caller's own
def caller_labels(n, maxP):
    """{name: labels [n, maxP] int32}: partitions that are no bodies, and values that name no group."""
    i = np.arange(maxP)
    split = np.where((i < maxP // 8) | (i >= maxP - maxP // 8), 5, 2)   # group 5 sits at both ends of the index range
    out = {"stripes": i % 3, "none": np.full(maxP, -1), "too large": np.full(maxP, maxP), "INT32_MIN": np.full(maxP, qr.INT32_MIN),
           "split": split, "mixed": np.where(i % 4 == 0, -1, np.where(i % 4 == 1, maxP, i % 2))}
    return {k: np.ascontiguousarray(np.broadcast_to(v.astype(np.int32), (n, maxP))) for k, v in out.items()}


def nonfinite_labels(n, maxP=8):
    """For case_saturation: everything in one group (the NaN and the infinity meet in it), and the two non-finite particles (data
    indices 1 and 5) in a group of their own."""
    one = np.zeros((n, maxP), np.int32)
    apart = np.zeros((n, maxP), np.int32)
    apart[:, [1, 5]] = 3
    return {"one group": one, "non-finite apart": apart}
