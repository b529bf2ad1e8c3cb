"""The scenes and points of tests/test_batch_nearest_cpu.py and tests/test_gpu_batch_nearest.py (BatchEngine.nearest):
twelve small scenes of one capacity, each with its own K rows.  Five are built by hand on integer coordinates, where every answer
is known exactly (`expect`: row -> (d, kind, index, qx, qy) for a call without labels, `expect_labelled` for one with the scene's
labels; `expect_within`: row -> (particles, beams), the same in both); the others are seeded draws.  Every scene carries `labels`
(bodies()'s labels of it, computed on the host) and `pending` (beam data indices a test may treat as carrying a pending break
flag).  coverage() states what the set must exercise."""
import numpy as np

import batch_nearest_ref as ref
import batch_raycast_cases as ray_cases
from batch_raycast_cases import hand_scene
from graph_cases import scene as graph_scene

F = np.float32
INF = ref.INF
CAP = ray_cases.CAP
LAYOUT = ray_cases.LAYOUT
K = 24
BOUNDS = 1000.0
ALL, P_, B_, W_ = 7, ref.PARTICLES, ref.BEAMS, ref.WALLS
BELOW_3 = float(np.nextafter(F(3.0), F(0.0)))


def segments(sb):
    """slots 0, 1: the segment (0, 0) -> (4, 0), beam 0; slots 2, 3 both at (20, 20): a degenerate beam 1; slot 4 alone at (40, 0)"""
    buf = hand_scene(sb, [(0, 0), (4, 0), (20, 20), (20, 20), (40, 0)], [(0, 1), (2, 3)])
    rows = [(B_, 1, 3, INF),                  # 0 inside: u = 0.25, Q = (1, 0), d2 = 9
            (B_, -2, 0, INF),                 # 1 before A: clamped to (0, 0)
            (B_, 7, 4, INF),                  # 2 past B: clamped to (4, 0), d2 = 9 + 16
            (ALL, 40, 0, INF),                # 3 on a particle: d = +0
            (B_, 20, 23, INF),                # 4 the degenerate beam answers as its endpoint A
            (B_, 1, 3, 3),                    # 5 rmax = 3 keeps d2 = 9 ...
            (B_, 1, 3, BELOW_3),              # 6 ... the float below 3 does not: a miss that returns rmax's bits
            (P_, 40, 0, 0),                   # 7 rmax = 0 on a particle: kept
            (P_, 40, 1, 0),                   # 8 rmax = 0 beside it: a miss
            (P_ | B_, 4, 0, INF),             # 9 on endpoint B: particle 1 and beam 0 both at d2 = 0: the particle
            (W_, 3, 500, INF),                # 10 .. 13 each wall
            (W_, 990, 500, INF),
            (W_, 500, 6, INF),
            (W_, 500, 995, INF),
            (ALL, 2, 1, 1.5)]                 # 14 beam 0 at d = 1 before the low wall at 1; particles out of reach
    expect = {0: (3, 2, 0, 1, 0), 1: (2, 2, 0, 0, 0), 2: (5, 2, 0, 4, 0), 3: (0, 1, 4, 40, 0), 4: (3, 2, 1, 20, 20), 5: (3, 2, 0, 1, 0),
              6: (BELOW_3, 0, -1, 1, 3), 7: (0, 1, 4, 40, 0), 8: (0, 0, -1, 40, 1), 9: (0, 1, 1, 4, 0), 10: (3, 3, 1, 0, 500),
              11: (10, 3, 2, 1000, 500), 12: (6, 3, 4, 500, 0), 13: (5, 3, 8, 500, 1000), 14: (1, 2, 0, 2, 0)}
    within = {0: (0, 2), 3: (5, 2), 5: (0, 1), 6: (0, 0), 7: (1, 0), 8: (0, 0), 9: (5, 2), 10: (0, 0), 14: (0, 1)}
    return dict(name="segments", buf=buf, rows=rows, expect=expect, expect_labelled=expect, expect_within=within)


def ties(sb):
    """slots 0, 1 at data indices 5, 2: two particles mirrored about the probe; slots 2, 3 (data 9, 7): a beam, data index 3, along
    x = 300"""
    buf = hand_scene(sb, [(100, 56), (100, 44), (300, 300), (300, 400)], [(2, 3)], pmap=[5, 2, 9, 7], bmap=[3])
    rows = [(ALL, 100, 50, INF),              # 0 both particles at d2 = 36: the smaller DATA index (slot 1's) wins
            (ALL, 300, 290, INF),             # 1 the beam clamps to its endpoint A, particle 9: the particle wins
            (B_ | W_, 300, 290, INF),         # 2 without particles the beam does
            (B_ | W_, 150, 350, INF),         # 3 the beam and the left wall both at d2 = 22500: the beam
            (ALL, 300, 290, INF, 7),          # 4 body {7, 9} skipped: the low wall at 290
            (ALL, 100, 50, INF, 2),           # 5 particle 2 skipped: its mirror image
            (W_, 5, 5, INF),                  # 6 the left and the low wall both at 5: the smaller wall word
            (P_ | B_, 300, 410, 10)]          # 7 clamped to endpoint B, particle 7
    lab = ref.bodies_labels(buf)
    assert lab[[2, 5, 7, 9]].tolist() == [2, 5, 7, 7]
    expect = {0: (6, 1, 2, 100, 44), 1: (10, 1, 9, 300, 300), 2: (10, 2, 3, 300, 300), 3: (150, 2, 3, 300, 350), 4: (0, -2, -1, 0, 0),
              5: (0, -2, -1, 0, 0), 6: (5, 3, 1, 0, 5), 7: (10, 1, 7, 300, 400)}
    return dict(name="ties", buf=buf, rows=rows, expect=expect,
                expect_labelled={**expect, 4: (290, 3, 4, 300, 0), 5: (6, 1, 5, 100, 56)}, expect_within={0: (4, 1), 7: (1, 1)})


def row_codes(sb):
    nan = float("nan")
    buf = hand_scene(sb, [(100, 50), (200, 50)], [(0, 1)])
    rows = [(0, 100, 60, INF),                # 0 empty
            (8, 100, 60, INF),                # 1 .. 2 an unknown mask bit
            (0x80000001, 100, 60, INF),
            (ALL, INF, 60, INF),              # 3 .. 4 a point that is not finite
            (ALL, 100, nan, INF),
            (ALL, 100, 60, -1),               # 5 .. 6 rmax not >= 0
            (ALL, 100, 60, nan),
            (ALL, 100, 60, INF, -1, 1),       # 7 .. 9 each reserved word
            (ALL, 100, 60, INF, -1, 0, 1),
            (ALL, 100, 60, INF, -1, 0, 0, 0x80000000),
            (ALL, 100, 60, INF, 0),           # 10 a skip_label: invalid without labels; with them it skips body 0, everything but the walls
            (ALL, 100, 50, -0.0),             # 11 rmax = -0 is >= 0: valid, and only d2 = 0 fits
            (0, nan, INF, nan, 5, 9, 9, 9),   # 12 mask 0 is empty whatever else the row holds
            (ALL, 100, 60, INF),              # 13 valid: particle 0 at 10
            (P_ | B_, 150, 80, 20)]           # 14 a miss: the beam is 30 away
    expect = {0: (0, -1, -1, 0, 0), 12: (0, -1, -1, 0, 0), 11: (0, 1, 0, 100, 50), 13: (10, 1, 0, 100, 50), 10: (0, -2, -1, 0, 0),
              14: (20, 0, -1, 150, 80)}
    expect.update({j: (0, -2, -1, 0, 0) for j in range(1, 10)})
    return dict(name="row codes", buf=buf, rows=rows, expect=expect, expect_labelled={**expect, 10: (60, 3, 4, 100, 0)},
                expect_within={0: (0, 0), 5: (0, 0), 13: (2, 1), 14: (0, 0)})


def non_finite(sb):
    """slot 0 at (NaN, 5), slot 1 at (inf, 7), slot 2 at (30, 40): three bodies of one particle"""
    buf = hand_scene(sb, [(0, 5), (0, 7), (30, 40)], [])
    buf.particles[0, 0], buf.particles[1, 0] = np.nan, np.inf
    rows = [(P_, 0, 0, INF),                  # 0 the finite particle at 50; within counts the infinite one too, never the NaN
            (P_, 0, 0, 1.0e6),                # 1 a finite reach: the infinite one is out
            (P_, 0, 0, INF, 2),               # 2 (with labels) the finite one skipped: the infinite one, at +inf
            (P_, 0, 0, 40),                   # 3 nothing within 40: a miss
            (P_, 0, 0, 1.0e6, 2)]             # 4 (with labels) the finite one skipped under a finite reach: a miss, the NaN is never kept
    expect = {0: (50, 1, 2, 30, 40), 1: (50, 1, 2, 30, 40), 2: (0, -2, -1, 0, 0), 3: (40, 0, -1, 0, 0), 4: (0, -2, -1, 0, 0)}
    return dict(name="non-finite positions", buf=buf, rows=rows, expect=expect,
                expect_labelled={**expect, 2: (INF, 1, 1, INF, 7), 4: (1.0e6, 0, -1, 0, 0)},
                expect_within={0: (2, 0), 1: (1, 0), 3: (0, 0)}, expect_within_labelled={2: (1, 0), 4: (0, 0)})


def masks_and_within(sb):
    """a 3 x 3 lattice of spacing 10 at (100, 100) with its 20 beams, and a lone particle at (200, 100)"""
    p, b = sb.scenes.rectangle(100.0, 100.0, 10.0, 3, 3, 50.0, 700.0, 0.2, 1.0e9, layout=LAYOUT)
    buf = sb.Buffers(LAYOUT, *CAP)
    buf.set_scene(p, b)
    buf.particles[buf.particle_count, :2] = (200.0, 100.0)
    buf.mapping[buf.particle_count] = buf.particle_count
    buf.particle_count += 1
    rows = [(m, 110, 110, r) for r in (INF, 10.0, 0.0) for m in (ALL, P_ | B_, P_ | W_, B_ | W_, P_, B_, W_)]
    rows += [(ALL, 110, 110, INF, 0), (ALL, 110, 110, INF, 9), (ALL, 110, 110, 95.0)]   # bodies 0 (the lattice) and 9 (the lone one) skipped
    return dict(name="masks and within", buf=buf, rows=rows, expect={}, expect_labelled={},
                expect_within={0: (10, 20), 4: (10, 0), 5: (0, 20), 6: (0, 0), 7: (5, 20), 14: (1, 8), 23: (10, 20)},
                expect_within_labelled={21: (1, 0), 22: (9, 20)})


def drawn_rows(buf, rng, labels, outside=False, short=False):
    """K rows of a seeded draw over a scene: a third on or near a particle or a live beam, the rest anywhere"""
    maxP = buf.max_particles
    pidx = buf.mapping[:buf.particle_count].astype(np.int64)
    live = buf.mapping[maxP:maxP + buf.beam_count].astype(np.int64)
    rows = []
    for j in range(K):
        o = rng.uniform(-300.0, 1300.0, 2) if outside else rng.uniform(0.0, 1000.0, 2)
        if j % 3 == 0 and pidx.size:
            if j % 6 == 0 or not live.size:
                target = buf.particles[rng.choice(pidx), :2].astype(np.float64)
            else:
                d = rng.choice(live)
                u = rng.uniform(-0.3, 1.3)
                target = (1.0 - u) * buf.particles[int(buf.beams["a"][d]), :2].astype(np.float64) + u * buf.particles[int(buf.beams["b"][d]), :2]
            if np.isfinite(target).all():
                o = target + (rng.normal(size=2) * 6.0 if j % 12 else 0.0)
        mask = (ALL, ALL, P_ | W_, B_ | W_, P_, B_, W_, P_ | B_)[int(rng.integers(8))]
        rmax = float(rng.uniform(5.0, 120.0)) if (short or j % 4 == 1) else INF
        skip = int(labels[rng.choice(pidx)]) if (j % 6 == 5 and pidx.size) else -1
        rows.append((mask, o[0], o[1], rmax, skip))
    return rows


def case_set(sb):
    """the twelve scenes: dicts of name, buf (None: never uploaded), rows (K packed rows), labels int32 [max_particles], pending"""
    rng = np.random.default_rng(529)
    default = sb.scenes.default_buffers(LAYOUT, *CAP)
    cases = [segments(sb), ties(sb), row_codes(sb), non_finite(sb), masks_and_within(sb)]

    def drawn(name, buf, **kw):
        lab = ref.bodies_labels(buf)
        cases.append(dict(name=name, buf=buf, rows=drawn_rows(buf, rng, lab, **kw)))

    drawn("default", default)
    drawn("default, short reach", default, short=True)
    # a sparse, permuted mapping (graph_cases): particle slot s at data index (5 s + 2) mod 128, beam slot s at (7 s + 3) mod 320
    n, pairs = 40, [(i, i + 1) for i in range(39)] + [(i, i + 8) for i in range(32)]
    sparse = graph_scene(sb, CAP, n, pairs, layout=LAYOUT, pmap=(5 * np.arange(n) + 2) % CAP[0], bmap=(7 * np.arange(len(pairs)) + 3) % CAP[1])
    drawn("sparse permuted mapping", sparse)
    buf, _, pending, removed = ray_cases.removed_and_pending(sb)
    rows = []
    for d in list(pending) + list(removed[:5]):     # rows 0 .. 4 beside the middle of a pending beam, rows 5 .. 9 of a removed one
        pa, pb = (buf.particles[int(buf.beams[e][d]), :2].astype(np.float64) for e in ("a", "b"))
        e = (pb - pa) / np.hypot(*(pb - pa))
        rows.append((B_, *(0.5 * (pa + pb) + 3.0 * np.array([-e[1], e[0]]) + 1.5 * e), 6.0))
    cases.append(dict(name="removed and pending beams", buf=buf, rows=rows + drawn_rows(buf, rng, ref.bodies_labels(buf))[:K - len(rows)],
                      pending=pending, removed=removed))
    broken = default.copy()
    broken.particles[3, :2] = np.nan
    broken.particles[7, 0], broken.particles[20, 1], broken.particles[60, :2] = np.inf, -np.inf, (np.nan, np.inf)
    drawn("NaN and infinite coordinates", broken)
    cases.append(dict(name="never uploaded", buf=None, rows=drawn_rows(default, rng, ref.bodies_labels(default), short=True)))
    p, b = sb.scenes.rectangle(40.0, 40.0, 50.0, 8, 16, 50.0, 700.0, 0.2, 1.0e9, layout=LAYOUT)
    dense = sb.Buffers(LAYOUT, *CAP)
    dense.set_scene(p, b[:CAP[1]])
    cases.append(dict(name="full capacity", buf=dense, rows=drawn_rows(dense, rng, ref.bodies_labels(dense), outside=True)))
    for c in cases:
        c.setdefault("pending", [])
        for key in ("expect", "expect_labelled", "expect_within", "expect_within_labelled"):
            c.setdefault(key, {})
        c["labels"] = np.full(CAP[0], -1, np.int32) if c["buf"] is None else ref.bodies_labels(c["buf"])
        c["rows"] = ref.pack(list(c["rows"]) + [(0, 0, 0, 0)] * (K - len(c["rows"])))
        assert c["rows"].shape == (K, 8)
    assert len(cases) == 12
    return cases


NEVER_UPLOADED = 10   # its place in the set


def stacked(cases):
    """(bufs, rows uint32 [N, K, 8], labels int32 [N, max_particles]) of a case list"""
    return [c["buf"] for c in cases], np.stack([c["rows"] for c in cases]), np.stack([c["labels"] for c in cases])


def coverage(cases):
    """what the set exercises, from the restatement: the kinds seen with and without labels, the branches of the segment test,
    exact ties, rows that skip"""
    kinds, branches, tie_rows, skips = set(), set(), 0, 0
    for labelled in (False, True):
        for c in cases:
            tied = []
            got = ref.nearest_ref(c["buf"], c["rows"], BOUNDS, c["labels"] if labelled else None, ties=tied, branches=branches)
            kinds |= set(got[1][:, 0].tolist())
            tie_rows += sum(1 for n in tied if n > 1)
            if labelled:
                plain = ref.nearest_ref(c["buf"], np.where(np.arange(8) == 4, np.uint32(0xFFFFFFFF), c["rows"]), BOUNDS, c["labels"])
                skips += int(((plain[1] != got[1]).any(axis=1) | (plain[3] != got[3]).any(axis=1)).sum())
    return dict(kinds=kinds, branches=branches, tie_rows=tie_rows, skips=skips)
