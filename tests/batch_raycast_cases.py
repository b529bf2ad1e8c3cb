"""The scenes and rays of tests/test_batch_raycast_cpu.py and tests/test_gpu_batch_raycast.py (BatchEngine.raycast):
twelve small scenes of one capacity, each with its own K rows.  Four are built by hand on integer coordinates, where every t is
known exactly (`expect`: row -> (t, kind, index) for a call without labels, `expect_labelled` for one with the scene's labels); the
others are seeded draws.  Every scene carries `labels` (bodies()'s labels of it, computed on the host) and `pending` (beam data
indices a test may treat as carrying a pending break flag).  coverage() states what the set must exercise."""
import numpy as np

import batch_raycast_ref as ref
from graph_cases import scene as graph_scene

F = np.float32
INF = ref.INF
CAP = (128, 320)
LAYOUT = 2
K = 24
BOUNDS, RADIUS = 1000.0, 10.0
ALL, P_, B_, W_ = 7, ref.PARTICLES, ref.BEAMS, ref.WALLS


def hand_scene(sb, pos, pairs, pmap=None, bmap=None):
    """particles at integer positions `pos` (by slot) and one beam per pair of slots"""
    buf = graph_scene(sb, CAP, len(pos), pairs, layout=LAYOUT, pmap=pmap, bmap=bmap)
    pd = np.arange(len(pos)) if pmap is None else np.asarray(pmap)
    buf.particles[pd, :2] = np.asarray(pos, F)
    return buf


def discs_and_walls(sb):
    buf = hand_scene(sb, [(100, 50)], [])
    rows = [(ALL, 0, 50, 1, 0, INF),          # 0 along +x to the disc at (100, 50), r = 10
            (ALL, 0, 50, 2, 0, INF),          # 1 the same with D = (2, 0)
            (ALL, 95, 50, 1, 0, INF),         # 2 the origin inside the disc
            (ALL, 0, 50, 1, 0, 89),           # 3 stops short
            (ALL, 100, 55, 0, 0, 5),          # 4 a zero D inside the disc ...
            (ALL, 500, 500, 0, 0, 5),         # 5 ... and outside everything
            (W_, 500, 500, -1, 0, INF), (W_, 500, 500, 1, 0, INF), (W_, 500, 500, 0, -1, INF), (W_, 500, 500, 0, 1, INF),   # 6 .. 9 the walls
            (P_, 0, 50, 1, 0, 90),            # 10 tmax == t: kept
            (W_, 0, 300, -1, 0, INF)]         # 11 on the left wall, outwards: t = -0 becomes +0
    expect = {0: (90, 1, 0), 1: (45, 1, 0), 2: (0, 1, 0), 3: (89, 0, -1), 4: (0, 1, 0), 5: (5, 0, -1), 6: (500, 3, 1), 7: (500, 3, 2),
              8: (500, 3, 4), 9: (500, 3, 8), 10: (90, 1, 0), 11: (0, 3, 1)}
    return dict(name="discs and walls", buf=buf, rows=rows, expect=expect, expect_labelled=expect)


def beams(sb):
    buf = hand_scene(sb, [(60, 0), (60, 100), (0, 200), (100, 200)], [(0, 1), (2, 3)])
    rows = [(B_, 0, 50, 1, 0, INF),           # 0 the vertical beam from (60, 0) to (60, 100)
            (B_, 0, 200, 1, 0, INF),          # 1 along the beam at y = 200: parallel
            (B_, 0, 0, 1, 0, INF),            # 2 touches endpoint A exactly: un == 0
            (B_, 0, 100, 1, 0, INF),          # 3 touches endpoint B exactly: un == den
            (B_, 120, 50, -1, 0, INF),        # 4 from the other side: den < 0, all three negated
            (B_, 0, 101, 1, 0, INF),          # 5 just past the end
            (B_ | W_, 0, 50, 1, 0, 59)]       # 6 stops short of beam and wall
    expect = {0: (60, 2, 0), 1: (INF, 0, -1), 2: (60, 2, 0), 3: (60, 2, 0), 4: (60, 2, 0), 5: (INF, 0, -1), 6: (59, 0, -1)}
    return dict(name="beams", buf=buf, rows=rows, expect=expect, expect_labelled=expect)


def ties(sb):
    """slots 0, 1 at data indices 5, 2: two discs mirrored about the ray; slots 2, 3 (data 9, 7): a beam whose endpoint A is the
    ray's origin.  Beam slots 0 at data index 3."""
    buf = hand_scene(sb, [(100, 56), (100, 44), (300, 300), (300, 400)], [(2, 3)], pmap=[5, 2, 9, 7], bmap=[3])
    rows = [(ALL, 0, 50, 1, 0, INF),          # 0 both discs at t = 92: the smaller DATA index (slot 1's) wins
            (ALL, 300, 300, 1, 0, INF),       # 1 particle 9 and beam 3 both at t = 0: the particle wins
            (B_ | W_, 300, 300, 1, 0, INF),   # 2 without particles the beam does
            (ALL, 300, 300, 1, 0, INF, 7),    # 3 body {7, 9} skipped: past the particle and its beam to the right wall
            (ALL, 0, 50, 1, 0, INF, 2)]       # 4 particle 2 skipped: its mirror image
    lab = ref.bodies_labels(buf)
    assert lab[[2, 5, 7, 9]].tolist() == [2, 5, 7, 7]
    return dict(name="ties", buf=buf, rows=rows, expect={0: (92, 1, 2), 1: (0, 1, 9), 2: (0, 2, 3), 3: (0, -2, -1), 4: (0, -2, -1)},
                expect_labelled={0: (92, 1, 2), 1: (0, 1, 9), 2: (0, 2, 3), 3: (700, 3, 2), 4: (92, 1, 5)})


def row_codes(sb):
    nan = float("nan")
    buf = hand_scene(sb, [(100, 50), (200, 50)], [(0, 1)])
    rows = [(0, 0, 50, 1, 0, INF),            # 0 empty
            (8, 0, 50, 1, 0, INF),            # 1 .. 2 an unknown mask bit
            (0x80000001, 0, 50, 1, 0, INF),
            (ALL, INF, 50, 1, 0, INF),        # 3 .. 6 an origin or a direction that is not finite
            (ALL, 0, nan, 1, 0, INF),
            (ALL, 0, 50, -INF, 0, INF),
            (ALL, 0, 50, 1, nan, INF),
            (ALL, 0, 50, 1, 0, -1),           # 7 .. 8 tmax not >= 0
            (ALL, 0, 50, 1, 0, nan),
            (ALL, 0, 50, 1, 0, INF, -1, 1),   # 9 the reserved word
            (ALL, 0, 50, 1, 0, INF, 0),       # 10 a skip_label: invalid without labels; with them it skips body 0, both particles and the beam
            (ALL, 0, 50, 1, 0, -0.0),         # 11 tmax = -0 is >= 0: valid, and only t = 0 fits
            (0, nan, INF, nan, nan, nan, 5, 9),   # 12 mask 0 is empty whatever else the row holds
            (ALL, 0, 50, 1, 0, INF)]          # 13 valid
    expect = {0: (0, -1, -1), 12: (0, -1, -1), 11: (-0.0, 0, -1), 13: (90, 1, 0), 10: (0, -2, -1)}
    expect.update({j: (0, -2, -1) for j in range(1, 10)})
    return dict(name="row codes", buf=buf, rows=rows, expect=expect, expect_labelled={**expect, 10: (1000, 3, 2)})


def drawn_rows(buf, rng, labels, outside=False, short=False):
    """K rows of a seeded draw over a scene: half aimed at a particle or at the middle of a live beam, the rest anywhere"""
    maxP = buf.max_particles
    pidx = buf.mapping[:buf.particle_count].astype(np.int64)
    live = buf.mapping[maxP:maxP + buf.beam_count].astype(np.int64)
    rows = []
    for j in range(K):
        o = rng.uniform(-300.0, 1300.0, 2) if outside else rng.uniform(0.0, 1000.0, 2)
        if j % 2 == 0 and pidx.size:
            if j % 4 == 0 or not live.size:
                target = buf.particles[rng.choice(pidx), :2].astype(np.float64)
            else:
                d = rng.choice(live)
                target = 0.5 * (buf.particles[int(buf.beams["a"][d]), :2].astype(np.float64) + buf.particles[int(buf.beams["b"][d]), :2])
            direction = target - o if np.isfinite(target).all() else rng.normal(size=2)
            if j % 8 == 0:
                direction /= np.hypot(*direction) or 1.0
        else:
            direction = rng.normal(size=2) * (1.0e3 if j % 5 == 0 else 1.0)
        mask = (ALL, ALL, P_ | W_, B_ | W_, P_, B_, W_, P_ | B_)[int(rng.integers(8))]
        tmax = float(rng.uniform(50.0, 400.0)) / max(float(np.hypot(*direction)), 1e-3) if (short or j % 3 == 0) else INF
        skip = int(labels[rng.choice(pidx)]) if (j % 6 == 5 and pidx.size) else -1
        rows.append((mask, o[0], o[1], direction[0], direction[1], tmax, skip))
    return rows


def removed_and_pending(sb):
    """the default scene with seven beams removed (their slots compacted away, as a delete pass leaves the mapping) and five live
    ones named `pending`; rows 0 .. 4 cross a pending beam at its middle from 4 away, rows 5 .. 9 a removed one"""
    buf = sb.scenes.default_buffers(LAYOUT, *CAP)
    maxP = buf.max_particles
    live = buf.mapping[maxP:maxP + buf.beam_count].astype(np.int64)
    removed, pending = live[[3, 40, 41, 100, 180, 250, 298]], live[[0, 30, 120, 200, 290]]
    kept = live[~np.isin(live, removed)]
    buf.mapping[maxP:maxP + kept.size] = kept
    buf.beam_count = kept.size
    rows = []
    for d in list(pending) + list(removed[:5]):
        pa, pb = buf.particles[int(buf.beams["a"][d]), :2].astype(np.float64), buf.particles[int(buf.beams["b"][d]), :2].astype(np.float64)
        mid, e = 0.5 * (pa + pb), (pb - pa) / np.hypot(*(pb - pa))
        n = np.array([-e[1], e[0]])
        rows.append((B_, *(mid + 4.0 * n + 1.5 * e), *(-n), 8.0))
    return buf, rows, [int(d) for d in pending], [int(d) for d in removed]


def case_set(sb):
    """the twelve scenes: dicts of name, buf (None: never uploaded), rows (K tuples), labels int32 [max_particles], pending"""
    rng = np.random.default_rng(527)
    default = sb.scenes.default_buffers(LAYOUT, *CAP)
    cases = [discs_and_walls(sb), beams(sb), ties(sb), row_codes(sb)]

    def drawn(name, buf, **kw):
        lab = ref.bodies_labels(buf)
        cases.append(dict(name=name, buf=buf, rows=drawn_rows(buf, rng, lab, **kw)))

    drawn("default", default)
    drawn("default, short rays", default, short=True)
    # a sparse, permuted mapping (graph_cases): particle slot s at data index (5 s + 2) mod 128, beam slot s at (7 s + 3) mod 320
    n, pairs = 40, [(i, i + 1) for i in range(39)] + [(i, i + 8) for i in range(32)]
    sparse = graph_scene(sb, CAP, n, pairs, layout=LAYOUT, pmap=(5 * np.arange(n) + 2) % CAP[0], bmap=(7 * np.arange(len(pairs)) + 3) % CAP[1])
    drawn("sparse permuted mapping", sparse)
    buf, rows, pending, removed = removed_and_pending(sb)
    lab = ref.bodies_labels(buf)
    cases.append(dict(name="removed and pending beams", buf=buf, rows=rows + drawn_rows(buf, rng, lab)[:K - len(rows)], pending=pending, removed=removed))
    broken = default.copy()
    broken.particles[3, :2] = np.nan
    broken.particles[7, 0], broken.particles[20, 1], broken.particles[60, :2] = np.inf, -np.inf, (np.nan, np.inf)
    drawn("NaN and infinite coordinates", broken)
    cases.append(dict(name="never uploaded", buf=None, rows=drawn_rows(default, rng, ref.bodies_labels(default))))
    drawn("origins outside the box", default, outside=True)
    p, b = sb.scenes.rectangle(40.0, 40.0, 50.0, 8, 16, 50.0, 700.0, 0.2, 1.0e9, layout=LAYOUT)
    dense = sb.Buffers(LAYOUT, *CAP)
    dense.set_scene(p, b[:CAP[1]])
    drawn("full capacity", dense)
    for c in cases:
        c.setdefault("pending", [])
        c.setdefault("expect", {})
        c.setdefault("expect_labelled", {})
        c["labels"] = np.full(CAP[0], -1, np.int32) if c["buf"] is None else ref.bodies_labels(c["buf"])
        c["rows"] = ref.pack(list(c["rows"]) + [(0, 0, 0, 0, 0, 0)] * (K - len(c["rows"])))
        assert c["rows"].shape == (K, 8)
    assert len(cases) == 12
    return cases


def stacked(cases):
    """(bufs, rows uint32 [N, K, 8], labels int32 [N, max_particles]) of a case list"""
    return [c["buf"] for c in cases], np.stack([c["rows"] for c in cases]), np.stack([c["labels"] for c in cases])


def coverage(cases):
    """what the set exercises, from the restatement: the kinds seen with and without labels, exact ties, rows that skip"""
    kinds, tie_rows, skips = set(), 0, 0
    for labelled in (False, True):
        for c in cases:
            tied = []
            _, hit, _ = ref.raycast_ref(c["buf"], c["rows"], BOUNDS, RADIUS, c["labels"] if labelled else None, ties=tied)
            kinds |= set(hit[:, 0].tolist())
            tie_rows += sum(1 for n in tied if n > 1)
            if labelled:
                plain = ref.raycast_ref(c["buf"], np.where(np.arange(8) == 6, np.uint32(0xFFFFFFFF), c["rows"]), BOUNDS, RADIUS, c["labels"])[1]
                skips += int((plain != hit).any(axis=1).sum())
    return dict(kinds=kinds, tie_rows=tie_rows, skips=skips)
