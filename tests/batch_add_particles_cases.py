"""The scenes and rows of tests/test_gpu_batch_add_particles.py and tests/test_gpu_batch_add_particles_width.py
(BatchEngine.add_particles), all small; tests/test_batch_add_particles_cpu.py runs every case through
tests/batch_add_particles_ref.py and the oracle alone and asserts what each case is built for."""
import numpy as np

import batch_add_beams_cases as beam_cases
import batch_add_particles_ref as ref
from float_keys import fkey, unkey

F = np.float32
DEFAULT_CAP = (128, 320)               # the default scene is 119 / 299: nine free particle slots
K = 4
RADIUS = 10.0


def default_case(sb, n=8):
    """n default scenes, each with its own K rows.  Row 0 flies at the left wall (x = 14, vx = -12: it reaches x <= 10 inside the
    first frame), row 1 sits 15 above the top particle of the body at (185, 70) and falls onto it, row 2 is a seeded draw in the
    empty middle of the box with a seeded velocity and acceleration, row 3 is an empty or an invalid row in turn."""
    buf = sb.scenes.default_buffers(1, *DEFAULT_CAP)
    rng = np.random.default_rng(26)
    rows = []
    for i in range(n):
        r = [(i, 14.0, 400.0 + 20.0 * i, -12.0, 0.0),
             (i, 185.0 + 0.25 * i, 85.0, 0.0, -1.0),
             (7, *(300.0 + 300.0 * rng.random(2)), *(4.0 * rng.normal(size=4)))]
        r.append([(-1 - i, 500.0, 500.0), (0, float("nan"), 500.0), (0, 500.0, float("inf")), (0, 500.0, 500.0, 0, 0, 0, 0, 1)][i % 4])
        rows.append(ref.pack(r))
    return dict(layout=1, cap=DEFAULT_CAP, bufs=[buf] * n, rows=np.stack(rows), flags=0)


def step_ulps(x, n):
    """the float32 n ulps above (n < 0: below) the positive float32 x"""
    return float(unkey(np.uint32(int(fkey(F(x))) + n)))


def codes_case(sb):
    """One default scene and rows of every code, for SKIP_TOUCHING.  The particle at data index 1 is (185, 70): a row at
    (185 + 20, 70) is exactly 2r away and is added, one ulp closer is BLOCKED, a coincident row is BLOCKED."""
    buf = sb.scenes.default_buffers(1, *DEFAULT_CAP)
    nan, inf = float("nan"), float("inf")
    x2r = 205.0
    rows = [(0, x2r, 70.0),                         # 0 exactly 2r from particle 1: added
            (0, step_ulps(265.0, -1), 70.0),        # 1 one ulp closer than 2r to particle 3 at (245, 70): BLOCKED
            (0, 185.0, 70.0),                       # 2 coincident with particle 1: BLOCKED
            (0, nan, 500.0),                        # 3 .. 6 INVALID: x NaN, y -inf, x +inf, reserved != 0
            (0, 500.0, -inf),
            (0, inf, 500.0),
            (0, 500.0, 500.0, 0, 0, 0, 0, 7),
            (-5, 500.0, 500.0),                     # 7 EMPTY
            (3, 500.0, 500.0, nan, inf, -inf, nan),  # 8 added: velocity and acceleration are taken verbatim
            (3, 510.0, 500.0),                      # 9 touches row 8, a clean earlier row: BLOCKED
            (3, 520.0, 505.0),                      # 10 touches row 9 (BLOCKED by a row, not E: it still blocks), not row 8: BLOCKED
            (3, 190.0, 75.0),                       # 11 E: touches particle 1
            (3, 176.0, 88.0),                       # 12 touches row 11 (which is E and so does not block), no particle and no other row: added
            (3, -50.0, 2000.0),                     # 13 outside the box: legal, added
            (0, 0.0, 0.0, 0, 0, 0, 0, 0)]           # 14 added
    return dict(layout=1, cap=DEFAULT_CAP, bufs=[buf], rows=ref.pack(rows)[None], flags=ref.SKIP_TOUCHING)


def lattice(sb, cap, w=4, h=4, layout=1, at=(200.0, 200.0)):
    p, b = sb.scenes.rectangle(at[0], at[1], 40.0, w, h, 50.0, 700.0, 0.2, 1.0e9, layout=layout)
    buf = sb.Buffers(layout, *cap)
    buf.set_scene(p, b)
    return buf


ROOM_CAP = (19, 64)


def room_case(sb):
    """P = cap - 3 with five rows: three added, two FULL; a full scene (19 of 19: a 4 x 4 rectangle and three free particles);
    a scene never uploaded (every counted row INVALID)"""
    a = lattice(sb, ROOM_CAP)
    full = lattice(sb, ROOM_CAP)
    full.particles[16:19, :2] = [[600.0, 600.0], [650.0, 600.0], [700.0, 600.0]]
    full.mapping[16:19] = [16, 17, 18]
    full.particle_count = 19
    rows = ref.pack([(0, 500.0 + 30.0 * j, 800.0) for j in range(4)] + [(-1, 0.0, 0.0), (0, 700.0, 800.0)])
    return dict(layout=1, cap=ROOM_CAP, bufs=[a, full, None], rows=np.stack([rows] * 3), flags=0)


SPARSE_CAP = (32, 64)


def sparse_case(sb):
    """beam_cases.sparse_case's scene: particle slot s at data index (5 s + 2) mod 32, sparse and out of slot order.  Three rows: the
    new particles take the smallest free data indices 1, 4, 6 -- not P = 16."""
    case = beam_cases.sparse_case(sb)
    rows = ref.pack([(0, 500.0 + 40.0 * j, 600.0, 1.0, 2.0) for j in range(3)])
    return dict(layout=2, cap=SPARSE_CAP, bufs=case["bufs"], rows=rows[None], flags=0)


ONE_FREE_CAP = (17, 64)


def one_free_case(sb):
    """a 4 x 4 rectangle at capacity 17: one free slot, for three spawn - reset episodes"""
    rows = ref.pack([(0, 600.0, 600.0, -3.0, 1.0)])
    return dict(layout=1, cap=ONE_FREE_CAP, bufs=[lattice(sb, ONE_FREE_CAP)], rows=rows[None], flags=0)


TRIANGLE = [(0.0, 0.0), (30.0, 0.0), (15.0, 26.0)]
TRIANGLE_EDGES = [(0, 1), (1, 2), (2, 0)]
MAT = beam_cases.MAT


def triangle_rows(n, at=(500.0, 500.0), v=(0.0, -2.0)):
    """n scenes' rows of a triangle body (three particles), scene i's shifted by 5 i in x"""
    return np.stack([ref.pack([(0, at[0] + 5.0 * i + x, at[1] + y, *v) for x, y in TRIANGLE]) for i in range(n)])


def expected(case, flags=None, loaded=None):
    """per scene (edited buffers, result, counts) of the restatement; loaded: the scenes as read back (None: as uploaded)"""
    bufs = case["bufs"] if loaded is None else loaded
    flags = case["flags"] if flags is None else flags
    return [ref.add_ref(b, case["rows"][i], flags, case.get("radius", RADIUS)) for i, b in enumerate(bufs)]


# ---------------------------------------------------------------- full width and capacity (tests/test_gpu_batch_add_particles_width.py)

BIG_CAP = (1024, 4096)


def big_scene(sb, P, free=None, seed=41, spacing=25.0):
    """P particles on a 32-wide lattice of the given spacing (no beams), with a shuffled mapping; free: the data indices left free
    (len == 1024 - P), None: a seeded draw"""
    rng = np.random.default_rng(seed)
    maxP = BIG_CAP[0]
    if free is None:
        data = rng.permutation(maxP)[:P]
    else:
        assert len(set(free)) == maxP - P
        data = rng.permutation(np.setdiff1d(np.arange(maxP), free))
    buf = sb.Buffers(2, *BIG_CAP)
    s = np.arange(P)
    buf.particles[data, 0], buf.particles[data, 1] = 30.0 + spacing * (s % 32), 30.0 + spacing * (s // 32)
    buf.mapping[:P] = data
    buf.particle_count, buf.beam_count = P, 0
    return buf


def sixty_four_case(sb):
    """64 rows in one call into a scene of 960 of 1024 whose free data indices are 12 even ones of bitmap words 0 and 1 and
    972 .. 1023, the end of word 30 and the whole of the last word: the scene is filled to exactly 1024.  A second scene of 1000
    takes 24 and refuses 40."""
    free = sorted(list(range(972, 1024)) + list(range(0, 64, 2))[:12])
    a, b = big_scene(sb, 960, free), big_scene(sb, 1000, seed=42)
    rows = ref.pack([(j, 40.0 + 14.0 * j, 960.0, 0.0, -1.0) for j in range(64)])
    return dict(layout=2, cap=BIG_CAP, bufs=[a, b], rows=np.stack([rows, rows]), flags=0)


def threshold_case(sb):
    """P from 250 to 260 across the default grid_min_particles of 256: ten rows above the lattice, falling onto it"""
    buf = big_scene(sb, 250, seed=43)
    rows = ref.pack([(0, 100.0 + 50.0 * j, 30.0 + 25.0 * 8 + 18.0, 0.0, -2.0) for j in range(10)])
    return dict(layout=2, cap=BIG_CAP, bufs=[buf], rows=rows[None], flags=0)


ODD_CAPS = [(33, 37), (65, 61)]


def odd_case(sb, cap):
    """beam_cases.odd_case's scene (25 particles, the last at data index max_particles - 1) in scene 1 of three; as many rows as
    free slots plus two: the last added row takes the largest free index, two are FULL.  Scenes 0 and 2 get empty rows."""
    buf = beam_cases.odd_case(sb, cap)["bufs"][1]
    n = cap[0] - 25 + 2
    rows = ref.pack([(0, 500.0 + 11.0 * j, 700.0 + 30.0 * (j % 3), 0.5, 0.0) for j in range(n)])
    return dict(layout=2, cap=cap, bufs=[buf, buf, buf], rows=np.stack([np.full_like(rows, -1), rows, np.full_like(rows, -1)]), flags=0)


def halves_case(sb):
    """SKIP_TOUCHING with rows 32 .. 63 blocked by rows 0 .. 31: row 32 + j sits 12 to the right of row j (rows are 40 apart, so
    it touches row j alone, and no particle of the 4 x 4 rectangle far below)"""
    buf = lattice(sb, (128, 64), layout=2, at=(100.0, 50.0))
    first = [(j, 30.0 + 40.0 * (j % 16), 600.0 + 40.0 * (j // 16)) for j in range(32)]
    rows = ref.pack(first + [(32 + j, x + 12.0, y) for j, x, y in first])
    return dict(layout=2, cap=(128, 64), bufs=[buf], rows=rows[None], flags=ref.SKIP_TOUCHING)
