"""The scenes and rows of tests/test_gpu_batch_add_beams.py (BatchEngine.add_beams), all small; the CPU test runs
every case through tests/batch_add_beams_ref.py and the oracle alone."""
import numpy as np

import batch_add_beams_ref as ref

F = np.float32
MAT = (1.0, 50.0, 1.0, 2.5)            # spring, damp, yield_strain, strain_break_limit of the default scene's first bodies
DEFAULT_CAP = (128, 320)               # the default scene is 119 / 299
K = 8


def cur(buf, a, b):
    return float(ref.distance(buf.particles[a], buf.particles[b]))


def default_case(sb, n=8):
    """n default scenes, each with its own K rows: pairs of a seeded draw at 0.95 .. 1.05 of their distance, one row of each scene
    empty and one invalid (a == b); scene 2's first row breaks at once (a tiny strain_break_limit on a beam 10 % short)."""
    buf = sb.scenes.default_buffers(1, *DEFAULT_CAP)
    rng = np.random.default_rng(24)
    rows = []
    for i in range(n):
        r = []
        for j in range(K):
            a, b = (int(v) for v in rng.choice(buf.particle_count, 2, replace=False))
            r.append((a, b, cur(buf, a, b) * (0.95 + 0.1 * rng.random())) + MAT)
        r[i % K] = (-1 - i, 5, 10.0) + MAT
        r[(i + 3) % K] = (7 + i, 7 + i, 10.0) + MAT
        if i == 2:
            a, b = r[0][0], r[0][1]
            r[0] = (a, b, cur(buf, a, b) * 0.9, 1.0, 50.0, 1.0, 1.0e-4)
        rows.append(ref.pack(r))
    return dict(layout=1, cap=DEFAULT_CAP, bufs=[buf] * n, rows=np.stack(rows), breaking=(2, 0))


def codes_case(sb):
    """One default scene whose two free particles (44 and 45) coincide, the beam (0, 1) to be cut (a disc that hits it alone), and rows of
    every code.  Returns (case, the shapes [1, 1, 8] of that cut)."""
    buf = sb.scenes.default_buffers(1, *DEFAULT_CAP)
    buf.particles[45, :2] = buf.particles[44, :2]
    nan, inf = float("nan"), float("inf")
    rows = [(128, 3, 10.0) + MAT,            # 0 out of range (a)
            (3, 4000, 10.0) + MAT,           # 1 out of range (b)
            (9, 9, 10.0) + MAT,              # 2 a == b
            (120, 3, 10.0) + MAT,            # 3 a data index no particle holds
            (3, 5, 10.0) + MAT + (1,),       # 4 reserved != 0
            (3, 5, 0.0) + MAT,               # 5 .. 8 length 0 / NaN / -1 / +inf (INVALID unless LENGTH_CURRENT resolves it)
            (3, 6, nan) + MAT,
            (3, 7, -1.0) + MAT,
            (3, 8, inf) + MAT,
            (44, 45, 25.0) + MAT,            # 9 coincident endpoints: INVALID under LENGTH_CURRENT only
            (2, 3, 60.0) + MAT,              # 10 a pair a live beam joins
            (1, 0, 60.0) + MAT,              # 11 a pair joined only by a beam with a pending break flag (endpoints swapped)
            (10, 40, 100.0) + MAT,           # 12 a new pair ...
            (40, 10, 100.0) + MAT,           # 13 ... and its duplicate in the call
            (-1, -1, 0.0, 0.0, 0.0, 0.0, 0.0),   # 14 a < 0
            (3, -5, 10.0) + MAT]             # 15 b < 0: no data index
    shapes = np.zeros((1, 1, 8), np.uint32)
    shapes[0, 0, 0] = 2
    shapes[0, 0, 1:4] = np.asarray([185.0, 40.0, 1.0], F).view(np.uint32)
    return dict(layout=1, cap=DEFAULT_CAP, bufs=[buf], rows=ref.pack(rows)[None]), shapes


def lattice(sb, cap, beams, layout=1):
    """a 4 x 4 rectangle of the reference's (16 particles, 42 beams), its first `beams` beams"""
    p, b = sb.scenes.rectangle(200.0, 200.0, 40.0, 4, 4, 50.0, 700.0, 0.2, 1.0e9, layout=layout)
    buf = sb.Buffers(layout, *cap)
    buf.set_scene(p, b[:beams])
    return buf


ROOM_CAP = (64, 40)
# eight pairs no beam of the 4 x 4 rectangle joins (two columns apart)
ROOM_PAIRS = [(0, 8), (1, 9), (2, 10), (3, 11), (4, 12), (5, 13), (6, 14), (7, 15)]


def room_case(sb):
    """36 beams of 40 (four rows find room), 40 of 40 (none does), a scene never uploaded"""
    a, b = lattice(sb, ROOM_CAP, 36), lattice(sb, ROOM_CAP, 40)
    rows = ref.pack([(x, y, 80.0, 50.0, 700.0, 0.2, 1.0e9) for x, y in ROOM_PAIRS])
    return dict(layout=1, cap=ROOM_CAP, bufs=[a, b, None], rows=np.stack([rows] * 3))


SPARSE_CAP = (32, 64)


def sparse_case(sb):
    """The 4 x 4 rectangle's first 30 beams with both mappings scattered: particle slot s at data index (5 s + 2) mod 32, beam
    slot s at data index (7 s + 3) mod 64 -- sparse, and not in slot order.  Five rows: the new slots 30 .. 34 straddle a flag word."""
    src = lattice(sb, SPARSE_CAP, 30, layout=2)
    maxP, maxB = SPARSE_CAP
    pd = (5 * np.arange(16) + 2) % maxP
    bd = (7 * np.arange(30) + 3) % maxB
    buf = sb.Buffers(2, maxP, maxB)
    buf.particles[pd] = src.particles[:16]
    rec = src.beams[:30].copy()
    rec["a"], rec["b"] = pd[rec["a"]], pd[rec["b"]]
    buf.beams[bd] = rec
    buf.mapping[:16] = pd
    buf.mapping[maxP:maxP + 30] = bd
    buf.particle_count, buf.beam_count = 16, 30
    rows = ref.pack([(int(pd[x]), int(pd[y]), 80.0, 50.0, 700.0, 0.2, 1.0e9) for x, y in ROOM_PAIRS[:5]])
    return dict(layout=2, cap=SPARSE_CAP, bufs=[buf], rows=rows[None])


TOUCH_CAP = (16, 32)


def touching_case(sb):
    """two 2 x 2 bodies (spacing 30) side by side, 15 apart: each particle of the first's right column touches its neighbour"""
    p1, b1 = sb.scenes.rectangle(300.0, 300.0, 30.0, 2, 2, *MAT, layout=1)
    p2, b2 = sb.scenes.rectangle(345.0, 300.0, 30.0, 2, 2, *MAT, base=4, layout=1)
    buf = sb.Buffers(1, *TOUCH_CAP)
    buf.set_scene(np.concatenate([p1, p2]), np.concatenate([b1, b2]))
    return dict(layout=1, cap=TOUCH_CAP, bufs=[buf, buf])


def expected(case, flags=0, loaded=None, reset_alive=None):
    """per scene (edited buffers, result, counts) of the restatement; loaded: the scenes as read back (None: as uploaded)"""
    bufs = case["bufs"] if loaded is None else loaded
    out = []
    for i, b in enumerate(bufs):
        ra = reset_alive[i] if reset_alive is not None else (None if case["bufs"][i] is None else ref.alive_set(case["bufs"][i]))
        out.append(ref.add_ref(b, case["rows"][i], flags, ra))
    return out
