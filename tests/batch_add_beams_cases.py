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


# ---------------------------------------------------------------- full width and capacity (tests/test_gpu_batch_add_beams_width.py)
# Every case below is a dict like the ones above plus `flags`; tests/test_batch_add_beams_cpu.py asserts, on the restatement alone,
# the structural facts each is named for, so that an edit of a generator cannot turn one into an easy case unnoticed.

SOFT = MAT
WIDE_CAP = (32, 128)


def scattered(sb, cap, w, h, beams, pd, bd, layout=2):
    """A w x h rectangle's first `beams` beams with particle slot s at data index pd[s] and beam slot s at data index bd[s]"""
    maxP, maxB = cap
    p, b = sb.scenes.rectangle(200.0, 200.0, 40.0, w, h, 50.0, 700.0, 0.2, 1.0e9, layout=layout)
    pd, bd = np.asarray(pd[:len(p)], dtype=np.int64), np.asarray(bd[:beams], dtype=np.int64)
    assert len(set(pd.tolist())) == len(p) and len(set(bd.tolist())) == beams and pd.max() < maxP and bd.max() < maxB
    buf = sb.Buffers(layout, maxP, maxB)
    buf.particles[pd, :2] = p
    rec = b[:beams].copy()
    rec["a"], rec["b"] = pd[rec["a"].astype(np.int64)], pd[rec["b"].astype(np.int64)]
    buf.beams[bd] = rec
    buf.mapping[:len(p)] = pd
    buf.mapping[maxP:maxP + beams] = bd
    buf.particle_count, buf.beam_count = len(p), beams
    return buf


def wide_lattice(sb, beams):
    """sparse_case's scatter at capacity 32 / 128: particle slot s at (5 s + 2) mod 32, beam slot s at (7 s + 3) mod 128"""
    return scattered(sb, WIDE_CAP, 4, 4, beams, (5 * np.arange(16) + 2) % 32, (7 * np.arange(beams) + 3) % 128)


def pairs_of(buf):
    """(the unordered pairs a live beam joins, every other pair of the scene's particles in a fixed order), as data indices"""
    maxP = buf.max_particles
    live = buf.mapping[maxP:maxP + buf.beam_count].astype(np.int64)
    joined = [(int(buf.beams["a"][d]), int(buf.beams["b"][d])) for d in live]
    have = {frozenset(p) for p in joined}
    pd = [int(d) for d in buf.mapping[:buf.particle_count]]
    other = [(pd[i], pd[j]) for i in range(len(pd)) for j in range(i + 1, len(pd)) if frozenset((pd[i], pd[j])) not in have]
    order = np.random.default_rng(5).permutation(len(other))
    return joined, [other[i] for i in order]


def weld(buf, a, b, scale=1.0):
    """a row that joins a and b at `scale` times their present distance, soft"""
    return (a, b, cur(buf, a, b) * scale) + SOFT


def quarter_discs(buf, slots):
    """one disc of radius 1 per beam slot, a quarter along the beam (where neither a diagonal's crossing nor a lattice node is)"""
    maxP = buf.max_particles
    out = np.zeros((len(slots), 8), np.uint32)
    for i, s in enumerate(slots):
        d = int(buf.mapping[maxP + s])
        pa, pb = buf.particles[int(buf.beams["a"][d]), :2], buf.particles[int(buf.beams["b"][d]), :2]
        out[i, 0] = 2
        out[i, 1:4] = np.asarray([0.75 * pa[0] + 0.25 * pb[0], 0.75 * pa[1] + 0.25 * pb[1], 1.0], F).view(np.uint32)
    return out


FLAG_WORD_CASES = {"three-words": (30, 64), "one-whole-word": (32, 32), "two-words-one-bit-each": (31, 2)}


def flag_words_case(sb, name):
    """1: Bc live beams, k rows that all find room, so that the new slots Bc .. Bc + k - 1 span the flag words the name says; the
    two slots before them (Bc - 2 and Bc - 1: 28 and 29 of word 0 in the first case) are cut first and stay pending."""
    bc, k = FLAG_WORD_CASES[name]
    buf = wide_lattice(sb, bc)
    _, other = pairs_of(buf)
    rows = ref.pack([weld(buf, a, b) for a, b in other[:k]])
    return dict(layout=2, cap=WIDE_CAP, bufs=[buf], rows=rows[None], flags=0, cut=quarter_discs(buf, [bc - 2, bc - 1])[None], cut_slots=[bc - 2, bc - 1])


UPPER_SPECIAL = (31, 32, 63)


def upper_half_case(sb):
    """2: three scenes of 64 rows under SKIP_JOINED.  Rows 33 and 47 (endpoints swapped) name pairs a live beam joins, and so does
    row 63 where it is free for it (scene 0; in scenes 1 and 2 that row is 61); row 40 repeats the pair of row 3 (swapped), row 62
    the pair of row 35.  An INVALID and an EMPTY row go round the rows 31, 32 and 63: scene s has the INVALID one at
    UPPER_SPECIAL[s] and the EMPTY one at UPPER_SPECIAL[s + 1], so each of the three rows is once invalid, once empty and once a
    candidate, and the ranks of the rows behind them shift across the half boundary.  `joined_rows`: per scene, the rows to be JOINED."""
    buf = wide_lattice(sb, 30)
    joined, other = pairs_of(buf)
    rows, want = [], []
    for s in range(3):
        inv, emp = UPPER_SPECIAL[s], UPPER_SPECIAL[(s + 1) % 3]
        r = [weld(buf, a, b) for a, b in other[:64]]
        third = 63 if 63 not in (inv, emp) else 61
        for j, (a, b) in ((33, joined[5]), (47, joined[17][::-1]), (third, joined[29])):
            r[j] = weld(buf, a, b)
        r[40] = weld(buf, r[3][1], r[3][0])
        r[62] = weld(buf, r[35][0], r[35][1])
        r[inv] = (7, 7, 10.0) + SOFT
        r[emp] = (-1, 5, 10.0) + SOFT
        rows.append(ref.pack(r))
        want.append(sorted({33, 47, third, 40, 62} - {inv, emp}))
    return dict(layout=2, cap=WIDE_CAP, bufs=[buf] * 3, rows=np.stack(rows), flags=ref.SKIP_JOINED, joined_rows=want)


BIG_CAP = (1024, 4096)
BIG_FREE = [4001, 4003, 4005, 4007, 4009, 4011, 4030, 4031] + list(range(4033, 4096, 2))    # 40 indices, six of them in word 125


def big_edges():
    """4096 beams between lattice neighbours of a 32 x 32 lattice of DATA indices (d and d + 1, d + 32, d + 33, d + 1 and d + 32:
    3906) and second neighbours in x (190), as pairs of data indices"""
    d = np.arange(1024).reshape(32, 32)
    e = [np.stack([d[:, :-1].ravel(), d[:, 1:].ravel()], 1), np.stack([d[:-1].ravel(), d[1:].ravel()], 1),
         np.stack([d[:-1, :-1].ravel(), d[1:, 1:].ravel()], 1), np.stack([d[:-1, 1:].ravel(), d[1:, :-1].ravel()], 1),
         np.stack([d[:, :-2].ravel(), d[:, 2:].ravel()], 1)[:190]]
    return np.concatenate(e)


def big_scene(sb, m, seed, free=None):
    """batch_bodies_cases.graph_scene at 1024 / 4096 with shuffled mappings: 1024 particles, the first m of big_edges() at rest (every
    length the endpoints' distance).  free: the beam data indices to leave free (len == 4096 - m): the others keep their order."""
    import batch_bodies_cases as bb
    D = np.random.default_rng(seed).permutation(1024)
    number = np.argsort(D)                                  # data index -> particle number
    buf, D2 = bb.graph_scene(sb, BIG_CAP, 1024, number[big_edges()[:m]].tolist(), seed=seed)
    assert np.array_equal(D, D2)
    maxP, maxB = BIG_CAP
    if free is not None:
        live = buf.mapping[maxP:maxP + m].astype(np.int64)
        assert len(free) == maxB - m
        room = np.setdiff1d(np.arange(maxB), free)          # ascending; rank among the used indices -> new index
        new = room[np.searchsorted(np.sort(live), live)]
        rec = buf.beams[live].copy()
        buf.beams[:] = 0
        buf.beams[new] = rec
        buf.mapping[maxP:maxP + m] = new
    live = buf.mapping[maxP:maxP + m].astype(np.int64)
    pa, pb = buf.particles[buf.beams["a"][live].astype(np.int64)], buf.particles[buf.beams["b"][live].astype(np.int64)]
    length = np.asarray([ref.distance(x, y) for x, y in zip(pa, pb)], F)
    for f in ("length", "target_length", "last_length"):
        col = buf.beams[f]
        col[live] = length
    return buf


def big_case(sb):
    """3: (a) 4056 beams, the 40 free indices BIG_FREE; 64 rows, 40 of which find room.  (b) 4096 beams: 64 x FULL.  (c) 700 beams
    under SKIP_JOINED: every fourth row names the pair of a live beam in a slot above 512 (the fourth trip of the sweep's loop)."""
    a, b, c = big_scene(sb, 4056, 31, BIG_FREE), big_scene(sb, 4096, 32), big_scene(sb, 700, 33)
    second = [(d, d + 64) for d in range(0, 64 * 14, 14)][:64]            # second neighbours in y: no beam joins them
    assert all(y < 1024 for _, y in second)
    rows = []
    for buf in (a, b):
        rows.append(ref.pack([weld(buf, x, y) for x, y in second]))
    maxP = BIG_CAP[0]
    late = [int(d) for d in c.mapping[maxP + 513:maxP + 700:12]]
    r = [weld(c, x, y) for x, y in second]
    joined_rows = list(range(1, 64, 4))
    for j, d in zip(joined_rows, late):
        x, y = int(c.beams["a"][d]), int(c.beams["b"][d])
        r[j] = weld(c, y, x) if j % 8 == 1 else weld(c, x, y)
    rows.append(ref.pack(r))
    return dict(layout=2, cap=BIG_CAP, bufs=[a, b, c], rows=np.stack(rows), flags=ref.SKIP_JOINED, joined_rows=joined_rows, late_slots=(513, 700, 12))


def no_index_case(sb):
    """4: capacity == the uploaded beam count (40 of 40).  Three beams are cut and a frame removes them: three slots are free, but
    every data index is still held by the reset state.  `cut_slots`: the beams cut (identity mapping: their data indices)."""
    buf = lattice(sb, ROOM_CAP, 40)
    slots = [7, 20, 33]
    rows = ref.pack([(x, y, 80.0, 50.0, 700.0, 0.2, 1.0e9) for x, y in ROOM_PAIRS[:3]])
    return dict(layout=1, cap=ROOM_CAP, bufs=[buf], rows=rows[None], flags=0, cut=quarter_discs(buf, slots)[None], cut_slots=slots)


ODD_CAPS = [(33, 37), (65, 61)]
ODD_FREE = 5


def odd_case(sb, cap):
    """5: a 5 x 5 rectangle's first max_beams - 5 beams at an odd capacity, its last particle at data index max_particles - 1, the
    free beam indices four shuffled ones and max_beams - 1.  Seven rows that join the last particle to others: five find room, the
    fifth takes the last index, two are FULL.  Scene 1 of three; scenes 0 and 2 hold the same scene and get empty rows."""
    maxP, maxB = cap
    rng = np.random.default_rng(maxP)
    pd = np.concatenate([rng.permutation(maxP - 1)[:24], [maxP - 1]])
    bd = rng.permutation(maxB - 1)[:maxB - ODD_FREE]
    buf = scattered(sb, cap, 5, 5, maxB - ODD_FREE, pd, bd)
    _, other = pairs_of(buf)
    last = [p for p in other if maxP - 1 in p][:ODD_FREE + 2]
    rows = ref.pack([weld(buf, a, b) for a, b in last])
    return dict(layout=2, cap=cap, bufs=[buf, buf, buf], rows=np.stack([np.full_like(rows, -1), rows, np.full_like(rows, -1)]), flags=ref.SKIP_JOINED)
