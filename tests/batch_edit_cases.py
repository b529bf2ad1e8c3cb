"""Seeded edit programs for tests/test_gpu_batch_edit_program.py: twelve small scenes at one capacity and about thirty batch-wide
ops -- frame, step, delete pass, cut, add_beams, reset, checkpoint, fork, and dry runs of cut and add -- drawn with a seed.  The rows
of an add and the shapes of a cut are drawn from the scenes as they are at that point of the program, so the generator runs the
host model (tests/batch_edit_model.py) while it draws; tests/test_batch_edit_model_cpu.py runs every program on the model alone
and asserts the conditions that make the GPU test meaningful."""
import functools
import os
import sys

import numpy as np

import batch_add_beams_ref as add_ref
import batch_edit_model as model
import cut_ref

F = np.float32
CAP = (48, 96)
LAYOUT = 2
N = 12
NEVER = 6            # the scene never uploaded: its physics constants are zero words, so no fork makes it a destination
FULL_SCENE = 7
MAT = (1.0, 50.0, 1.0, 2.5)          # the default scene's soft material: welded lattices stay finite
SEEDS = (1, 2, 3)
OP_KINDS = ("frame", "step", "delete", "cut", "add", "reset", "checkpoint", "fork map", "fork swap", "fork broadcast", "add dry", "cut dry")
# what a program is drawn from (shuffled): 28 ops
MIX = (["frame"] * 4 + ["step"] * 3 + ["delete"] * 2 + ["cut"] * 4 + ["add"] * 6 + ["reset"] * 2 + ["checkpoint"] * 2
       + ["fork map", "fork swap", "fork broadcast", "add dry", "cut dry"])


def oracle_module():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if os.path.join(root, "oracle") not in sys.path:
        sys.path.insert(0, os.path.join(root, "oracle"))
    import oracle
    return oracle


def scatter(sb, particles, beams, rng):
    """the scene with sparse, shuffled mappings: particle and beam slots and data indices are independent draws"""
    maxP, maxB = CAP
    P, B = len(particles), len(beams)
    D, S = rng.permutation(maxP)[:P], rng.permutation(P)
    E, T = rng.permutation(maxB)[:B], rng.permutation(B)
    buf = sb.Buffers(LAYOUT, maxP, maxB)
    buf.particles[D, :particles.shape[1]] = particles
    buf.mapping[S] = D
    rec = beams.copy()
    rec["a"], rec["b"] = D[beams["a"].astype(np.int64)], D[beams["b"].astype(np.int64)]
    buf.beams[E] = rec
    buf.mapping[maxP + T] = E
    buf.particle_count, buf.beam_count = P, B
    return buf


def body(sb, ox, oy, w, h, base=0, v=(0.0, 0.0)):
    p, b = sb.scenes.rectangle(ox, oy, 30.0, w, h, *MAT, base=base, layout=LAYOUT)
    pv = np.zeros((len(p), 6), F)
    pv[:, :2], pv[:, 2:4] = p, v
    return pv, b


def scenes(sb, rng):
    def one(*a, **k):
        return scatter(sb, *body(sb, *a, **k), rng)

    def two(w1, h1, w2, h2):    # two bodies whose facing columns are 15 apart: they touch
        p1, b1 = body(sb, 300.0, 300.0, w1, h1)
        p2, b2 = body(sb, 300.0 + 30.0 * (w1 - 1) + 15.0, 300.0, w2, h2, base=len(p1))
        return scatter(sb, np.concatenate([p1, p2]), np.concatenate([b1, b2]), rng)

    free = np.zeros((10, 6), F)
    free[:, 0], free[:, 1] = 400.0 + 35.0 * (np.arange(10) % 5), 500.0 + 35.0 * (np.arange(10) // 5)
    p, b = body(sb, 500.0, 200.0, 6, 5)                         # 89 beams, and seven to the second neighbour in y: 96 of 96
    extra = np.zeros(CAP[1] - len(b), b.dtype)
    idx = np.asarray([i for i in range(30) if i % 5 < 3][:len(extra)])
    extra["a"], extra["b"] = idx, idx + 2
    for f, val in zip(("length", "target_length", "last_length", "spring", "damp", "yield_strain", "strain_break_limit"), (60.0, 60.0, 60.0) + MAT):
        extra[f] = val
    full = scatter(sb, p, np.concatenate([b, extra]), rng)
    assert full.beam_count == CAP[1]
    return [one(200.0, 200.0, 4, 4), one(600.0, 400.0, 3, 3, v=(2.0, -3.0)), one(100.0, 600.0, 5, 4), two(2, 2, 2, 2), two(3, 2, 2, 3),
            scatter(sb, free, np.zeros(0, b.dtype), rng), None, full, one(700.0, 700.0, 4, 3, v=(-4.0, 0.0)), one(300.0, 100.0, 3, 4),
            one(100.0, 100.0, 2, 5, v=(1.0, 1.0)), one(500.0, 500.0, 4, 4, v=(0.0, -6.0))]


def make_models(sb, bufs, cls=model.SceneModel):
    events = {}
    return [cls(oracle_module(), b, LAYOUT, CAP, events=events) for b in bufs]


def draw_rows(m, k, flags, rng):
    """k rows for one scene: mostly pairs of its particles, at 0.95 .. 1.05 of their distance unless LENGTH_CURRENT; now and then an
    empty row, an invalid row, a repeated pair; the rows behind a random count are empty"""
    rows = [(-1, -1, 0.0, 0.0, 0.0, 0.0, 0.0)] * k
    n = int(rng.integers(1, k + 1)) if rng.random() < 0.6 else k
    if not m.loaded:
        return add_ref.pack([(int(rng.integers(-2, CAP[0] + 2)), int(rng.integers(0, CAP[0])), 10.0) + MAT for _ in range(k)])
    buf = m.current()
    pidx = [int(d) for d in buf.mapping[:buf.particle_count]]
    pairs = []
    for j in range(n):
        u = rng.random()
        if u < 0.04:
            rows[j] = (-1 - j, 3, 10.0) + MAT
            continue
        if u < 0.08:
            a = pidx[int(rng.integers(len(pidx)))]
            rows[j] = [(a, a, 10.0) + MAT, (CAP[0] + 1, a, 10.0) + MAT, (a, pidx[0] if pidx[0] != a else pidx[1], -1.0) + MAT][int(rng.integers(3))]
            if flags & add_ref.LENGTH_CURRENT and rows[j][2] < 0:
                rows[j] = (a, a, 10.0) + MAT
            continue
        if u < 0.16 and pairs:
            a, b = pairs[int(rng.integers(len(pairs)))][::-1 if rng.random() < 0.5 else 1]
        else:
            a, b = (pidx[int(i)] for i in rng.choice(len(pidx), 2, replace=False))
        pairs.append((a, b))
        length = 0.0 if flags & add_ref.LENGTH_CURRENT else float(add_ref.distance(buf.particles[a], buf.particles[b])) * (0.95 + 0.1 * rng.random())
        rows[j] = (a, b, length) + MAT
    return add_ref.pack(rows)


def draw_shapes(m, rng):
    """three shapes for one scene: one to three strokes and discs through the inside of its particles' box, CUT_NONE behind them; one
    scene in four gets CUT_NONE only"""
    out = np.zeros((3, 8), np.uint32)
    if m.loaded and rng.random() < 0.25:
        return out
    x0, y0, x1, y1 = 100.0, 100.0, 400.0, 400.0
    if m.loaded and m.current().particle_count:
        buf = m.current()
        p = buf.particles[buf.mapping[:buf.particle_count].astype(np.int64), :2]
        x0, y0, x1, y1 = (float(v) for v in (p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()))
    rows = []
    for _ in range(int(rng.integers(1, 4))):
        cx, cy = x0 + (x1 - x0) * rng.uniform(0.2, 0.8), y0 + (y1 - y0) * rng.uniform(0.2, 0.8)
        if rng.random() < 0.5:
            t, half = rng.uniform(0, np.pi), rng.uniform(0.1, 0.25) * max(x1 - x0, y1 - y0, 30.0)
            rows.append((cut_ref.SEGMENT, cx - half * np.cos(t), cy - half * np.sin(t), cx + half * np.cos(t), cy + half * np.sin(t)))
        else:
            rows.append((cut_ref.DISC, cx, cy, rng.uniform(4.0, 12.0), 0.0))
    sh = cut_ref.pack(rows)
    out[:len(sh)] = sh
    return out


def draw_op(name, models, rng):
    if name == "frame":
        return ("frame", 1)
    if name == "step":
        return ("step", int(rng.integers(1, 21)))
    if name == "delete":
        return ("delete",)
    if name in ("cut", "cut dry"):
        return ("cut", np.stack([draw_shapes(m, rng) for m in models]), name == "cut dry")
    if name in ("add", "add dry"):
        k = 64 if rng.random() < 0.4 else int(rng.integers(1, 65))
        flags = (add_ref.LENGTH_CURRENT if rng.random() < 0.4 else 0) | (add_ref.SKIP_JOINED if rng.random() < 0.5 else 0)
        return ("add", np.stack([draw_rows(m, k, flags, rng) for m in models]), flags, name == "add dry")
    if name in ("reset", "checkpoint"):
        mask = (rng.random(N) < 0.4).astype(np.uint8)
        mask[int(rng.integers(N))] = 1
        return (name, mask)
    src = np.full(N, model.KEEP, np.int32)
    others = [i for i in range(N) if i != NEVER]
    if name == "fork map":
        for i in others:
            if rng.random() < 0.5:
                src[i] = int(rng.integers(N))
    elif name == "fork swap":
        i, j = (others[int(x)] for x in rng.choice(len(others), 2, replace=False))
        src[i], src[j] = j, i
    else:
        s = others[int(rng.integers(len(others)))]
        for i in rng.choice(others, 4, replace=False):
            src[int(i)] = s
    return ("fork", src, bool(rng.random() < 0.5), name.split()[1])


@functools.lru_cache(maxsize=None)
def _program(sb, seed):
    rng = np.random.default_rng(7000 + seed)
    bufs = scenes(sb, rng)
    models = make_models(sb, bufs)
    ops = []
    for name in rng.permutation(MIX):
        op = draw_op(str(name), models, rng)
        model.apply(models, op)
        ops.append(op)
    return bufs, ops


def program(sb, seed):
    """(the twelve scenes to upload -- None: never uploaded --, the ops)"""
    return _program(sb, seed)
