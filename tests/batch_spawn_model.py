"""The host model of tests/batch_edit_model.py with the ninth editing call, add_particles, and seeded programs over all nine: a
subclass of SceneModel, not an edit of it.  What the batch keeps in its constant blob -- the particle mapping, which only grows at
its end, and the "holds a particle" bytes -- the model keeps beside the oracle engine (`pmap`, `pex`): a reset takes the engine
back to the reset state but leaves the mapping, clears the bytes of the slots P0 .. P - 1 and lowers P to P0, the particle count of
the reset engine.  tests/batch_add_particles_ref.py says what an add writes.

The programs are batch_edit_cases' (the same twelve scenes, the same draws of the other ops) with spawns mixed in; the generator
runs the model while it draws.  tests/test_batch_spawn_model_cpu.py runs them on the model alone."""
import functools

import numpy as np

import batch_add_particles_ref as spawn_ref
import batch_edit_cases as edit_cases
import batch_edit_model as model

F = np.float32
CAP, LAYOUT, N, SEEDS = edit_cases.CAP, edit_cases.LAYOUT, edit_cases.N, (1, 2, 3)
OP_KINDS = edit_cases.OP_KINDS + ("spawn", "spawn dry")
# what a program is drawn from (shuffled): 33 ops
MIX = list(edit_cases.MIX) + ["spawn"] * 4 + ["spawn dry"]


class SpawnModel(model.SceneModel):
    def __init__(self, orc, buf, layout, cap, subticks=64, events=None):
        super().__init__(orc, buf, layout, cap, subticks, events)
        self.pmap = self.pex = None
        if buf is not None:
            self.pmap = buf.mapping[:cap[0]].copy()          # the constant blob's particle mapping, every entry
            self.pex = spawn_ref.held(buf)                   # "holds a particle" by data index

    # ---- reading
    @property
    def P(self):
        return int(self.eng.metadata[1])

    @property
    def P0(self):
        return int(self.rst.metadata[1])

    def particles(self):
        return self.P if self.loaded else 0

    def spawned_now(self):
        """the data indices of the slots P0 .. P - 1: what a reset would remove"""
        return set(int(d) for d in self.pmap[self.P0:self.P]) if self.loaded else set()

    # ---- add_particles: the restatement on the buffers as loaded, with the model's own bytes
    def add_particles(self, rows, flags=0, dry=False):
        if not self.loaded:
            _, res, cnt = spawn_ref.add_ref(None, rows, flags)
            return res, cnt
        buf = self.current()
        edited, res, cnt = spawn_ref.add_ref(buf, rows, flags, holds=self.pex)
        new = [int(d) for d in res if d >= 0]
        if dry or not new:
            return res, cnt
        now = self.eng.particles_b if self.eng.final_in_b else self.eng.particles_a
        now[new] = edited.particles[new]
        self.eng.mapping[:], self.eng.metadata[:] = edited.mapping, edited.metadata
        self.pmap = edited.mapping[:self.cap[0]].copy()
        self.pex[new] = True
        self.note("spawn")
        return res, cnt

    # ---- add_beams: the base model's; a weld onto a particle that a reset would remove is counted
    def add(self, rows, flags=0, dry=False):
        res, cnt = super().add(rows, flags, dry)
        if self.loaded and not dry:
            young = self.spawned_now()
            for d in res[res >= 0]:
                if {int(self.eng.beams["a"][d]), int(self.eng.beams["b"][d])} & young:
                    self.note("weld onto a spawned particle")
        return res, cnt

    # ---- reset: the base model's, then what the constant blob keeps
    def clear_bytes(self, indices):
        self.pex[list(indices)] = False

    def count_after_reset(self, p, p0):
        return p0

    def reset(self):
        if not self.loaded:
            return
        p, p0 = self.P, self.P0
        if p > p0:
            self.note("reset undoes a spawn")
            self.clear_bytes(int(d) for d in self.pmap[p0:p])
        super().reset()
        self.eng.mapping[:self.cap[0]] = self.pmap
        self.eng.metadata[1] = self.count_after_reset(p, p0)

    def fork_from(self, src, as_reset=False):
        super().fork_from(src, as_reset)
        if self.loaded and self.P > self.P0:
            self.note("fork of a scene with an unsaved spawn")


# ---------------------------------------------------------------- programs

def make_models(sb, bufs, cls=SpawnModel):
    return edit_cases.make_models(sb, bufs, cls)


def draw_spawn_rows(m, k, rng):
    """k rows for one scene: positions drawn in the box, now and then beside a particle of the scene or beside an earlier row (what
    SKIP_TOUCHING refuses), an empty row, an invalid row; small velocities; the rows behind a random count are empty"""
    rows = [(-1, 0.0, 0.0)] * k
    n = int(rng.integers(1, k + 1))
    here = None
    if m.loaded and m.current().particle_count:
        buf = m.current()
        here = buf.particles[buf.mapping[:buf.particle_count].astype(np.int64), :2]
    made = []
    for j in range(n):
        u = rng.random()
        if u < 0.06:
            rows[j] = (-2 - j, 100.0, 100.0)
            continue
        if u < 0.12:
            rows[j] = [(0, float("nan"), 100.0), (0, 100.0, float("inf")), (0, 100.0, 100.0, 0, 0, 0, 0, 3)][int(rng.integers(3))]
            continue
        if u < 0.22 and here is not None:
            x, y = here[int(rng.integers(len(here)))] + rng.uniform(-12.0, 12.0, 2)
        elif u < 0.32 and made:
            x, y = np.asarray(made[int(rng.integers(len(made)))]) + rng.uniform(-12.0, 12.0, 2)
        else:
            x, y = rng.uniform(40.0, 960.0, 2)
        made.append((float(x), float(y)))
        rows[j] = (j, float(x), float(y), *(float(v) for v in rng.normal(size=2) * 2.0))
    return spawn_ref.pack(rows)


def draw_op(name, models, rng):
    if name in ("spawn", "spawn dry"):
        k = 64 if rng.random() < 0.15 else int(rng.integers(1, 9))
        flags = spawn_ref.SKIP_TOUCHING if rng.random() < 0.6 else 0
        return ("spawn", np.stack([draw_spawn_rows(m, k, rng) for m in models]), flags, name == "spawn dry")
    return edit_cases.draw_op(name, models, rng)


def kind(op):
    if op[0] == "spawn":
        return "spawn dry" if op[-1] else "spawn"
    return model.kind(op)


def changes_state(op):
    return not (op[0] in ("cut", "add", "spawn") and op[-1])


def apply(models, op):
    """One batch-wide op on the models; returns the tensors the batch's call returns, stacked over the scenes."""
    if op[0] == "spawn":
        out = [m.add_particles(op[1][i], op[2], dry=op[3]) for i, m in enumerate(models)]
        return dict(result=np.stack([o[0] for o in out]), counts=np.asarray([o[1] for o in out], np.int32))
    return model.apply(models, op)


def summary_words(models):
    """summary()'s words 0 .. 3: particles, beams, removed, pending"""
    return np.asarray([(m.particles(),) + tuple(m.observe()[1]) for m in models], np.float32)


@functools.lru_cache(maxsize=None)
def _program(sb, seed):
    rng = np.random.default_rng(9000 + seed)
    bufs = edit_cases.scenes(sb, rng)
    models = make_models(sb, bufs)
    ops = []
    for name in rng.permutation(MIX):
        op = draw_op(str(name), models, rng)
        apply(models, op)
        ops.append(op)
    return bufs, ops


def program(sb, seed):
    """(the twelve scenes to upload -- None: never uploaded --, the ops)"""
    return _program(sb, seed)
