"""A host model of ONE scene of a BatchEngine under the eight editing calls -- step, delete_pass, frame, cut, add_beams, reset,
checkpoint, fork -- built from what the suite already has: the oracle steps and deletes, tests/cut_ref.py says what a cut hits,
tests/batch_add_beams_ref.py what an add writes, layout.Buffers holds what load_scene returns.  Nothing of a kernel: no blobs, no
bitmaps, no ranks.

The current state is an oracle engine; its `delete` words are the pending flags (bit max_particles + slot).  The reset state is a
second engine in the state the latest upload, checkpoint or fork left.  Words 12 .. 27 of the metadata (physics constants, user
input) belong to the scene's place in the batch: a reset and a fork leave them.  `exists` is the set of beam data indices that an
upload or an add ever gave a beam (such an index, when not alive, reads "removed" in summary()).

The model also keeps a few counters of what happened to it (`events`), which tests/test_batch_edit_model_cpu.py asserts on."""
import numpy as np

import batch_add_beams_ref as add_ref
import cut_ref

ALLPAIRS = 1
KEEP = -1
ARRAYS = ("metadata", "mapping", "particles_a", "particles_b", "beams", "forces", "delete")


def clone(eng):
    new = type(eng).__new__(type(eng))
    new.__dict__.update(eng.__dict__)
    for k in ARRAYS:
        setattr(new, k, getattr(eng, k).copy())
    return new


class SceneModel:
    def __init__(self, orc, buf, layout, cap, subticks=64, events=None):
        self.layout, self.cap = layout, cap
        self.events = {} if events is None else events          # (shared by the scenes of a batch)
        self.own = np.zeros(16, "<u4")
        self.eng = self.rst = self.template = None
        self.last_full = None
        if buf is not None:
            self.eng = orc.OracleEngine(1000.0, 10.0, subticks, layout, ALLPAIRS, threads=2)
            self.eng.write_buffers(buf)
            self.own = buf.metadata[12:28].copy()
            self.template = buf.copy()                          # what load_scene is given to write into
            self.exists = add_ref.alive_set(buf)
            self.exact = True                                   # rows no live slot names are still those of `template`
            self.welds, self.removed = set(), set()             # live beams an add made; indices a delete pass removed
            self.unsaved_adds, self.welded = 0, False
            self.checkpoint()

    # ---- reading
    @property
    def loaded(self):
        return self.eng is not None

    def current(self, eng=None):
        return (eng or self.eng).load_buffers(self.template.copy())

    def pending_slots(self, eng=None):
        eng = eng or self.eng
        maxP, nb = self.cap[0], int(eng.metadata[6])
        bits = maxP + np.arange(nb)
        return np.flatnonzero((eng.delete[bits >> 5] >> (bits & 31).astype(np.uint32)) & 1)

    def observe(self):
        """(the scene as load_scene gives it -- None: never uploaded --, summary()'s words 1, 2, 3: beams, removed, pending)"""
        if not self.loaded:
            return None, (0, 0, 0)
        buf = self.current()
        return buf, (buf.beam_count, int(self.exists.sum()) - int(add_ref.alive_set(buf).sum()), len(self.pending_slots()))

    def note(self, what):
        self.events[what] = self.events.get(what, 0) + 1

    # ---- the oracle's
    def step(self, n):
        if self.loaded:
            self.eng.step(n)

    def delete_pass(self):
        if not self.loaded:
            return
        before = add_ref.alive_set(self.current())
        self.eng.delete_pass()
        gone = set(np.flatnonzero(before & ~add_ref.alive_set(self.current())).tolist())
        if gone & self.welds:
            self.note("weld removed by a delete pass")
        self.welds -= gone
        self.removed |= gone

    def frame(self, n=1):
        for _ in range(n):
            self.step(self.eng.subticks if self.loaded else 0)
            self.delete_pass()

    # ---- cut: cut_ref on the buffers as loaded; the hit slots' delete bits are raised
    def cut(self, shapes, dry=False):
        maxP, maxB = self.cap
        if not self.loaded:
            return np.zeros(maxB, np.uint8), [0, 0, 0, 0]
        buf = self.current()
        live = buf.mapping[maxP:maxP + buf.beam_count].astype(np.int64)
        pending = np.zeros(maxB, bool)
        pending[live[self.pending_slots()]] = True
        hit, counts = cut_ref.scene_ref(buf, shapes, pending=pending, dry=dry)
        if not dry:
            for s in np.flatnonzero(hit[live]):
                bit = maxP + int(s)
                self.eng.delete[bit >> 5] |= np.uint32(1 << (bit & 31))
        return hit, counts

    # ---- add: add_ref on the buffers as loaded, with the reset state's alive set
    def reset_alive(self):
        return add_ref.alive_set(self.current(self.rst))

    def new_slot_bits(self, slots):
        for s in slots:
            bit = self.cap[0] + int(s)
            self.eng.delete[bit >> 5] &= ~np.uint32(1 << (bit & 31))

    def add(self, rows, flags=0, dry=False):
        self.last_full = None
        if not self.loaded:
            _, res, cnt = add_ref.add_ref(None, rows, flags)
            return res, cnt
        buf = self.current()
        ra = self.reset_alive()
        edited, res, cnt = add_ref.add_ref(buf, rows, flags, ra)
        full = np.flatnonzero(res == add_ref.FULL)
        if full.size:      # which half of `Bc + added < max_beams and added < len(free)` refused first
            added = int((res[:full[0]] >= 0).sum())
            n_free = int((~add_ref.alive_set(buf) & ~(ra if ra is not None else False)).sum())
            room, index = buf.beam_count + added < buf.max_beams, added < n_free
            assert not (room and index) and (room or not index), "(no slot left means no index left: the alive indices are as many as the slots)"
            self.last_full = "index" if room else "room"
        if dry:
            return res, cnt
        new = [int(d) for d in res if d >= 0]
        if new:
            if self.rst_from_fork:
                self.note("add into a scene whose reset state came from a fork")
            if set(new) & self.rst_removed:
                self.note("a removed index handed out again after a checkpoint")
            self.eng.beams[:], self.eng.mapping[:], self.eng.metadata[:] = edited.beams, edited.mapping, edited.metadata
            self.new_slot_bits(range(buf.beam_count, edited.beam_count))
            self.exists[new] = True
            self.welds |= set(new)
            self.removed -= set(new)
            self.unsaved_adds += len(new)
            self.welded = True
        return res, cnt

    # ---- reset and checkpoint: copy the one state over the other
    def reset(self):
        if not self.loaded:
            return
        if self.unsaved_adds:
            self.note("reset after an add")
        self.eng = clone(self.rst)
        self.eng.metadata[12:28] = self.own
        self.welds, self.removed, self.unsaved_adds = set(self.rst_welds), set(self.rst_removed_all), 0
        if getattr(self, "welded", False):
            self.exact = False       # (an index whose add a reset undid exports the add's material beside the reset state's beam state)

    def checkpoint(self):
        if not self.loaded:
            return
        self.rst = clone(self.eng)
        self.rst_welds, self.rst_removed_all, self.rst_removed = set(self.welds), set(self.removed), set(self.removed)
        self.unsaved_adds, self.rst_from_fork = 0, False

    # ---- fork
    def snapshot(self):
        """everything a fork copies, as it is before the call"""
        s = dict(self.__dict__)
        if self.loaded:
            s["eng"], s["rst"] = clone(self.eng), clone(self.rst)
            for k in ("exists", "welds", "removed", "rst_welds", "rst_removed_all", "rst_removed"):
                s[k] = s[k].copy()
        return s

    def fork_reset(self, src, as_reset):
        """the reset engine after a fork from the snapshot `src`"""
        return clone(self.eng) if as_reset else clone(src["rst"])

    def fork_from(self, src, as_reset=False):
        """src: another scene's snapshot()"""
        own, events = self.own, self.events
        had = dict(self.__dict__)
        self.__dict__.update({k: (v.copy() if isinstance(v, (set, np.ndarray)) else v) for k, v in src.items()})
        self.own, self.events, self.last_full = own, events, None
        if src["eng"] is None:
            self.eng = self.rst = self.template = None
            return
        if len(self.pending_slots(src["eng"])):
            self.note("fork of a scene with pending flags")
        self.eng = clone(src["eng"])
        self.eng.metadata[12:28] = own
        self._had = had
        self.rst = self.fork_reset(src, as_reset)
        del self._had
        self.rst.metadata[12:28] = own
        self.rst_from_fork = True
        if as_reset:
            self.rst_welds, self.rst_removed_all, self.rst_removed, self.unsaved_adds = set(self.welds), set(self.removed), set(), 0
        else:
            self.rst_removed = set()     # (only a checkpoint of this scene's own counts for "after a checkpoint")


# ---------------------------------------------------------------- a batch of models, and the comparison with a batch

def kind(op):
    if op[0] == "fork":
        return "fork " + op[3]
    if op[0] in ("cut", "add") and op[-1]:
        return op[0] + " dry"
    return op[0]


def changes_state(op):
    return not (op[0] in ("cut", "add") and op[-1])


def apply(models, op):
    """One batch-wide op on the models; returns the tensors the batch's call returns, stacked over the scenes."""
    k = op[0]
    if k == "frame":
        for m in models:
            m.frame(op[1])
    elif k == "step":
        for m in models:
            m.step(op[1])
    elif k == "delete":
        for m in models:
            m.delete_pass()
    elif k == "cut":
        out = [m.cut(op[1][i], dry=op[2]) for i, m in enumerate(models)]
        return dict(hit=np.stack([o[0] for o in out]), counts=np.asarray([o[1] for o in out], np.int32))
    elif k == "add":
        out = [m.add(op[1][i], op[2], dry=op[3]) for i, m in enumerate(models)]
        return dict(result=np.stack([o[0] for o in out]), counts=np.asarray([o[1] for o in out], np.int32))
    elif k in ("reset", "checkpoint"):
        for m, bit in zip(models, op[1]):
            if bit:
                getattr(m, k)()
    elif k == "fork":
        snaps = [m.snapshot() for m in models]
        for i, s in enumerate(op[1]):
            s = int(s)
            if 0 <= s < len(models) and s != i:
                models[i].fork_from(snaps[s], as_reset=op[2])
    else:
        raise ValueError(op)
    return {}


def summary_words(models):
    return np.asarray([m.observe()[1] for m in models], np.float32)


def live_part(buf):
    maxP, P, B = buf.max_particles, buf.particle_count, buf.beam_count
    pm, bm = buf.mapping[:P].astype(np.int64), buf.mapping[maxP:maxP + B].astype(np.int64)
    return dict(counts=(P, B), metadata=buf.metadata.tobytes(), particle_mapping=pm.tolist(), beam_mapping=bm.tolist(),
                particles=buf.particles[pm].tobytes(), beams=buf.beams[bm].tobytes())


def scene_difference(got, want, exact):
    """None, or what differs between two read-backs of a scene: counts, metadata, the live part of both mappings, every particle
    row and beam record at a live data index; with `exact` the whole mapping, particle and beam buffers as well."""
    a, b = live_part(got), live_part(want)
    for k in a:
        if a[k] != b[k]:
            return k
    if exact:
        for k in ("mapping", "particles", "beams"):
            if getattr(got, k).tobytes() != getattr(want, k).tobytes():
                return "whole " + k
    return None


def outputs_difference(got, want):
    """None, or the name of the first returned tensor that differs (by its bits)"""
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in sorted(want):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.shape != w.shape or g.tobytes() != w.astype(g.dtype).tobytes():
            return k
    return None
