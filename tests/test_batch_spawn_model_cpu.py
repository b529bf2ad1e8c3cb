"""The spawn programs of tests/batch_spawn_model.py on the host model alone, without a GPU: the conditions that make
tests/test_gpu_batch_spawn_program.py meaningful -- finite throughout, every op kind over the nine editing calls, every row code of
a spawn, a spawn that a reset undoes, a weld onto a spawned particle, a fork of a scene with an unsaved spawn --, the model against
the hand-made reset episodes of tests/test_gpu_batch_add_particles.py, and two deliberately wrong models, each of which the
comparison of the GPU test catches inside a program."""
import numpy as np
import pytest

import batch_add_beams_ref as beam_ref
import batch_add_particles_cases as spawn_cases
import batch_add_particles_ref as ref
import batch_edit_model as model
import batch_spawn_model as spawn


def run(sb, seed, cls=spawn.SpawnModel, watch=None):
    bufs, ops = spawn.program(sb, seed)
    models = spawn.make_models(sb, bufs, cls)
    for k, op in enumerate(ops):
        out = spawn.apply(models, op)
        if watch:
            watch(k, op, models, out)
    return models


@pytest.fixture(scope="module")
def traces(sb):
    out = {}
    for seed in spawn.SEEDS:
        t = dict(kinds=[], codes=set(), finite=True, invariant=True, most=0)

        def watch(k, op, models, res, t=t):
            t["kinds"].append(spawn.kind(op))
            if op[0] == "spawn":
                t["codes"] |= {min(int(c), 0) for c in res["result"].ravel()}
                t["most"] = max(t["most"], int(res["counts"][:, 0].max()))
            for m in models:
                if m.loaded:
                    buf = m.current()
                    t["finite"] &= bool(np.isfinite(buf.particles[buf.mapping[:buf.particle_count].astype(np.int64)]).all())
                    # pex[d] == 1 iff a slot < P names d, the engine's mapping is the constant one, P0 <= P
                    t["invariant"] &= bool(np.array_equal(m.pex, ref.held(buf)) and np.array_equal(buf.mapping[:m.cap[0]], m.pmap) and m.P0 <= m.P)

        models = run(sb, seed, watch=watch)
        t["events"] = models[0].events
        out[seed] = t
    return out


def test_programs_stay_finite_and_keep_the_invariant(traces):
    assert all(t["finite"] for t in traces.values()) and all(t["invariant"] for t in traces.values())


def test_every_op_kind_and_row_code(traces):
    kinds = sum((t["kinds"] for t in traces.values()), [])
    assert set(kinds) == set(spawn.OP_KINDS) and all(len(t["kinds"]) == len(spawn.MIX) for t in traces.values())
    assert kinds.count("spawn") == 4 * len(spawn.SEEDS) and kinds.count("spawn dry") == len(spawn.SEEDS)
    codes = set().union(*(t["codes"] for t in traces.values()))
    assert codes == {0, ref.EMPTY, ref.INVALID, ref.BLOCKED, ref.FULL}
    assert max(t["most"] for t in traces.values()) >= 8, "a wide spawn"


@pytest.mark.parametrize("what", ["spawn", "reset undoes a spawn", "weld onto a spawned particle", "fork of a scene with an unsaved spawn",
                                  "reset after an add"])
def test_the_programs_reach(traces, what):
    print({seed: t["events"] for seed, t in traces.items()})
    assert sum(t["events"].get(what, 0) for t in traces.values()) >= 1


def test_model_replays_the_reset_episodes(sb, oracle):
    """test_reset_removes_the_particle_and_its_weld, on the model: three spawn - weld - reset episodes in a scene with one free slot"""
    case = spawn_cases.one_free_case(sb)
    m = spawn.SpawnModel(oracle, case["bufs"][0], case["layout"], case["cap"])
    for _ in range(3):
        res, cnt = m.add_particles(case["rows"][0])
        assert res.tolist() == [16] and cnt == [1, 0, 0, 0] and m.particles() == 17
        wres, wcnt = m.add(beam_ref.pack([(16, 3, 0.0) + spawn_cases.MAT]), beam_ref.LENGTH_CURRENT)
        assert wres.tolist() == [42] and wcnt == [1, 0, 0, 0] and m.observe()[1] == (43, 0, 0)
        m.frame()
        m.reset()
        assert m.particles() == 16 and m.observe()[1] == (42, 1, 0) and not m.pex[16]
    assert m.add_particles(np.concatenate([case["rows"][0]] * 2))[0].tolist() == [16, ref.FULL]
    m.checkpoint()
    m.frame(2)
    m.reset()
    assert m.particles() == 17 and m.add_particles(case["rows"][0])[0].tolist() == [ref.FULL]
    assert m.events["reset undoes a spawn"] == 3 and m.events["weld onto a spawned particle"] == 3


# ---------------------------------------------------------------- deliberately wrong models

class ResetKeepsP(spawn.SpawnModel):
    """a reset that copies the reset state but leaves the particle count where it was"""
    def count_after_reset(self, p, p0):
        return p


class ResetKeepsBytes(spawn.SpawnModel):
    """a reset that lowers P but forgets to clear the "holds a particle" bytes: the indices leak"""
    def clear_bytes(self, indices):
        pass


@pytest.mark.parametrize("wrong", [ResetKeepsP, ResetKeepsBytes])
def test_the_program_catches_a_wrong_model(sb, wrong):
    """the comparison of tests/test_gpu_batch_spawn_program.py, with the wrong model in the batch's place"""
    caught = {}
    for seed in spawn.SEEDS:
        bufs, ops = spawn.program(sb, seed)
        good, bad = spawn.make_models(sb, bufs), spawn.make_models(sb, bufs, wrong)
        for k, op in enumerate(ops):
            try:
                want, got = spawn.apply(good, op), spawn.apply(bad, op)
            except Exception as e:       # (a wrong model may leave the ground the restatements stand on)
                caught[seed] = (k, spawn.kind(op), "raised " + type(e).__name__)
                break
            got["summary"], want["summary"] = spawn.summary_words(bad), spawn.summary_words(good)
            diff = model.outputs_difference(got, want)
            for g, w in zip(bad, good):
                if diff is None and g.loaded and w.loaded:
                    diff = model.scene_difference(g.current(), w.current(), False)
            if diff is not None:
                caught[seed] = (k, spawn.kind(op), diff)
                break
    print(wrong.__name__, caught)
    assert caught, "no program tells %s from the model" % wrong.__name__
