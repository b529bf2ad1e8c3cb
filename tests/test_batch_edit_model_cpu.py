"""The edit programs of tests/batch_edit_cases.py on the host model alone (tests/batch_edit_model.py), without a GPU: the conditions
that make tests/test_gpu_batch_edit_program.py meaningful -- finite throughout, every op kind and row code, both halves of FULL, a
weld removed, an index reused after a checkpoint, forks of pending flags, resets after adds, adds behind a fork --, the model
against the literal results of the hand-made compositions of tests/test_gpu_batch_add_beams.py, and three deliberately wrong
models, each of which the comparison of the GPU test catches inside a program."""
import numpy as np
import pytest

import batch_add_beams_cases as add_cases
import batch_add_beams_ref as ref
import batch_edit_cases as cases
import batch_edit_model as model


def run(sb, seed, cls=model.SceneModel, watch=None):
    """the program on fresh models; watch(k, op, models, outputs) after every op"""
    bufs, ops = cases.program(sb, seed)
    models = cases.make_models(sb, bufs, cls)
    for k, op in enumerate(ops):
        out = model.apply(models, op)
        if watch:
            watch(k, op, models, out)
    return models


@pytest.fixture(scope="module")
def traces(sb):
    """per seed: what the conditions below look at"""
    out = {}
    for seed in cases.SEEDS:
        t = dict(kinds=[], codes=set(), full=set(), words=0, finite=True, stale=False)

        def watch(k, op, models, res, t=t):
            t["kinds"].append(model.kind(op))
            if op[0] == "add":
                t["codes"] |= {min(int(c), 0) for c in res["result"].ravel()}
                t["full"] |= {m.last_full for m in models if m.last_full}
                if not op[3]:
                    for m, c in zip(models, res["counts"]):
                        if m.loaded and c[0]:
                            bc = m.current().beam_count
                            t["words"] = max(t["words"], ((bc - 1) >> 5) - ((bc - int(c[0])) >> 5) + 1)
            for m in models:
                if m.loaded:
                    buf = m.current()
                    t["finite"] &= bool(np.isfinite(buf.particles[buf.mapping[:buf.particle_count].astype(np.int64)]).all())
                    bits = np.unpackbits(m.eng.delete.view(np.uint8), bitorder="little")
                    t["stale"] |= bool(bits[:m.cap[0]].any() or bits[m.cap[0] + buf.beam_count:].any())

        models = run(sb, seed, watch=watch)
        t["events"] = models[0].events
        out[seed] = t
    return out


def test_programs_stay_finite(traces):
    """the generator, not a tolerance, keeps the cases finite: NaN bits are outside the parity contract"""
    assert all(t["finite"] for t in traces.values())


def test_no_pending_bit_outside_the_live_slots(traces):
    """Why `add_beams` clearing the bits of its new slots cannot be seen to matter through legal calls: no call leaves a raised bit at
    or past the live count -- a delete pass zeroes every word, reset, checkpoint and fork carry the words with their count."""
    assert not any(t["stale"] for t in traces.values())


def test_every_op_kind_and_row_code(traces):
    kinds = sum((t["kinds"] for t in traces.values()), [])
    for k in cases.OP_KINDS:
        assert kinds.count(k) >= 3, k
    assert set(kinds) == set(cases.OP_KINDS)
    codes = set().union(*(t["codes"] for t in traces.values()))
    assert codes == {0, ref.EMPTY, ref.INVALID, ref.JOINED, ref.FULL}
    full = set().union(*(t["full"] for t in traces.values()))
    assert {"room", "index"} <= full, "FULL from each half of its condition"
    assert max(t["words"] for t in traces.values()) == 3, "a long add crosses three flag words"


@pytest.mark.parametrize("what", ["weld removed by a delete pass", "a removed index handed out again after a checkpoint",
                                  "fork of a scene with pending flags", "reset after an add", "add into a scene whose reset state came from a fork"])
def test_the_programs_reach(traces, what):
    print({seed: t["events"] for seed, t in traces.items()})
    assert sum(t["events"].get(what, 0) for t in traces.values()) >= 1


# ---------------------------------------------------------------- the hand-made compositions of test_gpu_batch_add_beams.py

def sparse_model(sb, oracle):
    case = add_cases.sparse_case(sb)
    return model.SceneModel(oracle, case["bufs"][0], case["layout"], case["cap"]), case["rows"][0], case["bufs"][0]


def disc(x, y, r):
    s = np.zeros((1, 8), np.uint32)
    s[0, 0] = 2
    s[0, 1:4] = np.asarray([x, y, r], "f4").view(np.uint32)
    return s


def test_model_replays_the_literal_results(sb, oracle):
    """test_index_choice_and_flag_words and test_lifecycle, on the model"""
    m, rows, buf = sparse_model(sb, oracle)
    res, cnt = m.add(rows)
    assert res.tolist() == [4, 5, 6, 11, 12] and cnt == [5, 0, 0, 0] and m.observe()[1] == (35, 0, 0)
    first = m.current()
    hit, c = m.cut(disc(260.0, 260.0, 1000.0))
    assert c == [35, 35, 35, 0] and m.observe()[1] == (35, 0, 35)
    m.reset()
    assert m.observe()[1] == (30, 5, 0), "reset: 30 slots, the five indices read removed, no flag"
    res2, _ = m.add(rows)
    assert res2.tolist() == [4, 5, 6, 11, 12] and m.observe()[1] == (35, 0, 0)
    assert model.scene_difference(m.current(), first, True) is None, "the same add after a reset: the same bits"
    m.checkpoint()
    m.frame(2)
    m.reset()
    assert model.scene_difference(m.current(), first, True) is None and m.observe()[1][0] == 35
    # cut -> frame -> add does not reuse the removed index; cut -> frame -> checkpoint -> add does
    for checkpoint, want in ((False, [4, 5, 6, 11, 12]), (True, [3, 4, 5, 6, 11])):
        m, rows, buf = sparse_model(sb, oracle)
        hit, c = m.cut(disc(200.0, 220.0, 1.0))
        assert c == [30, 1, 1, 0] and hit.nonzero()[0].tolist() == [3]
        m.frame()
        if checkpoint:
            m.checkpoint()
        res, cnt = m.add(rows)
        assert res.tolist() == want and m.observe()[1][:2] == (34, 0 if checkpoint else 1)
    # fork of a welded scene copies the weld; fork(as_reset=True), frame, reset keeps it
    a, rows, buf = sparse_model(sb, oracle)
    b, _, _ = sparse_model(sb, oracle)
    assert a.add(rows)[1] == [5, 0, 0, 0] and b.add(np.full_like(rows, -1))[0].tolist() == [ref.EMPTY] * 5
    welded = a.current()
    model.apply([a, b], ("fork", [0, 0], True, "broadcast"))
    assert model.scene_difference(b.current(), welded, True) is None
    b.frame()
    b.reset()
    assert model.scene_difference(b.current(), welded, True) is None and b.observe()[1][0] == 35


# ---------------------------------------------------------------- deliberately wrong models

class BitsNotClear(model.SceneModel):
    """an add after which the pending bits of its new slots are not clear (see test_no_pending_bit_outside_the_live_slots: a bit
    left standing cannot be told from a bit raised)"""
    def new_slot_bits(self, slots):
        for s in slots:
            bit = self.cap[0] + int(s)
            self.eng.delete[bit >> 5] |= np.uint32(1 << (bit & 31))


class FreeIgnoresReset(model.SceneModel):
    """a free-index rule that looks at the current state alone"""
    def reset_alive(self):
        return None


class ForkKeepsReset(model.SceneModel):
    """a fork that leaves the destination's reset state where it was"""
    def fork_reset(self, src, as_reset):
        old = self._had.get("rst")
        return model.clone(old) if old is not None else super().fork_reset(src, as_reset)


@pytest.mark.parametrize("wrong", [BitsNotClear, FreeIgnoresReset, ForkKeepsReset])
def test_the_program_catches_a_wrong_model(sb, wrong):
    """the comparison of tests/test_gpu_batch_edit_program.py, with the wrong model in the batch's place"""
    caught = {}
    for seed in cases.SEEDS:
        bufs, ops = cases.program(sb, seed)
        good, bad = cases.make_models(sb, bufs), cases.make_models(sb, bufs, wrong)
        for k, op in enumerate(ops):
            try:
                want, got = model.apply(good, op), model.apply(bad, op)
            except Exception as e:       # (a wrong model may leave the ground the restatements stand on)
                caught[seed] = (k, model.kind(op), "raised " + type(e).__name__)
                break
            got["summary"], want["summary"] = model.summary_words(bad), model.summary_words(good)
            diff = model.outputs_difference(got, want)
            for i, (g, w) in enumerate(zip(bad, good)):
                if diff is None and g.loaded and w.loaded:
                    diff = model.scene_difference(g.current(), w.current(), False)
                elif diff is None and g.loaded != w.loaded:
                    diff = "loaded"
            if diff is not None:
                caught[seed] = (k, model.kind(op), diff)
                break
    print(wrong.__name__, caught)
    assert caught, "no program tells %s from the model" % wrong.__name__
