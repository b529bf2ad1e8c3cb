"""The scenarios of tests/test_gpu_state_io_halves.py as scripts over the numpy model of the blocked beam-state store
(tests/state_io_model.py), run on the model and on each of its mutants: which of the writes of the beam import, the checkpoint and the
restore does which scenario notice, and on which half of the double buffers.

A script is a list of steps -- launch, reach (one or two launches, to a given half), import, checkpoint, restore -- with `read` where
the device test reads back.  A mutant is KILLED by a script when one of its reads differs from the model's.  A script "stays on half 0"
when every import, checkpoint and restore in it is issued while half 0 is current: what the suite did before these tests, by chance
(a fresh upload, or whole frames of an even number of launches).

(Case e of the device tests, the particle import, is not a script here: the model holds no per-particle state.  Its flag row is
single-sided by construction -- d_acc_flag[e->cur] -- and the device test runs it on each half.)"""
import numpy as np
import pytest

from state_io_model import EQUIVALENT, LAST, MUTANTS, TARGET, Store, floats, words

B0 = np.arange(0, 30, 6)           # 4 tiles of 6 beams
NB = int(B0[-1])
NAN, NEG_ZERO = 0x7FC00000, 0x80000000


def quiet_scene():
    rest = np.float32(30.0) + np.arange(NB, dtype="<f4") * np.float32(0.125)
    return rest, rest.copy(), rest * np.float32(1.001), B0


def odd_rest_scene():
    """one rest length a NaN, one +0.0, both uploaded with target == rest by bits: no tile is flagged"""
    rest = words(quiet_scene()[0])
    rest[8] = NAN
    rest[14] = 0
    return rest, rest.copy(), words(floats(rest) * np.float32(1.001)), B0


def the_edit(st):
    """the device test's edit on the model's export: tile 0's targets to 0.8 rest, one bit in tile 2, tile 3's lasts x 1.1, a NaN
    target in tile 1, a -0.0 last in tile 1"""
    rows = st.export()[:, :2].copy()
    rows[0:6, 0] = words(floats(st.rest[0:6]) * np.float32(0.8))
    rows[13, 0] += 1
    rows[18:24, 1] = words(floats(rows[18:24, 1]) * np.float32(1.1))
    rows[7, 0] = NAN
    rows[9, 1] = NEG_ZERO
    return rows


def the_odd_edit(st):
    """a target equal to a NaN rest length by bits (no flag), a -0.0 target over a +0.0 rest length (a flag: the words differ)"""
    rows = st.export()[:, :2].copy()
    rows[8, 0] = NAN
    rows[14, 0] = NEG_ZERO
    return rows


def all_scaled(st):
    rows = st.export()[:, :2].copy()
    rows[:, 0] = words(floats(rows[:, 0]) * np.float32(0.9))
    rows[:, 1] = words(floats(rows[:, 1]) * np.float32(1.05))
    return rows


# tiles that yield in the launch that starts at substep k (a breaking scene): tile 1 before any checkpoint, tile 2 for the first time
# between the checkpoint and the restore of every script below, tile 3 late
YIELDS = {0: (1,), 6: (2,), 7: (2,), 12: (3,)}


def inputs(st, yields):
    k = st.substeps_done
    f = np.float32(1.0) + np.float32(0.001) * ((k * 7 + np.arange(NB)) % 13).astype("<f4")
    with np.errstate(invalid="ignore"):
        return words(floats(st.rest) * f), (yields or {}).get(k, ())


def run(script, mutant=None):
    """-> (reads [(label, observation)], halves on which the imports / checkpoints / restores were issued)"""
    st = Store(*script["scene"](), mutant=mutant)
    reads, halves = [], []

    def launch(n=1):
        for _ in range(n):
            st.launch(*inputs(st, script.get("yields")))

    for op in script["ops"]:
        if op[0] == "launch":
            launch(op[1])
        elif op[0] == "reach":          # as the device tests: step(1), and once more if that is not the half
            launch()
            if st.cur != op[1]:
                launch()
        elif op[0] == "import":
            halves.append(st.cur)
            st.import_beams(op[1](st), op[2])
        elif op[0] == "checkpoint":
            halves.append(st.cur)
            st.checkpoint()
        elif op[0] == "restore":
            halves.append(st.cur)
            st.restore()
        elif op[0] == "read":
            reads.append((op[1], st.read()))
        else:
            raise AssertionError(op)
    return reads, halves


def reads_after(n, more):
    ops = []
    for i in range(n):
        ops += [("launch", 1), ("read", "step %d" % (i + 1))]
    return ops + [("launch", more), ("read", "later")]


def scripts():
    out = {}
    for h in (0, 1):
        out["a-import-h%d" % h] = dict(scene=quiet_scene, ops=[("launch", 2), ("reach", h), ("import", the_edit, TARGET | LAST),
                                                                 ("read", "imported")] + reads_after(3, 6))
        out["a-words-h%d" % h] = dict(scene=odd_rest_scene, ops=[("launch", 2), ("reach", h), ("import", the_odd_edit, TARGET),
                                                                   ("read", "imported")] + reads_after(3, 6))
        out["b-target-h%d" % h] = dict(scene=quiet_scene, ops=[("launch", 2), ("reach", h), ("import", the_edit, TARGET),
                                                                 ("read", "imported")] + reads_after(3, 0))
        out["b-last-h%d" % h] = dict(scene=quiet_scene, ops=[("launch", 2), ("reach", h), ("import", the_edit, LAST),
                                                               ("read", "imported")] + reads_after(3, 0))
        out["d-undo-a%d" % h] = dict(scene=quiet_scene, yields=YIELDS,
                                     ops=[("launch", 2), ("reach", h), ("checkpoint",), ("launch", 1), ("import", all_scaled, TARGET | LAST),
                                          ("launch", 4), ("restore",), ("read", "restored")] + reads_after(3, 6))
        for b in (0, 1):
            out["c-rewind-a%d-b%d" % (h, b)] = dict(scene=quiet_scene, yields=YIELDS,
                                                    ops=[("launch", 2), ("reach", h), ("checkpoint",), ("read", "checkpoint"), ("launch", 5),
                                                         ("reach", b), ("read", "ran on"), ("restore",), ("read", "restored")]
                                                    + reads_after(3, 8))
    return out


SCRIPTS = scripts()
# the mutants that survive every script that stays on half 0 -- the gap the both-halves tests close (computed below and compared)
HALF0_SURVIVORS = {"import-no-target_b", "import-no-plastic_b", "import-last-half0", "ckpt-last0", "restore-no-cur",
                   "restore-engine-halves"}


@pytest.fixture(scope="module")
def table():
    """{script: (halves, {mutant: killed})}"""
    out = {}
    for name, sc in SCRIPTS.items():
        truth, halves = run(sc)
        out[name] = (halves, {m: run(sc, m)[0] != truth for m in MUTANTS})
    return out


def test_scripts_reach_the_halves_they_name(table):
    for name, (halves, _) in table.items():
        tag = name.split("-", 2)[2]
        if tag.startswith("h"):
            assert halves == [int(tag[1])], name
        elif name.startswith("c-"):
            assert halves == [int(tag[1]), int(tag[4])], name
        else:                       # d: checkpoint on a, the import one launch later, the restore four launches after that
            a = int(tag[1])
            assert halves == [a, a ^ 1, a ^ 1], name
    half0 = sorted(n for n, (h, _) in table.items() if set(h) == {0})
    assert half0 == ["a-import-h0", "a-words-h0", "b-last-h0", "b-target-h0", "c-rewind-a0-b0"]


def test_every_mutant_is_killed_or_argued_equivalent(table):
    print()
    for m, text in MUTANTS.items():
        killers = [n for n, (_, k) in table.items() if k[m]]
        print("%-24s %-88s killed by: %s" % (m, text, ", ".join(killers) or "-"))
        if m in EQUIVALENT:
            assert not killers, "%s is declared equivalent, but %s tell it from the model" % (m, killers)
        else:
            assert killers, "%s (%s) survives every script" % (m, text)


def test_the_both_halves_scripts_close_the_gap(table):
    on_half0 = {n for n, (h, _) in table.items() if set(h) == {0}}
    survivors = {m for m in MUTANTS if m not in EQUIVALENT and not any(table[n][1][m] for n in on_half0)}
    assert survivors == HALF0_SURVIVORS, "what survives the half-0 scripts is not what this test records"
    for m in survivors:
        killers = [n for n in table if n not in on_half0 and table[n][1][m]]
        assert killers, m + " survives the both-halves scripts too"


def test_flag_rule_needs_its_own_script(table):
    """!= on floats raises a flag for a NaN target over the same NaN rest length (one flag too many: harmless, but plastic_tiles
    shows it) and none for -0.0 over +0.0 (the tile goes on using +0.0): only a scene with such rest lengths tells it apart."""
    for name, (_, killed) in table.items():
        assert killed["import-flag-float"] == name.startswith("a-words"), name


# ---- the model itself: the equalities the device tests assert must hold for it

def uploaded_like(a, rows):
    """an engine uploaded with a's state, its beams' target / last replaced by `rows`"""
    b = Store(a.rest, rows[:, 0], rows[:, 1], a.b0)
    b.strain, b.stress = a.strain.copy(), a.stress.copy()
    b.trace[0][:] = a.trace[a.pcur]
    b.substeps_done = a.substeps_done
    return b


def seen(st):
    return st.read()[:3]       # rows, particles, plastic_tiles: not the halves


@pytest.mark.parametrize("h", [0, 1])
@pytest.mark.parametrize("scene,edit,fields", [(quiet_scene, the_edit, TARGET | LAST), (odd_rest_scene, the_odd_edit, TARGET),
                                               (quiet_scene, the_edit, TARGET), (quiet_scene, the_edit, LAST)],
                         ids=["a", "a-words", "b-target", "b-last"])
def test_model_import_equals_upload(h, scene, edit, fields):
    a = Store(*scene())
    for _ in range(2):
        a.launch(*inputs(a, None))
    a.launch(*inputs(a, None))
    if a.cur != h:
        a.launch(*inputs(a, None))
    assert a.cur == h and a.plastic_tiles() == 0
    rows, base = edit(a), a.export()[:, :2].copy()
    if not fields & TARGET:
        rows[:, 0] = base[:, 0]
    if not fields & LAST:
        rows[:, 1] = base[:, 1]
    b = uploaded_like(a, rows)
    a.import_beams(edit(a), fields)
    assert np.array_equal(a.export()[:, :2], rows)
    for i in range(10):
        assert seen(a) == seen(b), "launch %d after the import" % i
        for st in (a, b):
            st.launch(*inputs(st, None))
    assert a.plastic_tiles() >= 1 if fields & TARGET else a.plastic_tiles() == 0


@pytest.mark.parametrize("a,b", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_model_rewind(a, b):
    reads, _ = run(SCRIPTS["c-rewind-a%d-b%d" % (a, b)])
    reads = dict(reads)
    assert reads["restored"] == reads["checkpoint"] and reads["ran on"] != reads["checkpoint"]
    assert reads["ran on"][2] > reads["checkpoint"][2], "a tile must yield for the first time between checkpoint and restore"
    straight = Store(*quiet_scene())
    while straight.substeps_done < reads["later"][5]:
        straight.launch(*inputs(straight, YIELDS))
        for label in ("step 1", "step 2", "step 3", "later"):
            if straight.substeps_done == reads[label][5]:
                assert seen(straight) == reads[label][:3], label


@pytest.mark.parametrize("a", [0, 1])
def test_model_restore_undoes_import(a):
    reads = dict(run(SCRIPTS["d-undo-a%d" % a])[0])
    straight = Store(*quiet_scene())
    hit = 0
    while straight.substeps_done < reads["later"][5]:
        for label in ("restored", "step 1", "step 2", "step 3"):
            if straight.substeps_done == reads[label][5]:
                assert seen(straight) == reads[label][:3], label
                hit += 1
        straight.launch(*inputs(straight, YIELDS))
    assert hit == 4 and seen(straight) == reads["later"][:3]
