"""BatchEngine.fork / checkpoint / write_beams_device (sb_batch_fork_device, _checkpoint_device, _write_beams_device; DESIGN.md
5.12) against one oracle.OracleEngine per scene: bit-exact, no tolerance.  Scenes, edits and the oracle-side bookkeeping live in
tests/batch_fork_cases.py; tests/test_batch_fork_cpu.py asserts on the CPU that every program here keeps the oracle finite."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
from batch_harness import apply_to_batch as apply_op, load_all, make_batch, upload_each  # noqa: E402
import batch_fork_cases as fc  # noqa: E402
import batch_grid_cases as gc  # noqa: E402
from render_ref import render_ref  # noqa: E402

pytestmark = pytest.mark.gpu


def apply_to_batch(be, ops):
    for op in ops:
        apply_op(be, op)


def sources(src, dtype="uint32"):
    import torch
    return torch.from_numpy(np.array(src, dtype=np.uint32).view(dtype)).cuda()


def compare(be, templates, refs, what):
    for i, (t, ref) in enumerate(zip(templates, refs)):
        if ref is None:
            continue
        exp = ref.load_buffers(t.copy())
        assert np.isfinite(exp.particles).all()
        bc.assert_same(be.load_scene(i, t.copy()), exp, "%s: scene %d" % (what, i))


def start(sb, oracle, case, n=None):
    """The batch and one oracle per scene after the case's program."""
    be = make_batch(sb, case, n)
    upload_each(be, case["bufs"])
    refs = [None if b is None else bc.make_oracle(oracle, case, b) for b in case["bufs"]]
    apply_to_batch(be, case["program"])
    fc.advance(refs, case["program"])
    return be, refs


# ---------------------------------------------------------------- 1. broadcast
@pytest.mark.parametrize("which", ["hetero", "break"])
def test_broadcast(sb, oracle, which):
    """2 frames + step(5) (flags pending), scene k over all -- an empty and a never-uploaded scene among the destinations of the
    heterogeneous batch, removed beams and a compacted mapping in the source of the other."""
    case = bc.case_hetero(sb) if which == "hetero" else bc.case_break(sb)
    k = 1 if which == "hetero" else 4
    n = len(case["bufs"])
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    ref = bc.make_oracle(oracle, case, case["bufs"][k])
    ops = [op for op in case["program"] if op[0] == "consts"] + [("frame", 2), ("step", 5)]
    apply_to_batch(be, ops)
    fc.advance([None] * k + [ref], ops)
    tpl = case["bufs"][k]
    before = be.load_scene(k, tpl.copy())
    bc.assert_same(before, ref.load_buffers(tpl.copy()), "source before the fork")
    if which == "break":
        assert ref.delete.any() and before.beam_count < tpl.beam_count
    be.fork(sources([k] * n), constants=True)
    # every scene keeps its own user input: what it was uploaded with, zeros in the scene that never was
    inputs = [np.zeros(8, "<u4") if b is None else b.metadata[20:28].copy() for b in case["bufs"]]
    refs = []
    for i in range(n):
        exp = before.copy()
        exp.metadata[20:28] = inputs[i]
        bc.assert_same(be.load_scene(i, tpl.copy()), exp, "%s: scene %d after the fork" % (which, i))
        refs.append(fc.clone(ref))
        refs[i].metadata[20:28] = inputs[i]
    assert be.info("fork_staging_bytes") > 0 and be.info("fork_bad_sources") == 0
    tail = [("delete",), ("frame", 2)]
    apply_to_batch(be, tail)
    fc.advance(refs, tail)
    compare(be, [tpl] * n, refs, which + " continued")
    be.destroy()


# ---------------------------------------------------------------- 2. snapshot semantics
def test_snapshot_semantics(sb, oracle):
    """64 distinct scenes: a rotation, a swap, and a broadcast whose source is itself overwritten.  Scene i equals OLD scene
    src[i] (with its own user input), and the next frame follows that oracle."""
    n = 64
    case = fc.case_distinct(sb, n)
    be, refs = start(sb, oracle, case)
    tpl = case["bufs"][0]
    assert be.info("fork_staging_bytes") == 0
    for name, src in fc.snapshot_sources(n):
        old = load_all(be, [tpl] * n)
        be.fork(sources(src, "int32"))
        for i in range(n):
            exp = old[src[i]].copy()
            exp.metadata[20:28] = old[i].metadata[20:28]
            bc.assert_same(be.load_scene(i, tpl.copy()), exp, "%s: scene %d is old scene %d" % (name, i, src[i]))
        refs = fc.fork_oracles(refs, src)
        compare(be, [tpl] * n, refs, name)
        be.frame()
        fc.advance(refs, [("frame", 1)])
        compare(be, [tpl] * n, refs, name + " + a frame")
    assert be.info("fork_bad_sources") == 0
    be.destroy()
    one_case = fc.case_distinct(sb, 1)
    one, ref = start(sb, oracle, one_case)
    one.fork(sources([0]))
    compare(one, [tpl], ref, "N = 1, src = [0]")
    one.frame()
    fc.advance(ref, [("frame", 1)])
    compare(one, [tpl], ref, "N = 1 + a frame")
    one.destroy()


# ---------------------------------------------------------------- 3. entries that leave the scene alone
def test_keep_self_and_out_of_range_entries(sb, oracle):
    import torch
    n = 8
    case = fc.case_distinct(sb, n)
    be, refs = start(sb, oracle, case)
    tpl = case["bufs"][0]
    src = fc.KEEP_SOURCES
    untouched = [i for i, s in enumerate(src) if s == i or s >= n]
    assert untouched == [0, 1, 2, 3, 5, 6]
    before = [t.clone() for t in be.state_tensors()]
    old = load_all(be, [tpl] * n)
    be.fork(sources(src))
    after = be.state_tensors()
    for i in untouched:
        for a, b in zip(after, before):
            assert torch.equal(a[i].view(torch.uint8), b[i].view(torch.uint8)), "scene %d changed" % i
        bc.assert_same(be.load_scene(i, tpl.copy()), old[i], "scene %d untouched" % i)
    assert be.info("fork_bad_sources") == fc.KEEP_BAD
    refs = fc.fork_oracles(refs, src)
    compare(be, [tpl] * n, refs, "after the fork")
    be.frame()
    fc.advance(refs, [("frame", 1)])
    compare(be, [tpl] * n, refs, "a frame later")
    be.fork(sources([-1 & 0xFFFFFFFF] * n, "int32"))          # -1 everywhere: nothing happens, nothing is counted
    compare(be, [tpl] * n, refs, "all KEEP")
    be.fork(sources([n + 5] * n))
    assert be.info("fork_bad_sources") == fc.KEEP_BAD + n      # counted over all forks
    compare(be, [tpl] * n, refs, "all out of range")
    be.destroy()


# ---------------------------------------------------------------- 4. constants and input
@pytest.mark.parametrize("constants", [False, True])
def test_constants_and_input(sb, oracle, constants):
    case = fc.case_consts(sb)
    be, refs = start(sb, oracle, case)
    tpl = case["bufs"][0]
    old = load_all(be, [tpl] * 4)
    src = fc.CONSTS_SOURCES
    be.fork(sources(src), constants=constants)
    for i in range(4):
        got = be.load_scene(i, tpl.copy())
        assert np.array_equal(got.metadata[20:28], old[i].metadata[20:28]), "scene %d keeps its user input" % i
        assert np.array_equal(got.metadata[12:20], old[src[i] if constants else i].metadata[12:20]), "scene %d: constants" % i
        assert not np.array_equal(old[i].metadata[12:20], old[src[i]].metadata[12:20])
        assert np.array_equal(got.particles.view("u4"), old[src[i]].particles.view("u4"))
    refs = fc.fork_oracles(refs, src, constants)
    be.frame()
    fc.advance(refs, [("frame", 1)])
    compare(be, [tpl] * 4, refs, "constants=%s" % constants)
    be.destroy()


# ---------------------------------------------------------------- 5. a source that was never uploaded
def test_never_uploaded_source(sb, oracle):
    import torch
    case = fc.case_distinct(sb, 3)
    case["bufs"] = case["bufs"][:2] + [None]
    be, refs = start(sb, oracle, case)
    tpl = case["bufs"][0]
    be.fork(sources([0, 2, fc.KEEP]))
    with pytest.raises(sb.EngineError) as ei:
        be.load_scene(1, tpl.copy())
    assert ei.value.status == 5
    refs = fc.fork_oracles(refs, [0, 2, fc.KEEP])
    assert refs[1] is None
    pics = be.render(32)
    be.frame()
    fc.advance(refs, [("frame", 1)])
    p, b, a = be.state_tensors()
    assert bool(p[1:].isnan().all()) and bool(b[1:].isnan().all()) and not bool(a[1:].any())
    assert not bool(pics[1:].any()) and bool(pics[0].any())
    with pytest.raises(sb.EngineError):
        be.load_scene(1, tpl.copy())
    be.reset()                                                  # fault-free on the scene that is no scene any more
    be.checkpoint()
    with pytest.raises(sb.EngineError):
        be.load_scene(1, tpl.copy())
    refs[0] = bc.make_oracle(oracle, case, tpl)
    refs[0].write_user_input(fc.distinct_inputs(sb, 3)[0])
    compare(be, [tpl, None, None], refs, "neighbour, reset to its upload")
    be.destroy()


# ---------------------------------------------------------------- 6. checkpoint
def pictures_equal(be, templates, want, what, res=64):
    got = be.render(res)
    be.sync()
    g = got.cpu().numpy()
    for i, t in enumerate(templates):
        assert np.array_equal(g[i], want[i]), "%s: picture of scene %d" % (what, i)


def test_checkpoint_and_reset(sb, oracle):
    import torch
    case = bc.case_break(sb)
    bufs = case["bufs"]
    n = len(bufs)
    be = make_batch(sb, case)
    upload_each(be, bufs)
    refs = [bc.make_oracle(oracle, case, b) for b in bufs]
    apply_to_batch(be, [("frame", 2)])
    fc.advance(refs, [("frame", 2)])
    assert any(int(r.metadata[6]) < b.beam_count for r, b in list(zip(refs, bufs))[0::2]), "a masked scene must have lost beams"
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
    mask[0::2] = 1
    be.checkpoint(mask)
    at = load_all(be, bufs)
    saved = [fc.clone(r) for r in refs]
    pics = [render_ref(at[i], 64, 1000.0, 10.0) for i in range(n)]
    state = [t.clone() for t in be.state_tensors()]
    compare(be, bufs, refs, "at the checkpoint")
    more = [("frame", 1), ("step", 5)]
    apply_to_batch(be, more)
    fc.advance(refs, more)
    again = torch.ones(n, dtype=torch.bool, device="cuda")
    again[3] = again[5] = False                                # scene 1: reset but not checkpointed -> its upload
    be.reset(again)
    for i in (0, 2, 4):
        got = be.load_scene(i, bufs[i].copy())
        bc.assert_same(got, at[i], "scene %d is back at its checkpoint" % i)
        assert got.beam_count == int(saved[i].metadata[6])
        refs[i] = fc.clone(saved[i])
    bc.assert_same(be.load_scene(1, bufs[1].copy()), bufs[1], "scene 1 is back at its upload")
    refs[1] = bc.make_oracle(oracle, case, bufs[1])
    compare(be, bufs, refs, "after the reset")
    now = be.state_tensors()
    for i in (0, 2, 4):
        for a, b in zip(now, state):
            assert torch.equal(a[i].view(torch.uint8), b[i].view(torch.uint8)), "read_state_device of scene %d" % i
    want = list(pics)
    for i in (1, 3, 5):
        want[i] = render_ref(be.load_scene(i, bufs[i].copy()), 64, 1000.0, 10.0)
    pictures_equal(be, bufs, want, "after the reset")
    # checkpoint(None) mid-frame: pending break flags are part of the checkpoint
    apply_to_batch(be, more)
    fc.advance(refs, more)
    assert any(r.delete.any() for r in refs)
    be.checkpoint()
    at = load_all(be, bufs)
    saved = [fc.clone(r) for r in refs]
    rest = [("step", 59), ("delete",), ("frame", 1)]
    apply_to_batch(be, rest)
    fc.advance(refs, rest)
    compare(be, bufs, refs, "past checkpoint(None)")
    be.reset()
    refs = [fc.clone(r) for r in saved]
    for i in range(n):
        bc.assert_same(be.load_scene(i, bufs[i].copy()), at[i], "reset to checkpoint(None), scene %d" % i)
    apply_to_batch(be, rest)
    fc.advance(refs, rest)
    compare(be, bufs, refs, "continued from checkpoint(None): the pending flags came back")
    # fork without as_reset: the destination's reset state becomes its source's (scene 4's checkpoint)
    be.fork(sources([4] * n))
    refs = fc.fork_oracles(refs, [4] * n)
    tpl = [bufs[4]] * n
    be.frame()
    fc.advance(refs, [("frame", 1)])
    but2 = torch.ones(n, dtype=torch.uint8, device="cuda")
    but2[2] = 0
    be.reset(but2)
    for i in range(n):
        if i != 2:
            bc.assert_same(be.load_scene(i, bufs[4].copy()), at[4], "reset after a plain fork, scene %d" % i)
            refs[i] = fc.clone(saved[4])
    apply_to_batch(be, rest)
    fc.advance(refs, rest)
    compare(be, tpl, refs, "after the plain fork")
    # fork with as_reset: the forked state itself
    mid, mid_ref = be.load_scene(2, bufs[4].copy()), fc.clone(refs[2])
    assert not np.array_equal(mid.particles, be.load_scene(0, bufs[4].copy()).particles)
    be.fork(sources([2, 2, fc.KEEP, 2, 2, 2]), as_reset=True)
    apply_to_batch(be, [("frame", 1), ("step", 3)])
    be.reset()
    for i in range(n):
        bc.assert_same(be.load_scene(i, bufs[4].copy()), at[4] if i == 2 else mid, "reset after fork(as_reset), scene %d" % i)
    refs = [fc.clone(saved[4]) if i == 2 else fc.clone(mid_ref) for i in range(n)]
    be.frame()
    fc.advance(refs, [("frame", 1)])
    compare(be, tpl, refs, "a frame after the last reset")
    be.destroy()


# ---------------------------------------------------------------- 7. beam import
def test_beam_import(sb, oracle):
    import torch
    case = fc.beam_case(sb)
    n, tpl = len(case["bufs"]), case["bufs"][0]
    be, refs = start(sb, oracle, case)
    be.frame()
    fc.advance(refs, [("frame", 1)])
    factors = torch.from_numpy(fc.beam_factors(n, tpl.max_beams)).cuda()
    last_f = torch.where(factors != 1.0, float(fc.LAST_FACTOR), 1.0).to(torch.float32)
    for target, last in fc.BEAM_ROUNDS:
        p, b, a = be.state_tensors()
        edit = b.clone()
        if target:
            edit[:, :, 0] = b[:, :, 0] * factors
        if last:
            edit[:, :, 1] = b[:, :, 1] * last_f
        edit[:, :, 2:] = 7.0                                    # strain and stress are never imported
        be.write_beams_device(edit, target_length=target, last_length=last)
        rows = edit.cpu().numpy()
        exp_rows = fc.edit_beams(b.cpu().numpy(), fc.beam_factors(n, tpl.max_beams), target, last)
        have = ~np.isnan(exp_rows[:, :, 0])
        assert np.array_equal(rows[have][:, :2].view("u4"), exp_rows[have][:, :2].view("u4"))      # the values the CPU test ran
        for i, r in enumerate(refs):
            fc.import_into_oracle(r, tpl, rows[i], target, last)
        compare(be, [tpl] * n, refs, "right after the import %s" % ((target, last),))
        be.frame()
        fc.advance(refs, [("frame", 1)])
        compare(be, [tpl] * n, refs, "a frame after the import %s" % ((target, last),))
    # a NaN target in scene 2: its neighbours stay exact
    p, b, a = be.state_tensors()
    idx = int(tpl.mapping[tpl.max_particles + 5])
    b[2, idx, 0] = float("nan")
    be.write_beams_device(b)
    assert bool(be.state_tensors()[1][2, idx, 0].isnan())
    be.frame()
    fc.advance(refs, [("frame", 1)])
    keep = [r if i != 2 else None for i, r in enumerate(refs)]
    compare(be, [tpl] * n, keep, "beside a NaN target")
    be.destroy()


def test_beam_import_identity_and_inert_rows(sb, oracle):
    """The batch's own export, imported mid-frame with flags pending, changes no later bit; rows of removed beams are written but
    inert; rows of data indices without a beam are not read."""
    import torch
    case = bc.case_break(sb)
    bufs = case["bufs"]
    be = make_batch(sb, case)
    upload_each(be, bufs)
    refs = [bc.make_oracle(oracle, case, b) for b in bufs]
    ops = [("frame", 2), ("step", 5)]
    apply_to_batch(be, ops)
    fc.advance(refs, ops)
    assert any(r.delete.any() for r in refs)
    p, b, a = be.state_tensors()
    be.write_beams_device(b, target_length=True, last_length=True)
    compare(be, bufs, refs, "identity import")
    # garbage into the rows of removed beams (the oracle's records get it too: load_scene shows a removed beam's last state)
    # and into rows that hold no beam (nobody reads those)
    exists = ~b[:, :, 0].isnan()
    removed = exists & ~a
    assert bool(removed.any()) and bool((~exists).any())
    edit = b.clone()
    edit[:, :, 0] = torch.where(a, b[:, :, 0], torch.full_like(b[:, :, 0], 12345.0))
    edit[:, :, 1] = torch.where(a, b[:, :, 1], torch.full_like(b[:, :, 1], -3.0))
    be.write_beams_device(edit, target_length=True, last_length=True)
    rem = removed.cpu().numpy()
    for i, r in enumerate(refs):
        r.beams["target_length"][rem[i]] = np.float32(12345.0)
        r.beams["last_length"][rem[i]] = np.float32(-3.0)
    rest = [("step", 59), ("delete",), ("frame", 1)]
    apply_to_batch(be, rest)
    fc.advance(refs, rest)
    compare(be, bufs, refs, "after the imports")
    p2, b2, a2 = be.state_tensors()
    assert bool(b2[~exists].isnan().all())
    be.destroy()


# ---------------------------------------------------------------- 8. contact cells
def test_fork_mid_frame_on_the_contact_cells(sb, oracle):
    case = gc.case_pile(sb)
    pile = case["bufs"][0]
    n = 8
    be = make_batch(sb, case, n)
    assert be.info("contact_cells_per_side") > 0
    be.write_scene(pile, 0, 1)
    pts = np.zeros((2, 6), "f4")
    pts[:, 0], pts[:, 1] = (400.0, 415.0), 300.0
    be.write_scene(gc.free_particles(sb, 2, case["cap"], pts), 1, 6)      # scene 7 is never uploaded
    ref = gc.make_oracle(oracle, case, pile)
    be.step(7)
    ref.step(7)
    seen = be.info("cell_substeps") + be.info("cell_overflow_substeps")
    assert seen == 7                                            # only scene 0 is large enough for the cells
    cells = be.info("cell_substeps")
    be.fork(sources([0] * n), constants=True)                  # (scene 7 has no physics constants of its own, and no user input)
    refs = [fc.clone(ref) for _ in range(n)]
    refs[7].metadata[20:28] = 0
    ops = [("step", 57), ("delete",), ("step", 5)]
    apply_to_batch(be, ops)
    fc.advance(refs, ops)
    compare(be, [pile] * n, refs, "pile forked mid-frame")
    assert be.info("cell_substeps") + be.info("cell_overflow_substeps") == 7 + n * 62
    assert be.info("cell_substeps") > cells
    be.destroy()


# ---------------------------------------------------------------- 9. stream ordering with torch
def test_stream_ordering_with_torch(sb, oracle):
    """src computed by torch from state_tensors() right before the fork, a render right after: no explicit sync anywhere."""
    import torch
    n = 8
    case = fc.case_distinct(sb, n)
    be, refs = start(sb, oracle, case)
    tpl = case["bufs"][0]
    old = load_all(be, [tpl] * n)
    p, b, a = be.state_tensors()
    score = torch.nan_to_num(p[:, :, 0] * 0.37 + p[:, :, 3]).sum(dim=1) * torch.tensor([3., -1., 4., -1., 5., -9., 2., -6.], device="cuda")
    src = torch.argsort(score).to(torch.int32)
    be.fork(src)
    pics = be.render(48)
    order = [int(x) for x in src.cpu()]
    assert sorted(order) == list(range(n)) and order != list(range(n))
    g = pics.cpu().numpy()
    for i in range(n):
        exp = old[order[i]].copy()
        exp.metadata[20:28] = old[i].metadata[20:28]
        got = be.load_scene(i, tpl.copy())
        bc.assert_same(got, exp, "scene %d is old scene %d" % (i, order[i]))
        assert np.array_equal(g[i], render_ref(got, 48, 1000.0, 10.0)), "picture of scene %d" % i
    be.destroy()


# ---------------------------------------------------------------- 10. error paths
def test_error_paths(sb):
    import torch
    case = bc.case_default(sb, 1)
    n = 4
    be = make_batch(sb, case, n)
    be.write_scene(case["bufs"][0])
    dev = "cuda"
    bad_calls = [lambda: be.fork(torch.zeros(n, dtype=torch.int64, device=dev)),              # dtype
                 lambda: be.fork(torch.zeros(n, dtype=torch.float32, device=dev)),
                 lambda: be.fork(torch.zeros(n - 1, dtype=torch.int32, device=dev)),           # size
                 lambda: be.fork(torch.zeros(n + 1, dtype=torch.int32, device=dev)),
                 lambda: be.fork(torch.zeros(n, dtype=torch.int32)),                           # on the CPU
                 lambda: be.checkpoint(torch.zeros(n, dtype=torch.int32, device=dev)),
                 lambda: be.checkpoint(torch.zeros(n - 1, dtype=torch.uint8, device=dev)),
                 lambda: be.checkpoint(torch.zeros(n, dtype=torch.uint8)),
                 lambda: be.write_beams_device(torch.zeros((n, 320, 4), dtype=torch.float64, device=dev)),
                 lambda: be.write_beams_device(torch.zeros((n, 319, 4), dtype=torch.float32, device=dev)),
                 lambda: be.write_beams_device(torch.zeros((n, 320, 4), dtype=torch.float32))]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    L = sb.batch.load_library()
    ok = torch.arange(n, dtype=torch.int32, device=dev)
    rows = torch.zeros((n, 320, 4), dtype=torch.float32, device=dev)
    import ctypes
    vp = ctypes.c_void_p
    assert L.sb_batch_fork_device(be._h, vp(ok.data_ptr()), 4) == 1 and b"flags" in L.sb_batch_last_error(be._h)
    assert L.sb_batch_fork_device(be._h, None, 0) == 1 and L.sb_batch_fork_device(be._h, vp(ok.data_ptr() + 2), 0) == 1
    assert L.sb_batch_write_beams_device(be._h, vp(rows.data_ptr()), 0) == 1 and L.sb_batch_write_beams_device(be._h, vp(rows.data_ptr()), 4) == 1
    assert L.sb_batch_write_beams_device(be._h, None, 1) == 1
    with pytest.raises(sb.EngineError) as ei:
        be.write_beams_device(rows, target_length=False, last_length=False)
    assert ei.value.status == 1
    assert be.info("fork_staging_bytes") == 0                   # no failed call allocated anything
    be.fork(ok)                                                 # the identity: nothing changes
    bc.assert_same(be.load_scene(3, case["bufs"][0].copy()), case["bufs"][0], "identity fork")
    assert be.info("fork_staging_bytes") > 0
    be.destroy()
