"""BatchEngine.bodies (sb_batch_bodies_device) against tests/batch_bodies_ref.py: on one oracle.OracleEngine per
scene, and on what load_scene returns.  Everything is integers and compared exactly.  Scenes and programs live in
tests/batch_bodies_cases.py; tests/test_batch_bodies_cpu.py shows on the CPU that they bite."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
from batch_harness import apply_to_batch, load_all, make_batch, upload_each  # noqa: E402
import batch_bodies_cases as cs  # noqa: E402
import batch_bodies_ref as br  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("labels", "sizes", "counts")
SENTINEL = -7


def bodies_np(be):
    """(labels, sizes, counts) of the batch as numpy arrays, in the reference's order."""
    labels, counts, sizes = be.bodies(sizes=True)
    return labels.cpu().numpy(), sizes.cpu().numpy(), counts.cpu().numpy()


def assert_bodies(got, exp, what):
    for name, g, e in zip(NAMES, got, exp):
        assert g.dtype == np.int32 and g.shape == e.shape, (what, name, g.dtype, g.shape, e.shape)
        if not np.array_equal(g, e):
            at = tuple(int(x[0]) for x in np.nonzero(g != e))
            raise AssertionError("%s: %s differ in %d words, first at %s: got %d, expected %d" % (what, name, int((g != e).sum()), at, g[at], e[at]))


def assert_against_load_scene(be, bufs, got, what):
    assert_bodies(got, br.bodies_of(load_all(be, bufs), be.max_particles), what + " against load_scene")


def assert_info(be):
    maxP, maxB = be.max_particles, be.max_beams
    assert be.info("body_words") == 4 and be.info("bodies_kernel_scratch_bytes") == 0 and 0 < be.info("bodies_kernel_vgprs") <= 128
    assert be.info("bodies_lds_bytes") == (4 * maxP + maxB + 6) * 4 <= 33 * 1024


@pytest.fixture(scope="module")
def expected(sb, oracle):
    """Every stepped case on one oracle per scene, once: {name: (case, {op index: (labels, sizes, counts)})}."""
    return {c["name"]: (c, cs.expected_bodies(oracle, c)[0]) for c in cs.stepped_cases(sb)}


def run_case(sb, case, exp):
    """The program on the batch; after the ops of compare_after the three outputs against the oracles' and against the reference
    on what load_scene returns."""
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    got = {}
    for k, op in enumerate(case["program"]):
        apply_to_batch(be, op)
        if k in case["compare_after"]:
            got[k] = bodies_np(be)
            assert_bodies(got[k], exp[k], "%s after op %d" % (case["name"], k))
            assert_against_load_scene(be, case["bufs"], got[k], "%s after op %d" % (case["name"], k))
    assert_info(be)
    return be, got


def test_breaking_lattices_removed_beams_stale_mapping_tail_and_pending_flags(sb, expected):
    case, exp = expected["yield / break / delete"]
    be, got = run_case(sb, case, exp)
    after_frames, mid_frame = (got[k][2] for k in case["compare_after"])
    assert after_frames[:, 0].tolist() == [1, 6, 21, 38, 56, 1] and after_frames[:, 1].tolist() == [144, 139, 120, 101, 84, 144]
    assert after_frames[:, 2].tolist() == [0, 5, 18, 33, 53, 0]
    pending = be.summary()[:, sb.batch.SUMMARY_FIELDS.index("pending_breaks")].cpu().numpy()
    assert (pending > 0).any() and np.array_equal(mid_frame, after_frames)      # a pending flag still connects
    be.destroy()


def test_heterogeneous_batch_pending_flags_connect_and_the_delete_pass_splits(sb, expected):
    case, exp = expected["heterogeneous"]
    assert case["cap"] == (1024, 4096)
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    n = len(case["program"])
    for k, op in enumerate(case["program"]):
        if k == n - 1:   # in front of the delete pass: 129 flags pending in the lattice, which is still one body
            pending = be.summary()[:, sb.batch.SUMMARY_FIELDS.index("pending_breaks")].cpu().numpy()
            assert pending[cs.LATTICE] == 129
        apply_to_batch(be, op)
        if k in case["compare_after"]:
            got = bodies_np(be)
            assert_bodies(got, exp[k], "heterogeneous after op %d" % k)
            assert_against_load_scene(be, case["bufs"], got, "heterogeneous after op %d" % k)
            if k == n - 2:
                assert br.brief(got[2]) == [(9, 40, 2), (1, 144, 0), (1, 1024, 0), (1, 2, 0), (0, 0, 0), (0, 0, 0)]
                assert got[2][:, 3].tolist() == [46, 0, 0, 0, -1, -1] and (got[0][4:] == -1).all() and not got[1][4:].any()
            if k == n - 1:
                assert br.brief(got[2])[cs.LATTICE] == (9, 110, 3) and br.brief(got[2])[2] == (58, 967, 57)
    assert_info(be)
    be.destroy()


@pytest.mark.parametrize("which", ["mapping", "default", "default_120_300", "saturation", "pile"])
def test_bodies_against_the_oracle(sb, expected, which):
    """Slots != data indices with particles at data indices 50 and up; the default scene at 128 / 320 and 120 / 300; capacity
    8 / 8; 256 particles with max_beams = 0."""
    case = getattr(cs, "case_" + which)(sb)
    case, exp = expected[case["name"]]
    be, got = run_case(sb, case, exp)
    labels, sizes, counts = got[max(got)]
    if which == "mapping":
        for i, b in enumerate(case["bufs"]):
            holds = np.zeros(be.max_particles, bool)
            holds[b.mapping[:b.particle_count]] = True
            assert np.array_equal(labels[i] == -1, ~holds) and not holds[:3].any(), i   # -1 exactly where no particle is
    if which in ("default", "default_120_300"):
        assert br.brief(counts) == [(9, 40, 2)]
    if which == "pile":
        assert be.max_beams == 0 and br.brief(counts) == [(256, 1, 256)] and np.array_equal(labels[0], np.arange(256))
        assert np.array_equal(sizes[0], np.stack([np.ones(256, np.int32), np.zeros(256, np.int32)], axis=1))
    be.destroy()


@pytest.mark.parametrize("which", [0, 1, 2])
def test_graphs_built_for_the_search(sb, which):
    """The shuffled path of 1024 (the deepest component there is), a cycle, a star with the hub at the largest data index, 16
    pieces of 64, 512 pairs, 4096 parallel beams -- in one batch at capacity 1024 / 4096; the path at 8 / 8 and at 65 / 64."""
    case = cs.graph_cases(sb)[which]
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    got = bodies_np(be)
    assert_bodies(got, br.bodies_of(case["bufs"], be.max_particles), case["name"])
    assert [tuple(r) for r in got[2].tolist()] == [tuple(c) for c in case["counts"]]
    assert_against_load_scene(be, case["bufs"], got, case["name"])
    if which == 0:
        pieces = got[1][case["order"].index("pieces")]
        assert sorted(pieces[pieces[:, 0] > 0].tolist()) == [[64, 63]] * 16
        assert all(np.array_equal(got[0][0], got[0][i]) for i, k in enumerate(case["order"]) if k == "path")
    assert_info(be)
    be.destroy()


def test_every_combination_of_outputs_writes_exactly_its_own(sb):
    """Through the C call: a NULL output is not written, a non-NULL one whole, and nothing behind its n_scenes rows."""
    import torch
    case = cs.case_small_path(sb, (65, 64))
    n, maxP = len(case["bufs"]), 65
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    exp = br.bodies_of(case["bufs"], maxP)
    L = sb.batch.load_library()
    shapes = ((n + 1, maxP), (n + 1, maxP, 2), (n + 1, 4))
    for mask in range(1, 8):
        outs = [torch.full(s, SENTINEL, dtype=torch.int32, device="cuda") for s in shapes]
        torch.cuda.synchronize()
        ptrs = [ctypes.c_void_p(o.data_ptr()) if mask >> k & 1 else None for k, o in enumerate(outs)]
        assert L.sb_batch_bodies_device(be._h, *ptrs) == 0, L.sb_batch_last_error(be._h)
        be.sync()
        for k, o in enumerate(outs):
            a = o.cpu().numpy()
            if mask >> k & 1:
                assert np.array_equal(a[:n], exp[k]) and (a[n:] == SENTINEL).all(), (mask, NAMES[k])
            else:
                assert (a == SENTINEL).all(), (mask, NAMES[k])
    # the Python call: tensors larger than needed and of another shape are written at their head, and come back as views
    flat = [torch.full((int(np.prod(s)) + 3,), SENTINEL, dtype=torch.int32, device="cuda") for s in shapes]
    labels, counts, sizes = be.bodies(labels=flat[0], sizes=flat[1], counts=flat[2])
    assert (labels.data_ptr(), sizes.data_ptr(), counts.data_ptr()) == tuple(f.data_ptr() for f in flat)
    assert tuple(labels.shape) == (n, maxP) and tuple(sizes.shape) == (n, maxP, 2) and tuple(counts.shape) == (n, 4)
    for k, (f, view) in enumerate(zip(flat, (labels, sizes, counts))):
        assert np.array_equal(view.cpu().numpy(), exp[k]) and bool((f[view.numel():] == SENTINEL).all()), NAMES[k]
    two = be.bodies()
    assert len(two) == 2 and np.array_equal(two[0].cpu().numpy(), exp[0]) and np.array_equal(two[1].cpu().numpy(), exp[2])
    be.destroy()


def assert_scenes_equal(a, b, bufs, what):
    for i, (x, y) in enumerate(zip(load_all(a, bufs), load_all(b, bufs))):
        if x is not None:
            bc.assert_same(x, y, "%s: scene %d" % (what, i))


def test_bodies_only_reads(sb):
    """frame, bodies, frame equals frame, frame -- bit for bit through load_scene; likewise mid-frame with flags pending."""
    case = cs.case_break(sb)
    a, b = make_batch(sb, case), make_batch(sb, case)
    for be in (a, b):
        upload_each(be, case["bufs"])
        be.frame(1)
    a.bodies(sizes=True)
    a.frame(1)
    b.frame(1)
    assert_scenes_equal(a, b, case["bufs"], "frame, bodies, frame")
    a.step(5)
    b.step(5)
    a.bodies()
    a.step(59)
    a.delete_pass()
    b.step(59)
    b.delete_pass()
    assert_scenes_equal(a, b, case["bufs"], "step, bodies, step, delete")
    assert a.info("frames_done") == b.info("frames_done") and a.info("substeps_done") == b.info("substeps_done")
    a.destroy()
    b.destroy()


def test_bodies_between_fork_reset_and_checkpoint_without_a_sync(sb):
    """bodies() in front of fork(argsort(counts[:, 0])) and right behind fork / reset / checkpoint: the stream orders them."""
    import torch
    case = cs.case_break(sb)
    bufs, n = case["bufs"], len(case["bufs"])
    be = make_batch(sb, case)
    upload_each(be, bufs)
    be.frame(2)
    l0, c0, s0 = be.bodies(sizes=True)
    src = torch.argsort(c0[:, 0], stable=True).to(torch.int32)
    be.fork(src)
    l1, c1, s1 = be.bodies(sizes=True)
    idx = src.long()
    assert c0[:, 0].tolist() == [1, 6, 21, 38, 56, 1] and idx.tolist() == [0, 5, 1, 2, 3, 4]         # (the first wait)
    assert torch.equal(c1, c0[idx]) and torch.equal(l1, l0[idx]) and torch.equal(s1, s0[idx])
    mask = torch.tensor([0, 0, 0, 1, 0, 1], dtype=torch.uint8, device="cuda")
    be.checkpoint(mask)                    # scenes 3 and 5 keep what they hold as their reset state
    l2, c2 = be.bodies()
    assert torch.equal(c2, c1) and torch.equal(l2, l1)
    be.reset()                             # the others go back to the reset state of their fork's source: the whole lattice
    l3, c3 = be.bodies()
    whole = torch.tensor([1, 144, 0, 0], dtype=torch.int32, device="cuda")
    for i in range(n):
        assert torch.equal(c3[i], c1[i] if int(mask[i]) else whole), i
        if int(mask[i]):
            assert torch.equal(l3[i], l1[i]), i
    got = (l3.cpu().numpy(), be.bodies(sizes=True)[2].cpu().numpy(), c3.cpu().numpy())
    forked = [bufs[int(k)] for k in idx]   # (load_scene needs Buffers of the capacity only)
    assert_against_load_scene(be, forked, got, "fork, checkpoint, reset")
    be.destroy()


def test_a_forked_never_uploaded_source(sb):
    import torch
    case = cs.case_small_path(sb, (8, 8))
    bufs = case["bufs"] + [None]           # path, path, empty, path, never uploaded
    be = make_batch(sb, case, n=5)
    upload_each(be, bufs)
    before = bodies_np(be)
    assert_bodies(before, br.bodies_of(bufs, 8), "before the fork")
    assert before[2].tolist() == [[1, 8, 0, 0], [1, 8, 0, 0], [0, 0, 0, -1], [1, 8, 0, 0], [0, 0, 0, -1]]
    be.fork(torch.tensor([4, 1, 0, 2, 4], dtype=torch.int32, device="cuda"))
    after = bodies_np(be)
    assert_bodies(after, tuple(x[[4, 1, 0, 2, 4]] for x in before), "after the fork")
    assert (after[0][0] == -1).all() and not after[1][0].any() and after[2][0].tolist() == [0, 0, 0, -1]
    with pytest.raises(sb.EngineError):
        be.load_scene(0, bufs[0].copy())   # scene 0 is a never-uploaded scene now
    be.destroy()


def test_error_paths(sb):
    import torch
    case = cs.case_small_path(sb, (8, 8))
    n = len(case["bufs"])
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    i32 = dict(dtype=torch.int32, device="cuda")
    for call in (lambda: be.bodies(torch.zeros((n, 8), dtype=torch.int64, device="cuda")),            # dtype
                 lambda: be.bodies(counts=torch.zeros((n, 4), dtype=torch.float32, device="cuda")),
                 lambda: be.bodies(torch.zeros((n, 8), dtype=torch.int32)),                           # device
                 lambda: be.bodies(sizes=torch.zeros((n, 8, 2), dtype=torch.int32)),
                 lambda: be.bodies(torch.zeros((n, 7), **i32)),                                       # size
                 lambda: be.bodies(sizes=torch.zeros((n, 8), **i32)),
                 lambda: be.bodies(counts=torch.zeros((n, 3), **i32)),
                 lambda: be.bodies(torch.zeros((n, 16), **i32)[:, ::2]),                              # contiguity
                 lambda: be.bodies(counts=torch.zeros((n, 8), **i32)[:, ::2]),
                 lambda: be.bodies("no"), lambda: be.bodies(sizes=1.5)):
        with pytest.raises(ValueError):
            call()
    buf = torch.zeros(n * 8 * 2 + 8, **i32)
    for call in (lambda: be.bodies(labels=buf.data_ptr() + 2), lambda: be.bodies(counts=buf.data_ptr() + 1),
                 lambda: be.bodies(sizes=buf.data_ptr() + 3)):
        with pytest.raises(sb.EngineError) as ei:
            call()
        assert ei.value.status == 1
    L = sb.batch.load_library()
    assert L.sb_batch_bodies_device(be._h, None, None, None) == 1 and "all null" in L.sb_batch_last_error(be._h).decode()
    assert L.sb_batch_bodies_device(None, ctypes.c_void_p(buf.data_ptr()), None, None) == 1
    labels, counts = be.bodies()           # and the batch is as usable as before
    assert counts.cpu().numpy().tolist() == [list(c) for c in case["counts"]]
    be.sync()
    be.destroy()
