"""BatchEngine.contacts (sb_batch_contacts_device) against tests/batch_contacts_ref.py, a numpy float32 all-pairs
test without a grid: on what load_scene returns, and (finite cases) on one oracle.OracleEngine per scene.  Everything compared is
int32 and compared exactly.  Scenes and programs live in tests/batch_contacts_cases.py; tests/test_batch_contacts_cpu.py shows
on the CPU that they bite."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
from batch_harness import apply_to_batch, load_all, make_batch, upload_each  # noqa: E402
import batch_grid_cases as gc  # noqa: E402
import batch_contacts_cases as cs  # noqa: E402
import batch_contacts_ref as cr  # noqa: E402
from test_gpu_batch_bodies import assert_scenes_equal  # noqa: E402

pytestmark = pytest.mark.gpu

OFF, ALLPAIRS, GRID = 0, 1, 2
NAMES = ("touch", "pairs", "counts")
SENTINEL = -7
N_CASES = 21
_expected = {}


def expected(oracle, case):
    """The case on one oracle per scene, computed once and shared; never changed."""
    if case["name"] not in _expected:
        _expected[case["name"]] = cs.expected_contacts(oracle, case)
    return _expected[case["name"]]


def contacts_np(be, max_pairs, labels=True, other_body=False):
    """(touch, pairs, counts) of the batch as numpy arrays, in the reference's order."""
    out = be.contacts(labels=labels, pairs=max_pairs, other_body=other_body)
    touch, counts = out[0].cpu().numpy(), out[1].cpu().numpy()
    pairs = out[2].cpu().numpy() if len(out) == 3 else np.zeros((be.n_scenes, 0, 2), np.int32)
    return touch, pairs, counts


def assert_contacts(got, exp, what):
    for name, g, e in zip(NAMES, got, exp):
        assert g.dtype == np.int32 and g.shape == e.shape, (what, name, g.dtype, g.shape, e.shape)
        if not np.array_equal(g, e):
            at = tuple(int(x[0]) for x in np.nonzero(g != e))
            raise AssertionError("%s: %s differ in %d words, first at %s: got %d, expected %d" % (what, name, int((g != e).sum()), at, g[at], e[at]))


def reference_now(be, case, max_pairs=None, other_body=False, labels=True):
    """The reference on what load_scene returns now, with bodies()' labels."""
    lab = be.bodies()[0].cpu().numpy() if labels else None
    radius, bounds = cs.geometry(case)
    m = case["max_pairs"] if max_pairs is None else max_pairs
    return cr.contacts_of(load_all(be, case["bufs"]), be.max_particles, radius, bounds, lab, m, other_body)


@pytest.mark.parametrize("which", range(N_CASES))
def test_contacts_before_and_after_every_op(sb, oracle, which):
    cases = cs.all_cases(sb)
    assert len(cases) == N_CASES
    case = cases[which]
    exp = expected(oracle, case) if case.get("finite", True) else None
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    for k in range(-1, len(case["program"])):
        if k >= 0:
            apply_to_batch(be, case["program"][k])
        what = "%s after op %d" % (case["name"], k)
        got = contacts_np(be, case["max_pairs"])
        assert int(got[2][:, 0].max()) <= case["max_pairs"], what
        assert_contacts(got, reference_now(be, case), what + " against load_scene")
        if exp is not None:
            assert_contacts(got, exp[k][:3], what + " against the oracles")
    be.destroy()


def test_truncation_on_the_pile(sb):
    case = cs.case_pile(sb)
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    be.frame(1)
    full = contacts_np(be, case["max_pairs"])
    count = int(full[2][0, 0])
    assert count > max(cs.TRUNCATIONS) + 1
    assert_contacts(full, reference_now(be, case), "the pile after a frame")
    for m in cs.TRUNCATIONS + (count - 1, count, count + 3):
        got = contacts_np(be, m)
        assert got[1].shape == (1, m, 2)
        assert np.array_equal(got[1][0, :min(m, count)], full[1][0, :min(m, count)]) and (got[1][0, count:] == -1).all(), m
        assert np.array_equal(got[0], full[0]) and np.array_equal(got[2], full[2]) and got[2][0, 0] == count, m
        assert_contacts(got, reference_now(be, case, max_pairs=m), "the pile, max_pairs %d" % m)
    for pairs in (None, 0):
        two = be.contacts(labels=True, pairs=pairs)
        assert len(two) == 2 and np.array_equal(two[0].cpu().numpy(), full[0]) and np.array_equal(two[1].cpu().numpy(), full[2])
    be.destroy()


def test_other_body_lists_the_cross_body_pairs_in_order(sb):
    import torch
    case = cs.case_two_bodies(sb)
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    every = contacts_np(be, 64)
    cross = contacts_np(be, 64, other_body=True)
    labels = be.bodies()[0].cpu().numpy()
    assert every[2].tolist() == [[22, 3, 0, 15], [0, 0, 0, 0]]
    want = [p for p in every[1][0, :22].tolist() if labels[0, p[0]] != labels[0, p[1]]]
    assert len(want) == 3 and cross[1][0, :3].tolist() == want and (cross[1][0, 3:] == -1).all() and (cross[1][1] == -1).all()
    assert np.array_equal(cross[0], every[0]) and np.array_equal(cross[2], every[2])
    assert_contacts(cross, reference_now(be, case, max_pairs=64, other_body=True), "other_body")
    short = contacts_np(be, 2, other_body=True)
    assert short[1][0].tolist() == want[:2] and short[2][0].tolist() == [22, 3, 0, 15]
    # labels of the caller's own: arbitrary values are only compared
    own = torch.full((2, be.max_particles), -123456789, dtype=torch.int32, device="cuda")
    own[0, ::2] = 2 ** 31 - 1
    got = be.contacts(labels=own, pairs=64, other_body=True)
    exp = cr.contacts_of(load_all(be, case["bufs"]), be.max_particles, labels=own.cpu().numpy(), max_pairs=64, other_body=True)
    assert_contacts((got[0].cpu().numpy(), got[2].cpu().numpy(), got[1].cpu().numpy()), exp, "the caller's labels")
    assert 0 < exp[2][0, 1] < 22
    # without labels
    bare = contacts_np(be, 64, labels=None)
    assert (bare[0][..., 1] == -1).all() and (bare[2][:, 1] == -1).all() and np.array_equal(bare[1], every[1])
    assert np.array_equal(bare[0][..., [0, 2, 3]], every[0][..., [0, 2, 3]]) and np.array_equal(bare[2][:, [0, 2, 3]], every[2][:, [0, 2, 3]])
    assert_contacts(bare, reference_now(be, case, labels=False), "no labels")
    with pytest.raises(sb.EngineError) as ei:
        be.contacts(pairs=4, other_body=True)
    assert ei.value.status == 1 and "labels" in str(ei.value)
    be.destroy()


def test_contacts_only_read(sb):
    """frame, contacts, frame equals frame, frame -- bit for bit through load_scene; likewise mid-frame with break flags pending."""
    import batch_bodies_cases as bo
    case = bo.case_break(sb)
    a, b = make_batch(sb, case), make_batch(sb, case)
    for be in (a, b):
        upload_each(be, case["bufs"])
        be.frame(1)
    a.contacts(labels=True, pairs=256)
    a.frame(1)
    b.frame(1)
    assert_scenes_equal(a, b, case["bufs"], "frame, contacts, frame")
    a.step(5)
    b.step(5)
    pending = a.summary()[:, sb.batch.SUMMARY_FIELDS.index("pending_breaks")].cpu().numpy()
    assert (pending > 0).any()
    a.contacts(pairs=256)
    a.contacts(labels=True, pairs=3, other_body=True)
    a.step(59)
    a.delete_pass()
    b.step(59)
    b.delete_pass()
    assert_scenes_equal(a, b, case["bufs"], "step, contacts, step, delete")
    assert a.info("frames_done") == b.info("frames_done") and a.info("substeps_done") == b.info("substeps_done")
    a.destroy()
    b.destroy()


@pytest.mark.parametrize("which", ["pile", "edges", "mixed", "two_bodies", "geometry"])
def test_every_collision_mode_gives_the_same_contacts(sb, which):
    case = cs.case_geometry(sb, 1000.0, 600.0) if which == "geometry" else getattr(cs, "case_" + which)(sb)
    outs = []
    for mode, gmp in ((OFF, None), (ALLPAIRS, None), (GRID, None), (GRID, 1), (GRID, gc.NEVER)):
        be = make_batch(sb, case, mode=mode, grid_min_particles=gmp)
        upload_each(be, case["bufs"])
        outs.append(contacts_np(be, case["max_pairs"]))
        if len(outs) == 1:
            assert_contacts(outs[0], reference_now(be, case), case["name"] + " with collisions off")
        assert be.info("contacts_cells_per_side") == gc.cell_geometry(cs.geometry(case)[1], cs.geometry(case)[0], case["cap"][0])[0]
        be.destroy()
    for o in outs[1:]:
        assert_contacts(o, outs[0], case["name"] + " in another mode")


def test_every_combination_of_outputs_writes_exactly_its_own(sb):
    """Through the C call: a NULL output is not written, a non-NULL one whole, and nothing behind its n_scenes rows."""
    import torch
    case = cs.case_two_bodies(sb)
    n, maxP, M = len(case["bufs"]), case["cap"][0], 30
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    labels = be.bodies()[0]
    exp = reference_now(be, case, max_pairs=M)
    L = sb.batch.load_library()
    shapes = ((n + 1, maxP, 4), (n + 1, M, 2), (n + 1, 4))
    for mask in range(1, 8):
        outs = [torch.full(s, SENTINEL, dtype=torch.int32, device="cuda") for s in shapes]
        torch.cuda.synchronize()
        ptrs = [ctypes.c_void_p(o.data_ptr()) if mask >> k & 1 else None for k, o in enumerate(outs)]
        st = L.sb_batch_contacts_device(be._h, 0, ctypes.c_void_p(labels.data_ptr()), ptrs[0], ptrs[1], M, ptrs[2])
        assert st == 0, L.sb_batch_last_error(be._h)
        be.sync()
        for k, o in enumerate(outs):
            a = o.cpu().numpy()
            if mask >> k & 1:
                assert np.array_equal(a[:n], exp[k]) and (a[n:] == SENTINEL).all(), (mask, NAMES[k])
            else:
                assert (a == SENTINEL).all(), (mask, NAMES[k])
    # a touch buffer that is only 4-byte aligned
    raw = torch.full((n * maxP * 4 + 4,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert L.sb_batch_contacts_device(be._h, 0, ctypes.c_void_p(labels.data_ptr()), ctypes.c_void_p(raw.data_ptr() + 4), None, 0, None) == 0
    be.sync()
    a = raw.cpu().numpy()
    assert a[0] == SENTINEL and a[-3:].tolist() == [SENTINEL] * 3 and np.array_equal(a[1:1 + n * maxP * 4].reshape(n, maxP, 4), exp[0])
    # the Python call: tensors larger than needed and of another shape are written at their head, and come back as views
    flat = [torch.full((int(np.prod(s)) + 3,), SENTINEL, dtype=torch.int32, device="cuda") for s in ((n, maxP, 4), (n, M, 2), (n, 4))]
    touch, counts, pairs = be.contacts(labels=labels, touch=flat[0], pairs=flat[1][:n * M * 2].view(n, M, 2), counts=flat[2])
    assert (touch.data_ptr(), pairs.data_ptr(), counts.data_ptr()) == tuple(f.data_ptr() for f in flat)
    assert tuple(touch.shape) == (n, maxP, 4) and tuple(pairs.shape) == (n, M, 2) and tuple(counts.shape) == (n, 4)
    for k, (f, view) in enumerate(zip(flat, (touch, pairs, counts))):
        assert np.array_equal(view.cpu().numpy(), exp[k]) and bool((f[view.numel():] == SENTINEL).all()), NAMES[k]
    be.destroy()


def test_a_batch_far_larger_than_its_scene(sb):
    """Two particles at capacity 1024 / 4096 beside a scene never uploaded: the defined rows beyond the particles, in tensors
    filled with a sentinel."""
    import torch
    case = cs.case_two_in_1024(sb)
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    for labels in (True, None):
        touch = torch.full((2, 1024, 4), SENTINEL, dtype=torch.int32, device="cuda")
        counts = torch.full((2, 4), SENTINEL, dtype=torch.int32, device="cuda")
        pairs = torch.full((2, 4, 2), SENTINEL, dtype=torch.int32, device="cuda")
        be.contacts(labels=labels, touch=touch, counts=counts, pairs=pairs)
        got = (touch.cpu().numpy(), pairs.cpu().numpy(), counts.cpu().numpy())
        assert not any((g == SENTINEL).any() for g in got)
        assert_contacts(got, reference_now(be, case, labels=bool(labels)), "two in 1024")
        none = 0 if labels else -1
        assert (got[0][0, 2:] == [0, none, 0, -1]).all() and (got[0][1] == [0, none, 0, -1]).all() and got[2].tolist() == [[0, none, 0, 0]] * 2
    buf = case["bufs"][0].copy()
    buf.particles[1, 0] = buf.particles[0, 0] + np.float32(19.0)          # now they touch
    be.write_scene(buf, 0, 1)
    got = contacts_np(be, 4)
    assert got[2].tolist() == [[1, 0, 0, 2], [0, 0, 0, 0]] and got[1][0].tolist() == [[0, 1], [-1, -1], [-1, -1], [-1, -1]]
    assert got[0][0, :2].tolist() == [[1, 0, 0, 1], [1, 0, 0, 0]]
    be.destroy()


def test_argument_errors(sb):
    import torch
    case = cs.case_never_empty_one(sb)
    n, maxP = len(case["bufs"]), case["cap"][0]
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    L = sb.batch.load_library()
    vp = ctypes.c_void_p
    buf = torch.zeros(n * maxP * 4 + 8, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    for args, needle in (((None, 0, None, vp(p), None, 0, None), "null batch"),
                         ((be._h, 2, None, vp(p), None, 0, None), "unknown flags"),
                         ((be._h, 0x80000000, vp(p), vp(p), None, 0, None), "unknown flags"),
                         ((be._h, 1, None, vp(p), None, 0, None), "labels"),
                         ((be._h, 0, None, None, None, 0, None), "all null"),
                         ((be._h, 0, vp(p), None, None, 4, None), "all null"),
                         ((be._h, 0, None, None, vp(p), 0, None), "max_pairs 0"),
                         ((be._h, 0, vp(p + 2), vp(p), None, 0, None), "4-byte aligned"),
                         ((be._h, 0, None, vp(p + 1), None, 0, None), "4-byte aligned"),
                         ((be._h, 0, None, None, vp(p + 3), 4, None), "4-byte aligned"),
                         ((be._h, 0, None, None, None, 0, vp(p + 2)), "4-byte aligned")):
        assert L.sb_batch_contacts_device(*args) == 1, needle
        msg = L.sb_batch_last_error(args[0]).decode()
        assert "sb_batch_contacts_device" in msg and needle in msg, (needle, msg)
    i32 = dict(dtype=torch.int32, device="cuda")
    for call in (lambda: be.contacts(touch=torch.zeros((n, maxP, 4), dtype=torch.int64, device="cuda")),      # dtype
                 lambda: be.contacts(counts=torch.zeros((n, 4), dtype=torch.float32, device="cuda")),
                 lambda: be.contacts(labels=torch.zeros((n, maxP), dtype=torch.float32, device="cuda")),
                 lambda: be.contacts(touch=torch.zeros((n, maxP, 4), dtype=torch.int32)),                   # device
                 lambda: be.contacts(pairs=torch.zeros((n, 4, 2), dtype=torch.int32)),
                 lambda: be.contacts(touch=torch.zeros((n, maxP, 3), **i32)),                               # size
                 lambda: be.contacts(counts=torch.zeros((n, 3), **i32)),
                 lambda: be.contacts(labels=torch.zeros((n, maxP - 1), **i32)),
                 lambda: be.contacts(touch=torch.zeros((n, maxP, 8), **i32)[:, :, ::2]),                    # contiguity
                 lambda: be.contacts(pairs=torch.zeros((n, 4, 4), **i32)[:, :, ::2]),
                 lambda: be.contacts(touch="no"), lambda: be.contacts(pairs=1.5), lambda: be.contacts(labels="yes")):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: be.contacts(touch=p + 2), lambda: be.contacts(counts=p + 1), lambda: be.contacts(labels=p + 3)):
        with pytest.raises(sb.EngineError) as ei:
            call()
        assert ei.value.status == 1
    touch, counts = be.contacts()          # and the batch is as usable as before
    assert counts.cpu().numpy().tolist() == [[0, -1, 0, 0], [0, -1, 0, 0], [0, -1, 1, 0], [0, -1, 0, 0]]
    be.sync()
    be.destroy()


def test_info_keys(sb):
    for cap, bounds, radius, g in (((1024, 4096), 1000.0, 10.0, 49), ((1024, 64), 1000.0, 600.0, 1), ((256, 512), 1000.0, 0.5, 25), ((8, 8), 1000.0, 10.0, 4)):
        for mode in (OFF, GRID):
            be = sb.BatchEngine(n_scenes=2, bounds_size=bounds, particle_radius=radius, max_particles=cap[0], max_beams=cap[1], layout=2,
                                collision_mode=mode)
            assert be.info("contact_words") == 4 and be.info("contacts_kernel_scratch_bytes") == 0 and 0 < be.info("contacts_kernel_vgprs") <= 128
            assert be.info("contacts_cells_per_side") == g == gc.cell_geometry(bounds, radius, cap[0])[0]
            # sbk_lds_bytes: pos (2 words), label, cell, sorted, above per particle; G^2 + 1 cell words; 4 sums and 4 wave totals
            assert be.info("contacts_lds_bytes") == (6 * cap[0] + g * g + 1 + 8) * 4 <= 36 * 1024
            be.destroy()
