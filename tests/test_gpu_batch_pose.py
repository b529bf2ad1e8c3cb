"""BatchEngine.pose (sb_batch_pose_device) against tests/batch_pose_ref.py: on what load_scene returns, and for the
stepped cases on one oracle.OracleEngine per scene.  Every word of the rows and of the moments is compared by its bits (NaN words as
NaN), ranks exactly; the one tolerance is the geometric property's.  The reference that `ref=None` stands for is rebuilt on the host
from what load_scene returned when the reset state was made.  Scenes, programs and references live in tests/batch_pose_cases.py
and tests/batch_body_summary_cases.py; tests/test_batch_pose_cpu.py pins their figures on the CPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
from batch_harness import apply_to_batch, load_all, make_batch, upload_each  # noqa: E402
import batch_body_summary_cases as qc  # noqa: E402
import batch_body_summary_ref as qr  # noqa: E402
import batch_pose_cases as pc  # noqa: E402
import batch_pose_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7


def call(be, rows, labels=None, ref=None):
    """(rows, moments, rank) of the batch as numpy arrays; labels: None (bodies()) or numpy [n, maxP]; ref: None (the reset
    state) or a list of numpy [maxP, 2] per scene."""
    import torch
    p = be.pose(None if labels is None else torch.from_numpy(labels).cuda(), None if ref is None else torch.from_numpy(np.stack(ref)).cuda(),
                rows=rows, moments=True, rank=True)
    assert tuple(p.rows.shape) == (be.n_scenes, rows, 24) and tuple(p.moments.shape) == (be.n_scenes, rows, 8)
    assert tuple(p.rank.shape) == (be.n_scenes, be.max_particles) and p.moments.dtype == torch.float64
    return p.rows.cpu().numpy(), p.moments.cpu().numpy(), p.rank.cpu().numpy()


def refs_of(bufs):
    """The references `ref=None` stands for when `bufs` (one Buffers per scene, None: never uploaded) is the reset state."""
    maxP = next(b.max_particles for b in bufs if b is not None)
    return [np.full((maxP, 2), np.nan, np.float32) if b is None else pr.reference_of(b) for b in bufs]


def assert_info(be):
    maxP = be.max_particles
    W = 1 << (maxP - 1).bit_length()
    assert be.info("pose_words") == 24 and be.info("pose_moment_words") == 8 and be.info("pose_kernel_scratch_bytes") == 0
    assert 0 < be.info("pose_kernel_vgprs") <= 128
    assert be.info("pose_lds_bytes") == W * 96 + maxP * 12 <= 160 * 1024


def assert_matches_body_summary(be, got, rows):
    """Row k names body_summary's row k; where no member is unmatched, centroid and mean velocity are its words 6 .. 9 by bits."""
    b, brank = be.body_summary(rows=rows, rank=True)
    b, brank = b.cpu().numpy(), brank.cpu().numpy()
    assert np.array_equal(got[2], brank) and np.array_equal(got[0][:, :, 1], b[:, :, 2]) and np.array_equal(got[0][:, :, 0], b[:, :, 0])
    whole = (got[0][:, :, 1] >= 0) & (got[0][:, :, 3] == b[:, :, 4])   # (every finite member is matched)
    assert whole.any()
    assert got[0][whole][:, [4, 5, 8, 9]].tobytes() == b[whole][:, 6:10].tobytes()


@pytest.fixture(scope="module")
def expected(sb, oracle):
    """Every stepped case on one oracle per scene, once: {name: (case, {op index: (bufs_now, labels, pending)})}."""
    return {c["name"]: (c, qc.expected(oracle, c)[0]) for c in pc.stepped_cases(sb)}


def run_case(sb, case, exp, row_counts, extra=None):
    """The program on the batch; after the ops of compare_after, for every row count, rows, moments and ranks with ref=None (the
    upload is the reset state) against the restatement on the oracles' state and on what load_scene returns."""
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    refs = refs_of(case["bufs"])
    got = {}
    for k, op in enumerate(case["program"]):
        apply_to_batch(be, op)
        if k not in case["compare_after"]:
            continue
        now, labels, pending = exp[k]
        mine = load_all(be, case["bufs"])
        for m in row_counts:
            got[k, m] = call(be, m)
            what = "%s after op %d, %d rows" % (case["name"], k, m)
            pr.assert_equal(got[k, m], pr.pose_of(now, labels, m, refs), what + " against the oracles")
            pr.assert_equal(got[k, m], pr.pose_of(mine, labels, m, refs), what + " against load_scene")
        if extra:
            extra(be, k, exp[k], refs)
    assert_info(be)
    return be, got


@pytest.mark.parametrize("which", [0, 1, 2])
def test_graphs_at_the_limit_and_at_the_smallest_capacities(sb, which):
    """1024 / 4096 in one batch: the shuffled path of 1024 (one group of all W leaves), 16 pieces of 64, 512 pairs, a star, 2
    particles, an empty and a never-uploaded scene; 8 / 8 (W = 8) and 65 / 64 (W = 128 with leaves never used): a path and two
    pairs.  Against the reset state (the upload itself: b == +0.0 and a == I == I0 by bits) and against a caller's reference with
    NaN rows; max_rows of 1, 16 and max_particles."""
    case = qc.graph_cases(sb)[which]
    maxP = case["cap"][0]
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    labels = qr.body_labels_of(case["bufs"], maxP)
    mine = load_all(be, case["bufs"])
    own, callers = refs_of(case["bufs"]), pc.caller_refs(case["bufs"], maxP)
    for m in (1, min(16, maxP), maxP):
        got = call(be, m)
        pr.assert_equal(got, pr.pose_of(case["bufs"], labels, m, own), "%s, %d rows" % (case["name"], m))
        pr.assert_equal(got, pr.pose_of(mine, labels, m, own), "%s, %d rows, against load_scene" % (case["name"], m))
        pr.assert_equal(call(be, m, ref=callers), pr.pose_of(case["bufs"], labels, m, callers), "%s, %d rows, the caller's reference" % (case["name"], m))
    rows, moms, rank = got
    assert_matches_body_summary(be, got, maxP)
    assert [int((r[:, 1] >= 0).sum()) for r in rows] == case["groups"]
    live = rows[:, :, 1] >= 0
    m = moms[live]
    assert (m[:, 1].view(np.uint64) == 0).all() and (m[:, 0].view(np.uint64) == m[:, 2].view(np.uint64)).all()
    assert (m[:, 2].view(np.uint64) == m[:, 3].view(np.uint64)).all() and (rows[live][:, 3] == 0).all()
    lost = call(be, maxP, ref=callers)[0]
    assert lost[:, :, 3].sum() > 0 and np.array_equal(lost[:, :, 0], rows[:, :, 0])
    if which == 0:
        assert rows[0, 0, 0] == 1024 and rows[0, 1, 1] == -1 and (rank[5:] == -1).all() and (rows[1, :16, 0] == 64).all()
    assert_info(be)
    be.destroy()


def test_default_scene_at_120_300_row_counts(sb, expected):
    """W = 128 above the capacity, two frames from the reset state; max_rows = 1, one less than the 9 bodies, and max_particles."""
    case, exp = expected["default scene at 120 / 300"]
    be, got = run_case(sb, case, exp, (1, 8, 120))
    rows, moms, rank = got[0, 8]
    assert rows[0, :, 0].tolist() == [40, 36, 25, 4, 4, 4, 4, 1] and rank[0].max() == 8 and (rank[0] == 8).sum() == 1
    assert got[0, 1][0][0, 0].tobytes() == rows[0, 0].tobytes() and np.array_equal(got[0, 1][2], rank)
    full = got[0, 120][0]
    assert full[0, :, 0].sum() == 119 and full[0, 8, 0] == 1 and full[0, 9, 1] == -1 and np.isnan(full[0, 8, 15])
    assert_matches_body_summary(be, got[0, 8], 8)
    be.destroy()


def test_breaking_lattices_mid_frame_callers_labels_and_references(sb, expected):
    case, exp = expected["yield / break / delete"]
    n, maxP = len(case["bufs"]), case["cap"][0]
    L = qc.caller_labels(n, maxP)
    callers = pc.caller_refs(case["bufs"], maxP)

    def extra(be, k, exp_k, refs):
        now, labels, pending = exp_k
        assert_matches_body_summary(be, call(be, 4), 4)
        if k != case["compare_after"][0]:
            return
        for name, lab in L.items():
            for m in (2, 4):
                pr.assert_equal(call(be, m, lab), pr.pose_of(now, lab, m, refs), "%s, %d rows" % (name, m))
        pr.assert_equal(call(be, 4, L["stripes"], callers), pr.pose_of(now, L["stripes"], 4, callers), "stripes against the caller's reference")
        rows, moms, rank = call(be, 4, L["stripes"])
        assert rows[0, :, 1].tolist() == [0, 1, 2, -1] and rows[0, :3, 0].sum() == 144
        assert (call(be, 1, L["INT32_MIN"])[2] == -1).all()

    be, got = run_case(sb, case, exp, (4,), extra)
    a, b = (got[k, 4] for k in case["compare_after"])
    assert [int(r.max()) + 1 for r in a[2]] == [1, 6, 21, 38, 56, 1] and a[0][:, 0, 0].tolist() == [144, 139, 120, 101, 84, 144]
    assert not np.array_equal(a[1], b[1])
    be.destroy()


def test_non_finite_particles(sb, expected):
    """A NaN coordinate and an infinite velocity in one group are members that are not matched; a group of only such has NaN
    words and NaN moments and keeps its count."""
    case, exp = expected["force saturation"]
    k = case["compare_after"][0]
    now, labels, pending = exp[k]
    N = qc.nonfinite_labels(len(now))

    def extra(be, k, exp_k, refs):
        for name, lab in N.items():
            pr.assert_equal(call(be, 2, lab), pr.pose_of(now, lab, 2, refs), name)

    be, got = run_case(sb, case, exp, (2, 8), extra)
    bad = call(be, 2, N["one group"])[0][pc.NONFINITE_SCENE]
    assert bad[0, :4].tolist() == [6, 0, 4, 2] and np.isfinite(bad[0]).all()
    rows, moms, rank = call(be, 2, N["non-finite apart"])
    bad = rows[pc.NONFINITE_SCENE]
    assert bad[:, :4].tolist() == [[4, 0, 4, 0], [2, 3, 0, 2]] and np.isnan(bad[1, 4:17]).all() and not bad[1, 17:].any()
    assert (moms[pc.NONFINITE_SCENE, 1, :5].view(np.uint64) == 0x7FF8000000000000).all() and not moms[pc.NONFINITE_SCENE, 1, 5:].any()
    be.destroy()


def test_a_spawned_particle_has_no_reference_until_a_checkpoint(sb):
    """ref=None: unmatched when spawned, matched after checkpoint(), a second spawn unmatched again and removed by reset()."""
    import torch
    case = qc.case_small(sb, (8, 8))
    bufs, n, maxP = case["bufs"], len(case["bufs"]), 8
    be = make_batch(sb, case)
    upload_each(be, bufs)
    PAIRS = 1   # (two pairs, 4 of 8 particles: room to spawn; the paths fill their capacity)

    def check(reset_bufs, what, unmatched):
        now = load_all(be, bufs)
        labels = qr.body_labels_of(now, maxP)
        got = call(be, maxP)
        pr.assert_equal(got, pr.pose_of(now, labels, maxP, refs_of(reset_bufs)), what)
        assert got[0][PAIRS, :, 3].sum() == unmatched, what
        return now

    def spawn(x):
        pos = torch.full((n, 1, 2), x, dtype=torch.float32, device="cuda")
        result, counts = be.add_particles(sb.batch.new_particle_rows(pos))
        assert result[PAIRS, 0].item() >= 0

    spawn(300.0)
    be.step(2)
    now1 = check(bufs, "spawned", 1)
    assert now1[PAIRS].particle_count == 5
    be.checkpoint()
    check(now1, "spawned, checkpoint", 0)
    spawn(600.0)
    be.step(2)
    now2 = check(now1, "second spawn", 1)
    assert now2[PAIRS].particle_count == 6
    be.reset()
    now3 = check(now1, "reset", 0)
    assert now3[PAIRS].particle_count == 5
    be.destroy()


def test_reset_and_fork(sb):
    """Right after reset() every body gives b == +0.0 and a == I == I0 by bits; after fork() the source's bits."""
    import torch
    case = qc.case_break(sb)
    bufs, n = case["bufs"], len(case["bufs"])
    be = make_batch(sb, case)
    upload_each(be, bufs)
    be.frame(1)
    p0 = be.pose(rows=4, moments=True, rank=True)
    src = torch.tensor([4, 3, 2, 1, 0, 5], dtype=torch.int32, device="cuda")
    be.fork(src)
    p1 = be.pose(rows=4, moments=True, rank=True)
    idx = src.long()
    assert torch.equal(p1.rows.view(torch.int32), p0.rows[idx].view(torch.int32)) and torch.equal(p1.rank, p0.rank[idx])
    assert torch.equal(p1.moments.view(torch.int64), p0.moments[idx].view(torch.int64))
    assert bool((p0.moments[:, 0, 1] != 0).any())            # (a frame in: the lattices have turned)
    be.reset()
    rows, moms, rank = call(be, 4)
    live = rows[:, :, 1] >= 0
    m = moms[live]
    assert live.sum() == n and (m[:, 1].view(np.uint64) == 0).all() and (m[:, 0].view(np.uint64) == m[:, 2].view(np.uint64)).all()
    assert (m[:, 2].view(np.uint64) == m[:, 3].view(np.uint64)).all() and (m[:, 5] == 144).all() and (rows[live][:, 16] == 1).all()
    be.destroy()


def assert_scenes_equal(a, b, bufs, what):
    for i, (x, y) in enumerate(zip(load_all(a, bufs), load_all(b, bufs))):
        if x is not None:
            bc.assert_same(x, y, "%s: scene %d" % (what, i))


def test_pose_only_reads(sb):
    """frame, pose, frame equals frame, frame -- bit for bit through load_scene; and a reset returns to the same bytes."""
    case = qc.case_break(sb)
    a, b = make_batch(sb, case), make_batch(sb, case)
    for be in (a, b):
        upload_each(be, case["bufs"])
        be.frame(1)
    a.pose(moments=True, rank=True)
    a.frame(1)
    b.frame(1)
    assert_scenes_equal(a, b, case["bufs"], "frame, pose, frame")
    a.pose(rows=3)
    a.reset()
    b.reset()
    assert_scenes_equal(a, b, case["bufs"], "pose, reset")
    assert a.info("frames_done") == b.info("frames_done") and a.info("substeps_done") == b.info("substeps_done")
    a.destroy()
    b.destroy()


def test_every_combination_of_outputs_writes_exactly_its_own(sb):
    """Through the C call: a NULL output is not written, a non-NULL one whole, and nothing behind its n_scenes rows."""
    import torch
    case = qc.case_small(sb, (65, 64))
    n, maxP, m = len(case["bufs"]), 65, 3
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    labels = be.bodies()[0]
    callers = pc.caller_refs(case["bufs"], maxP)
    ref = torch.from_numpy(np.stack(callers)).cuda()
    exp = pr.pose_of(case["bufs"], labels.cpu().numpy(), m, callers)
    L = sb.batch.load_library()
    vp = ctypes.c_void_p
    for mask in range(1, 8):
        rows = torch.full((n + 1, m, 24), float(SENTINEL), dtype=torch.float32, device="cuda")
        moms = torch.full((n + 1, m, 8), float(SENTINEL), dtype=torch.float64, device="cuda")
        rank = torch.full((n + 1, maxP), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ptrs = [vp(o.data_ptr()) if mask >> k & 1 else None for k, o in enumerate((rows, moms, rank))]
        assert L.sb_batch_pose_device(be._h, vp(labels.data_ptr()), vp(ref.data_ptr()), m, *ptrs) == 0, L.sb_batch_last_error(be._h)
        be.sync()
        got = [o.cpu().numpy() for o in (rows, moms, rank)]
        pr.assert_equal([g[:n] if mask >> k & 1 else None for k, g in enumerate(got)], exp, "mask %d" % mask)
        for k, g in enumerate(got):
            assert (g[n if mask >> k & 1 else 0:] == SENTINEL).all(), (mask, k)
    # the Python call: tensors larger than needed and of another shape are written at their head, and come back as views
    flat = [torch.full((n * m * 24 + 3,), float(SENTINEL), dtype=torch.float32, device="cuda"),
            torch.full((n * m * 8 + 3,), float(SENTINEL), dtype=torch.float64, device="cuda"),
            torch.full((n * maxP + 3,), SENTINEL, dtype=torch.int32, device="cuda")]
    p = be.pose(labels, ref, rows=m, out=flat[0], moments=flat[1], rank=flat[2])
    assert [x.data_ptr() for x in p] == [x.data_ptr() for x in flat]
    pr.assert_equal([x.cpu().numpy() for x in p], exp, "views")
    assert bool((flat[0][n * m * 24:] == SENTINEL).all()) and bool((flat[1][n * m * 8:] == SENTINEL).all()) and bool((flat[2][n * maxP:] == SENTINEL).all())
    only = be.pose(labels, ref, rows=m)
    assert isinstance(only, torch.Tensor) and torch.equal(only.view(torch.int32), p.rows.view(torch.int32))
    assert_info(be)
    be.destroy()


def test_info_at_the_limit_capacity(sb):
    be = sb.BatchEngine(n_scenes=1, max_particles=1024, max_beams=4096)
    assert be.info("pose_kernel_scratch_bytes") == 0 and be.info("pose_lds_bytes") == 110592 <= 160 * 1024
    be.destroy()


def test_the_turned_lattice_gives_its_angle_within_the_bounds(sb):
    """The one test with a tolerance: atan2(b, a) equals the angle the lattice was turned by within 2 (|delta| / r_rms + 2^-23),
    and pose_fit's rms is at most 2e-5 (tests/batch_pose_cases.py derives both; the CPU test shows the restatement inside them)."""
    import torch
    g = pc.turned_lattice(sb)
    be = sb.BatchEngine(n_scenes=1, layout=2, max_particles=g["cap"][0], max_beams=g["cap"][1])
    be.write_scene(g["buf"])
    ref = torch.from_numpy(g["ref"][None]).cuda()
    labels = torch.zeros((1, g["cap"][0]), dtype=torch.int32, device="cuda")
    p = be.pose(labels, ref, rows=1, moments=True)
    pr.assert_equal((p.rows.cpu().numpy(), p.moments.cpu().numpy(), None), pr.pose_of([g["buf"]], labels.cpu().numpy(), 1, [g["ref"]]), "turned lattice")
    row = p.rows[0, 0].cpu().numpy()
    theta = np.arctan2(np.float64(row[11]), np.float64(row[10]))
    fit = sb.batch.pose_fit(p.moments)
    print("theta error %.3e (bound %.3e), rms %.3e (bound %.1e)" % (abs(theta - pc.THETA), g["theta_bound"], fit.rms[0, 0].item(), pc.RMS_BOUND))
    assert abs(theta - pc.THETA) <= g["theta_bound"]
    assert fit.rms[0, 0].item() <= pc.RMS_BOUND and abs(fit.theta[0, 0].item() - pc.THETA) <= g["theta_bound"]
    assert fit.omega[0, 0].item() == 0.0 and row[2] == 64
    be.destroy()


def test_error_paths(sb):
    import torch
    case = qc.case_small(sb, (8, 8))
    n = len(case["bufs"])
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
    good = torch.zeros((n, 8), **i32)
    for bad in (lambda: be.pose(torch.zeros((n, 8), dtype=torch.int64, device="cuda")),                # dtype
                lambda: be.pose(good, moments=torch.zeros((n, 8, 8), **f32)),
                lambda: be.pose(good, ref=torch.zeros((n, 8, 2), dtype=torch.float64, device="cuda")),
                lambda: be.pose(good, ref=torch.zeros((n, 8, 2), dtype=torch.float32)),                 # device
                lambda: be.pose(good, ref=torch.zeros((n, 7, 2), **f32)),                               # size
                lambda: be.pose(good, rows=8, moments=torch.zeros((n, 7, 8), dtype=torch.float64, device="cuda")),
                lambda: be.pose(good, rows=0), lambda: be.pose(good, rows=9), lambda: be.pose(good, rank=1.5)):
        with pytest.raises(ValueError):
            bad()
    buf = torch.zeros(n * 8 * 24 + 8, dtype=torch.float64, device="cuda")
    for bad in (lambda: be.pose(good.data_ptr() + 2), lambda: be.pose(good, out=buf.data_ptr() + 1), lambda: be.pose(good, ref=buf.data_ptr() + 2),
                lambda: be.pose(good, moments=buf.data_ptr() + 4), lambda: be.pose(good, rank=buf.data_ptr() + 3)):
        with pytest.raises(sb.EngineError) as ei:
            bad()
        assert ei.value.status == 1 and "aligned" in str(ei.value)
    L = sb.batch.load_library()
    vp = ctypes.c_void_p
    lp, rp = vp(good.data_ptr()), vp(buf.data_ptr())
    assert L.sb_batch_pose_device(be._h, lp, None, 1, None, None, None) == 1 and "all null" in L.sb_batch_last_error(be._h).decode()
    assert L.sb_batch_pose_device(be._h, None, None, 1, rp, None, None) == 1 and "null labels" in L.sb_batch_last_error(be._h).decode()
    assert L.sb_batch_pose_device(be._h, lp, None, 0, rp, None, None) == 1 and L.sb_batch_pose_device(be._h, lp, None, 9, None, rp, None) == 1
    assert "max_rows" in L.sb_batch_last_error(be._h).decode() and L.sb_batch_pose_device(None, lp, None, 1, rp, None, None) == 1
    rows = be.pose(rows=8)                 # and the batch is as usable as before
    assert [int((r[:, 1] >= 0).sum()) for r in rows.cpu().numpy()] == case["groups"]
    be.sync()
    be.destroy()
