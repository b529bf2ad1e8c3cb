"""BatchEngine.body_summary (sb_batch_body_summary_device) against tests/batch_body_summary_ref.py: on what
load_scene returns with bodies()' labels, and for the stepped cases on one oracle.OracleEngine per scene.  Counts, labels, sums and
means are compared by their bits, extremes by value, NaN words as NaN, ranks exactly.  Scenes, programs and label sets live in
tests/batch_body_summary_cases.py; tests/test_batch_body_summary_cpu.py pins their figures on the CPU."""
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
import batch_summary_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7


def call(be, rows, labels=None):
    """(rows, rank) of the batch as numpy arrays; labels: None (bodies()) or a numpy array [n, maxP] of the caller's."""
    import torch
    r, k = be.body_summary(None if labels is None else torch.from_numpy(labels).cuda(), rows=rows, rank=True)
    assert tuple(r.shape) == (be.n_scenes, rows, 24) and tuple(k.shape) == (be.n_scenes, be.max_particles)
    return r.cpu().numpy(), k.cpu().numpy()


def assert_info(be):
    maxP = be.max_particles
    W = 1 << (maxP - 1).bit_length()
    assert be.info("body_summary_words") == 24 and be.info("body_summary_kernel_scratch_bytes") == 0
    assert 0 < be.info("body_summary_kernel_vgprs") <= 128
    assert be.info("body_summary_lds_bytes") == W * 56 + maxP * 52 <= 160 * 1024


@pytest.fixture(scope="module")
def expected(sb, oracle):
    """Every stepped case on one oracle per scene, once: {name: (case, {op index: (bufs_now, labels, pending)})}."""
    return {c["name"]: (c, qc.expected(oracle, c)[0]) for c in qc.stepped_cases(sb)}


def run_case(sb, case, exp, row_counts, extra=None):
    """The program on the batch; after the ops of compare_after, for every row count, rows and ranks against the reference on the
    oracles' state and on what load_scene returns (the pending flags, which load_scene does not show, are the oracle's)."""
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    got = {}
    for k, op in enumerate(case["program"]):
        apply_to_batch(be, op)
        if k not in case["compare_after"]:
            continue
        now, labels, pending = exp[k]
        mine = load_all(be, case["bufs"])
        assert np.array_equal(be.bodies()[0].cpu().numpy(), labels)
        for m in row_counts:
            got[k, m] = call(be, m)
            what = "%s after op %d, %d rows" % (case["name"], k, m)
            qr.assert_equal(got[k, m], qr.body_summary_of(now, labels, m, pending), what + " against the oracles")
            qr.assert_equal(got[k, m], qr.body_summary_of(mine, labels, m, pending), what + " against load_scene")
        if extra:
            extra(be, k, exp[k])
    assert_info(be)
    return be, got


@pytest.mark.parametrize("which", [0, 1, 2])
def test_graphs_at_the_limit_and_at_the_smallest_capacities(sb, which):
    """1024 / 4096 in one batch: the shuffled path of 1024 (one group of all W leaves), 16 pieces of 64 (a tie the label
    resolves), 512 pairs, a star, 2 particles, an empty and a never-uploaded scene; 8 / 8 and 65 / 64: a path and two pairs."""
    case = qc.graph_cases(sb)[which]
    maxP = case["cap"][0]
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    labels = qr.body_labels_of(case["bufs"], maxP)
    mine = load_all(be, case["bufs"])
    for m in (1, min(16, maxP), maxP):
        got = call(be, m)
        qr.assert_equal(got, qr.body_summary_of(case["bufs"], labels, m), "%s, %d rows" % (case["name"], m))
        qr.assert_equal(got, qr.body_summary_of(mine, labels, m), "%s, %d rows, against load_scene" % (case["name"], m))
    rows, rank = got
    assert [int((r[:, 2] >= 0).sum()) for r in rows] == case["groups"]
    for i, b in enumerate(case["bufs"]):
        assert rows[i, :, 0].sum() == (0 if b is None else b.particle_count) == (rank[i] >= 0).sum(), i
    if which == 0:
        pieces = call(be, 16)[0][1]
        assert (pieces[:, 0] == 64).all() and (np.diff(pieces[:, 2]) > 0).all() and pieces[0, 2] == 0
        assert rows[0, 0, 0] == 1024 and rows[0, 1, 2] == -1 and (rank[5:] == -1).all()
    assert_info(be)
    be.destroy()


def test_default_scene_at_120_300_row_counts(sb, expected):
    """W = 128 above the capacity; max_rows = 1, one less than the 9 bodies (rank still names the cut body), and max_particles."""
    case, exp = expected["default scene at 120 / 300"]
    be, got = run_case(sb, case, exp, (1, 8, 120))
    rows, rank = got[0, 8]
    assert rows[0, :, 0].tolist() == [40, 36, 25, 4, 4, 4, 4, 1] and rank[0].max() == 8 and (rank[0] == 8).sum() == 1
    assert got[0, 1][0][0, 0].tobytes() == rows[0, 0].tobytes() and np.array_equal(got[0, 1][1], rank)
    full = got[0, 120][0]
    assert full[0, :, 0].sum() == 119 and full[0, 8, 0] == 1 and full[0, 9, 2] == -1
    be.destroy()


def test_breaking_lattices_callers_labels_and_the_one_body_identity(sb, expected):
    case, exp = expected["yield / break / delete"]
    n, maxP = len(case["bufs"]), case["cap"][0]
    L = qc.caller_labels(n, maxP)
    seen = []

    def extra(be, k, exp_k):
        now, labels, pending = exp_k
        # a scene that is ONE body: row 0 is summary()'s row, by bits
        s = be.summary().cpu().numpy()
        rows, rank = call(be, 2)
        for i in range(n):
            if rank[i].max() == 0:
                w = list(qr.SUMMARY_SHARED_WORDS)
                assert rows[i, 0, w].tobytes() == s[i, w].tobytes(), (k, i)
                seen.append((k, i))
        assert np.array_equal(call(be, maxP)[0][:, :, 0].sum(axis=1), s[:, 0])   # the rows' particles add up to the scene's
        if k != case["compare_after"][0]:
            return
        for name, lab in L.items():
            for m in (2, 4):
                qr.assert_equal(call(be, m, lab), qr.body_summary_of(now, lab, m, pending), "%s, %d rows" % (name, m))
        rows, rank = call(be, 4, L["stripes"])
        assert rows[0, :, 2].tolist() == [0, 1, 2, -1] and 0 < rows[0, :, 1].sum() < now[0].beam_count
        assert (call(be, 1, L["INT32_MIN"])[1] == -1).all()

    be, got = run_case(sb, case, exp, (4,), extra)
    a, b = (got[k, 4] for k in case["compare_after"])
    assert [int(r.max()) + 1 for r in a[1]] == [1, 6, 21, 38, 56, 1] and a[0][:, 0, 0].tolist() == [144, 139, 120, 101, 84, 144]
    assert a[0][:, :, 3].sum() == 0 and b[0][:, :, 3].sum() > 0
    assert sorted(seen) == [(0, 0), (0, 5), (1, 0), (1, 5)]
    be.destroy()


def test_heterogeneous_batch_pending_flags_before_and_after_the_delete_pass(sb, expected):
    case, exp = expected["heterogeneous"]
    assert case["cap"] == (1024, 4096)
    be, got = run_case(sb, case, exp, (4,))
    grabbed, deleted = (got[k, 4][0] for k in case["compare_after"])
    assert grabbed[qc.LATTICE, 0, [0, 2, 3]].tolist() == [144, 0, 129] and grabbed[2, 0, 3] == 220
    assert deleted[qc.LATTICE, :, 0].tolist() == [110, 19, 3, 3] and deleted[:, :, 3].sum() == 0
    assert deleted[4].tobytes() == deleted[5].tobytes() == np.stack([qr.empty_row()] * 4).tobytes()
    be.destroy()


def test_permuted_mapping(sb, expected):
    case, exp = expected["permuted mapping + coincident particles"]
    be, got = run_case(sb, case, exp, (8,))
    rows, rank = got[case["compare_after"][0], 8]
    assert (rank[0, :50] == -1).all() and rows[0, 0, 0] == 40 and rows[0, 0, 2] >= 50 and rows[1, :6, 0].tolist() == [2, 1, 1, 1, 1, 0]
    be.destroy()


def test_non_finite_particles(sb, expected):
    """A NaN coordinate and an infinite velocity in one group (word 4 = 2, the statistics leave them out); a group of only
    non-finite particles keeps its count and has NaN means."""
    case, exp = expected["force saturation"]
    k = case["compare_after"][0]
    now, labels, pending = exp[k]
    N = qc.nonfinite_labels(len(now))

    def extra(be, k, exp_k):
        for name, lab in N.items():
            qr.assert_equal(call(be, 2, lab), qr.body_summary_of(now, lab, 2, pending), name)

    be, got = run_case(sb, case, exp, (2, 8), extra)
    bad = call(be, 2, N["one group"])[0][sc.NONFINITE_SCENE]
    assert bad[0, :6].tolist() == [6, 3, 0, 0, 2, 1] and np.isfinite(bad[0, 6:20]).all()
    bad = call(be, 2, N["non-finite apart"])[0][sc.NONFINITE_SCENE]
    assert bad[:, 0].tolist() == [4, 2] and bad[1, 2] == 3 and bad[1, 4] == 2 and np.isnan(bad[1, 6:14]).all() and bad[1, 14] == 0
    be.destroy()


def assert_scenes_equal(a, b, bufs, what):
    for i, (x, y) in enumerate(zip(load_all(a, bufs), load_all(b, bufs))):
        if x is not None:
            bc.assert_same(x, y, "%s: scene %d" % (what, i))


def test_body_summary_only_reads(sb):
    """frame, body_summary, frame equals frame, frame -- bit for bit through load_scene; likewise mid-frame with flags pending."""
    case = qc.case_break(sb)
    a, b = make_batch(sb, case), make_batch(sb, case)
    for be in (a, b):
        upload_each(be, case["bufs"])
        be.frame(1)
    a.body_summary(rank=True)
    a.frame(1)
    b.frame(1)
    assert_scenes_equal(a, b, case["bufs"], "frame, body_summary, frame")
    a.step(5)
    b.step(5)
    a.body_summary(rows=3)
    a.step(59)
    a.delete_pass()
    b.step(59)
    b.delete_pass()
    assert_scenes_equal(a, b, case["bufs"], "step, body_summary, step, delete")
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
    exp = qr.body_summary_of(case["bufs"], labels.cpu().numpy(), m)
    L = sb.batch.load_library()
    for mask in (1, 2, 3):
        rows = torch.full((n + 1, m, 24), float(SENTINEL), dtype=torch.float32, device="cuda")
        rank = torch.full((n + 1, maxP), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ptrs = [ctypes.c_void_p(o.data_ptr()) if mask >> k & 1 else None for k, o in enumerate((rows, rank))]
        assert L.sb_batch_body_summary_device(be._h, ctypes.c_void_p(labels.data_ptr()), m, *ptrs) == 0, L.sb_batch_last_error(be._h)
        be.sync()
        r, k = rows.cpu().numpy(), rank.cpu().numpy()
        if mask & 1:
            qr.assert_rows_equal(r[:n], exp[0], "mask %d" % mask)
        if mask & 2:
            assert np.array_equal(k[:n], exp[1]), mask
        assert (r[n if mask & 1 else 0:] == SENTINEL).all() and (k[n if mask & 2 else 0:] == SENTINEL).all(), mask
    # the Python call: tensors larger than needed and of another shape are written at their head, and come back as views
    flat = [torch.full((n * m * 24 + 3,), float(SENTINEL), dtype=torch.float32, device="cuda"),
            torch.full((n * maxP + 3,), SENTINEL, dtype=torch.int32, device="cuda")]
    rows, rank = be.body_summary(labels, rows=m, out=flat[0], rank=flat[1])
    assert (rows.data_ptr(), rank.data_ptr()) == (flat[0].data_ptr(), flat[1].data_ptr())
    qr.assert_equal((rows.cpu().numpy(), rank.cpu().numpy()), exp, "views")
    assert bool((flat[0][n * m * 24:] == SENTINEL).all()) and bool((flat[1][n * maxP:] == SENTINEL).all())
    only = be.body_summary(rows=m)
    assert isinstance(only, torch.Tensor) and torch.equal(only.view(torch.int32), rows.view(torch.int32))
    be.destroy()


def test_body_summary_between_fork_reset_and_checkpoint_without_a_sync(sb):
    """body_summary() in front of fork(argsort(...)) and right behind fork / checkpoint / reset: the stream orders them."""
    import torch
    case = qc.case_break(sb)
    bufs, n = case["bufs"], len(case["bufs"])
    be = make_batch(sb, case)
    upload_each(be, bufs)
    be.frame(2)
    r0, k0 = be.body_summary(rows=4, rank=True)
    src = torch.argsort(r0[:, 0, 0], stable=True).to(torch.int32)      # the scene whose largest body is smallest first
    be.fork(src)
    r1, k1 = be.body_summary(rows=4, rank=True)
    idx = src.long()
    assert r0[:, 0, 0].tolist() == [144, 139, 120, 101, 84, 144] and idx.tolist() == [4, 3, 2, 1, 0, 5]   # (the first wait)
    assert torch.equal(r1.view(torch.int32), r0[idx].view(torch.int32)) and torch.equal(k1, k0[idx])
    mask = torch.tensor([1, 0, 0, 0, 0, 1], dtype=torch.uint8, device="cuda")
    be.checkpoint(mask)
    r2 = be.body_summary(rows=4)
    assert torch.equal(r2.view(torch.int32), r1.view(torch.int32))
    be.reset()                             # the others go back to the reset state of their fork's source: the whole lattice
    r3, k3 = be.body_summary(rows=4, rank=True)
    for i in range(n):
        if int(mask[i]):
            assert torch.equal(r3[i].view(torch.int32), r1[i].view(torch.int32)) and torch.equal(k3[i], k1[i]), i
        else:
            assert r3[i, :, 0].tolist() == [144, 0, 0, 0] and r3[i, 0, 8] != 0, i
    forked = [bufs[int(k)] for k in idx]   # (load_scene needs Buffers of the capacity only)
    mine = load_all(be, forked)
    qr.assert_equal((r3.cpu().numpy(), k3.cpu().numpy()), qr.body_summary_of(mine, qr.body_labels_of(mine, be.max_particles), 4),
                    "fork, checkpoint, reset")
    be.destroy()


def test_error_paths(sb):
    import torch
    case = qc.case_small(sb, (8, 8))
    n = len(case["bufs"])
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
    good = torch.zeros((n, 8), **i32)
    for bad in (lambda: be.body_summary(torch.zeros((n, 8), dtype=torch.int64, device="cuda")),       # dtype
                lambda: be.body_summary(out=torch.zeros((n, 8, 24), **i32)),
                lambda: be.body_summary(rank=torch.zeros((n, 8), **f32)),
                lambda: be.body_summary(torch.zeros((n, 8), dtype=torch.int32)),                      # device
                lambda: be.body_summary(good, out=torch.zeros((n, 8, 24), dtype=torch.float32)),
                lambda: be.body_summary(torch.zeros((n, 7), **i32)),                                  # size
                lambda: be.body_summary(good, rows=8, out=torch.zeros((n, 7, 24), **f32)),
                lambda: be.body_summary(good, rank=torch.zeros((n, 7), **i32)),
                lambda: be.body_summary(torch.zeros((n, 16), **i32)[:, ::2]),                         # contiguity
                lambda: be.body_summary(good, rows=0), lambda: be.body_summary(good, rows=9), lambda: be.body_summary("no"),
                lambda: be.body_summary(good, rank=1.5)):
        with pytest.raises(ValueError):
            bad()
    buf = torch.zeros(n * 8 * 24 + 8, **f32)
    for bad in (lambda: be.body_summary(good.data_ptr() + 2), lambda: be.body_summary(good, out=buf.data_ptr() + 1),
                lambda: be.body_summary(good, rank=buf.data_ptr() + 3)):
        with pytest.raises(sb.EngineError) as ei:
            bad()
        assert ei.value.status == 1
    L = sb.batch.load_library()
    vp = ctypes.c_void_p
    lp, rp = vp(good.data_ptr()), vp(buf.data_ptr())
    assert L.sb_batch_body_summary_device(be._h, lp, 1, None, None) == 1 and "both null" in L.sb_batch_last_error(be._h).decode()
    assert L.sb_batch_body_summary_device(be._h, None, 1, rp, None) == 1 and "null labels" in L.sb_batch_last_error(be._h).decode()
    assert L.sb_batch_body_summary_device(be._h, lp, 0, rp, None) == 1 and L.sb_batch_body_summary_device(be._h, lp, 0, None, rp) == 1
    assert L.sb_batch_body_summary_device(be._h, lp, 9, rp, None) == 1 and "max_rows" in L.sb_batch_last_error(be._h).decode()
    assert L.sb_batch_body_summary_device(None, lp, 1, rp, None) == 1
    rows = be.body_summary(rows=8)         # and the batch is as usable as before
    assert [int((r[:, 2] >= 0).sum()) for r in rows.cpu().numpy()] == case["groups"]
    be.sync()
    be.destroy()
