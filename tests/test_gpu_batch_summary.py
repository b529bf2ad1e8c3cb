"""BatchEngine.summary / rollout (sb_batch_summary_device, sb_batch_rollout_device) against tests/batch_summary_ref.py
on one oracle.OracleEngine per scene.  Every word is compared by its bits, NaN words as NaN.
Scenes and programs live in tests/batch_summary_cases.py; tests/test_batch_summary_cpu.py shows on the CPU that they bite."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
from batch_harness import apply_to_batch, device_bytes, load_all, make_batch, upload_each  # noqa: E402
import batch_summary_cases as sc  # noqa: E402
import batch_summary_ref as sr  # noqa: E402
import summary_cases as ec  # noqa: E402

pytestmark = pytest.mark.gpu


def assert_scenes_equal(a, b, bufs, what):
    for i, (x, y) in enumerate(zip(load_all(a, bufs), load_all(b, bufs))):
        if x is not None:
            bc.assert_same(x, y, "%s: scene %d" % (what, i))


def run_case(sb, oracle, case):
    """The program on the batch; after the ops of compare_after the batch's rows against the oracles' -- and against the
    reference applied to what load_scene returns, where the pending flags (which load_scene does not show) are the oracle's."""
    import torch
    exp, refs = sc.expected_rows(oracle, case)
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    out = torch.full((len(case["bufs"]), 24), -7.0, dtype=torch.float32, device="cuda")
    got = {}
    for k, op in enumerate(case["program"]):
        apply_to_batch(be, op)
        if k in case["compare_after"]:
            r = be.summary(out)
            assert r.data_ptr() == out.data_ptr()
            got[k] = r.cpu().numpy().copy()
            sr.assert_rows_equal(got[k], exp[k], "%s after op %d" % (case["name"], k))
    mine = np.stack([sr.never_uploaded_row() if s is None else sr.summary_ref(s, b, int(exp[max(exp)][i, 3]))
                     for i, (s, b) in enumerate(zip(load_all(be, case["bufs"]), case["bufs"]))])
    sr.assert_rows_equal(got[max(got)], mine, case["name"] + " against load_scene")
    assert be.info("summary_words") == 24 and be.info("summary_kernel_scratch_bytes") == 0 and 0 < be.info("summary_kernel_vgprs") <= 128
    return be, got, exp


def test_heterogeneous_batch_full_width_trees_nan_rule_and_pending_flags(sb, oracle):
    case = sc.case_hetero(sb)
    be, got, exp = run_case(sb, oracle, case)
    a, b, c = (got[k] for k in case["compare_after"])
    assert a[5].tobytes() == sr.never_uploaded_row().tobytes() and a[4, 20] == 1 and np.isnan(a[4, 6:14]).all()
    assert (c[:, 3] > 0).any() and (exp[case["compare_after"][2]][:, 3] > 0).any()
    be.destroy()


def test_removed_beams_compacted_mapping_and_pending_flags(sb, oracle):
    case = sc.case_break(sb)
    be, got, exp = run_case(sb, oracle, case)
    a, b = (got[k] for k in case["compare_after"])
    assert (a[:, 2] > 0).any() and (a[:, 2] == 0).any() and (b[:, 3] > 0).any()
    be.destroy()


@pytest.mark.parametrize("which", ["mapping", "default_120_300", "saturation", "pile"])
def test_summary_against_the_oracle(sb, oracle, which):
    """Data index != slot; W above the capacity; the smallest W and non-finite state; a scene on the contact cells, mid-frame."""
    case = getattr(sc, "case_" + which)(sb)
    be, got, exp = run_case(sb, oracle, case)
    r = got[max(got)]
    if which == "saturation":
        assert r[sc.NONFINITE_SCENE, 4] > 0 and r[sc.NONFINITE_SCENE, 5] > 0 and np.isfinite(r[sc.NONFINITE_SCENE, 6:20]).all()
    if which == "pile":
        assert be.info("cell_substeps") > 0
    be.destroy()


def test_a_zero_extreme_does_not_depend_on_which_leaves_share_a_thread(sb):
    """Capacity 1024 / 0: data indices 0 and 256 are leaves of thread 0.  Zeros of both signs in x, y, vx, vy, in either order:
    the minimum is -0.0 and the maximum +0.0 (the keys' order), as where the two meet in different threads."""
    scenes = ec.zero_sign_scenes(sb)
    bufs = [c["buf"] for c in scenes]
    be = make_batch(sb, dict(layout=2, cap=(1024, 0), mode=0, bufs=bufs))
    upload_each(be, bufs)
    rows = be.summary().cpu().numpy()
    be.destroy()
    print("rows", rows.view(np.uint32).tolist())
    for i, c in enumerate(scenes):
        bits = rows[i].view(np.uint32)
        assert bits[10] == 0x80000000 and bits[12] == 0, (c["name"], hex(bits[10]), hex(bits[12]))   # min_x, max_x
        assert bits[11] == 0x80000000 and bits[13] == 0, (c["name"], hex(bits[11]), hex(bits[13]))   # min_y, max_y
        sr.assert_rows_equal(rows[i], sr.summary_ref(c["buf"], c["buf"], 0), c["name"])


def test_summary_only_reads(sb):
    """frame, summary, frame equals frame, frame; a fork / reset right behind a summary behaves as without it."""
    import torch
    case = sc.case_break(sb)
    n = len(case["bufs"])
    a, b = make_batch(sb, case), make_batch(sb, case)
    for be in (a, b):
        upload_each(be, case["bufs"])
        be.frame(1)
    rows = a.summary()
    a.frame(1)
    b.frame(1)
    assert_scenes_equal(a, b, case["bufs"], "frame, summary, frame")
    a.step(5)          # flags pending
    b.step(5)
    a.summary(rows)
    a.step(59)
    a.delete_pass()
    b.step(59)
    b.delete_pass()
    assert_scenes_equal(a, b, case["bufs"], "step, summary, step")
    src = torch.tensor([4, 4, 2, 0, 4, 5], dtype=torch.int32, device="cuda")
    mask = torch.tensor([0, 1, 0, 0, 0, 1], dtype=torch.uint8, device="cuda")
    a.step(3)
    b.step(3)
    a.summary(rows)
    a.fork(src)
    b.fork(src)
    a.summary(rows)
    a.reset(mask)
    b.reset(mask)
    a.frame(1)
    b.frame(1)
    assert_scenes_equal(a, b, case["bufs"], "summary, fork, summary, reset")
    assert a.info("frames_done") == b.info("frames_done") and a.info("substeps_done") == b.info("substeps_done")
    a.destroy()
    b.destroy()


def test_rollout_equals_the_individual_calls_and_the_oracles(sb, oracle):
    import torch
    case = bc.case_inputs(sb)
    bufs, T, n = case["bufs"], 3, 4
    ins = [bc.user_inputs(sb, k) for k in range(T)]
    dev = torch.stack([device_bytes(r) for r in ins])          # uint8 [3, 4, 32]
    a, b = make_batch(sb, case), make_batch(sb, case)
    upload_each(a, bufs)
    upload_each(b, bufs)
    ra = a.rollout(dev.view(torch.float32))                    # float32 [3, 4, 8]
    assert tuple(ra.shape) == (T, n, 24) and ra.dtype == torch.float32
    rb = torch.empty_like(ra)
    refs = [bc.make_oracle(oracle, case, x) for x in bufs]
    exp = []
    for t in range(T):
        b.write_user_input(dev[t])
        b.frame()
        b.summary(rb[t])
        bc.apply_to_oracles(refs, ("inputs", ins[t]))
        bc.apply_to_oracles(refs, ("frame", 1))
        exp.append(sr.rows_of(refs, bufs))
    assert_scenes_equal(a, b, bufs, "rollout against the calls")
    assert torch.equal(ra.view(torch.int32), rb.view(torch.int32))
    sr.assert_rows_equal(ra.cpu().numpy(), np.stack(exp), "rollout against the oracles")
    for i, ref in enumerate(refs):
        bc.assert_same(a.load_scene(i, bufs[i].copy()), ref.load_buffers(bufs[i].copy()), "rollout, scene %d" % i)
    assert a.info("frames_done") == b.info("frames_done") == T and a.info("substeps_done") == b.info("substeps_done")
    assert not torch.equal(ra[0, 0], ra[0, 2]) and not torch.equal(ra[0], ra[2])
    # inputs=None: the last slice stays in force; summary=False; frames=0
    r2 = a.rollout(frames=2)
    b.frame()
    s1 = b.summary()
    b.frame()
    s2 = b.summary()
    assert tuple(r2.shape) == (2, n, 24) and torch.equal(r2.view(torch.int32), torch.stack([s1, s2]).view(torch.int32))
    assert a.rollout(dev[:1], summary=False) is None
    b.write_user_input(dev[0])
    b.frame()
    r0 = a.rollout(frames=0)
    assert tuple(r0.shape) == (0, n, 24) and a.rollout(dev[:0]).shape[0] == 0 and a.rollout(frames=0, summary=False) is None
    assert_scenes_equal(a, b, bufs, "rollouts without inputs / summaries / frames")
    assert a.info("frames_done") == b.info("frames_done") == T + 3
    out = torch.full((T * n * 24 + 5,), -7.0, dtype=torch.float32, device="cuda")
    r3 = a.rollout(dev, out=out)
    assert tuple(r3.shape) == (T, n, 24) and r3.data_ptr() == out.data_ptr() and bool((out[T * n * 24:] == -7.0).all())
    a.destroy()
    b.destroy()


def test_rollout_argmin_fork_summary_without_a_sync(sb):
    """rollout -> torch.argmin over a summary column -> fork of the best scene over all -> summary: every row is the best's."""
    import torch
    case = bc.case_inputs(sb)
    n = 4
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    dev = torch.stack([device_bytes(bc.user_inputs(sb, k)) for k in range(2)])
    rows = be.rollout(dev)
    col = sb.batch.SUMMARY_FIELDS.index("mean_y")
    best = torch.argmin(rows[-1, :, col])
    be.fork(best.to(torch.int32).repeat(n))
    after = be.summary()
    k = int(best)               # (the first wait)
    got, before = after.cpu().numpy(), rows[-1].cpu().numpy()
    assert len({before[i].tobytes() for i in range(n)}) == n, "the scenes must differ"
    for i in range(n):
        assert got[i].tobytes() == before[k].tobytes(), (i, k)
    be.destroy()


def test_error_paths(sb):
    import torch
    case = bc.case_inputs(sb)
    n = 4
    be = make_batch(sb, case)
    upload_each(be, case["bufs"])
    good_in = torch.zeros((2, n, 8), dtype=torch.float32, device="cuda")
    for call in (lambda: be.summary(torch.zeros((n, 24), dtype=torch.float64, device="cuda")),            # dtype
                 lambda: be.summary(torch.zeros((n, 24), dtype=torch.float32)),                           # device
                 lambda: be.summary(torch.zeros((n, 23), dtype=torch.float32, device="cuda")),            # size
                 lambda: be.summary(torch.zeros((n, 48), dtype=torch.float32, device="cuda")[:, ::2]),    # contiguity
                 lambda: be.rollout(torch.zeros((2, n, 8), dtype=torch.float32)),                         # device
                 lambda: be.rollout(good_in, frames=3),                                                   # size
                 lambda: be.rollout(torch.zeros((2, n, 16), dtype=torch.float32, device="cuda")[:, :, ::2]),
                 lambda: be.rollout(good_in, out=torch.zeros((2, n, 24), dtype=torch.float16, device="cuda")),
                 lambda: be.rollout(good_in, out=torch.zeros((1, n, 24), dtype=torch.float32, device="cuda")),
                 lambda: be.rollout(None)):
        with pytest.raises(ValueError):
            call()
    buf = torch.zeros(2 * n * 24 + 8, dtype=torch.float32, device="cuda")
    for call in (lambda: be.summary(buf.data_ptr() + 2), lambda: be.rollout(good_in.data_ptr() + 1, frames=1, out=buf.data_ptr()),
                 lambda: be.rollout(good_in.data_ptr(), frames=1, out=buf.data_ptr() + 2)):
        with pytest.raises(sb.EngineError) as ei:
            call()
        assert ei.value.status == 1
    L = sb.batch.load_library()
    assert L.sb_batch_summary_device(be._h, None) == 1 and "null" in L.sb_batch_last_error(be._h).decode()
    assert be.info("frames_done") == 0
    be.sync()
    be.destroy()
