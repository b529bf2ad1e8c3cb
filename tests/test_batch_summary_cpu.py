"""sb_batch_summary_device / sb_batch_rollout_device without a GPU: declared, exported, bound with prototypes, argument errors before
a device is looked for; tests/batch_summary_ref.py against values worked out by hand; and the oracle side of every program of
tests/test_gpu_batch_summary.py: free of warnings, and biting where the GPU test relies on it (pending flags, removed beams,
non-finite state)."""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_cases as bc  # noqa: E402
import batch_summary_cases as sc  # noqa: E402
import batch_summary_ref as sr  # noqa: E402
import summary_cases as ec  # noqa: E402

F = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "softbody-webgpu_amd", "csrc")


def test_header_declares_and_library_exports_both_calls(sb):
    names = sb.engine.declared_symbols()
    L = sb.batch.load_library()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    for s in ("sb_batch_summary_device", "sb_batch_rollout_device"):
        assert s in names, s
        assert hasattr(L, s), s
        assert getattr(L, s).restype is ctypes.c_int, s
    assert L.sb_batch_summary_device.argtypes == [vp, vp]
    assert L.sb_batch_rollout_device.argtypes == [vp, u32, vp, vp]
    assert L.sb_abi_version() == 1   # additions only
    header = open(sb.engine.HEADER_PATH).read()
    for needle in ("#define SB_BATCH_SUMMARY_WORDS 24u", "summary_words", "summary_kernel_vgprs", "summary_kernel_scratch_bytes"):
        assert needle in header, needle
    assert callable(sb.BatchEngine.summary) and callable(sb.BatchEngine.rollout)


def test_argument_errors_are_invalid_before_anything_touches_a_device(sb):
    L = sb.batch.load_library()
    word = (ctypes.c_uint32 * 32)()
    p = ctypes.cast(word, ctypes.c_void_p)
    assert L.sb_batch_summary_device(None, None) == 1 and L.sb_batch_summary_device(None, p) == 1
    assert L.sb_batch_rollout_device(None, 1, None, None) == 1 and L.sb_batch_rollout_device(None, 0, p, p) == 1


def test_summary_fields_name_the_24_words(sb):
    f = sb.batch.SUMMARY_FIELDS
    assert sb.batch.SUMMARY_WORDS == sr.WORDS == 24 == len(f) == len(set(f))
    assert isinstance(f, tuple) and all(isinstance(x, str) and x for x in f)
    assert (f.index("particles"), f.index("pending_breaks"), f.index("kinetic_energy"), f.index("mean_strain"), f.index("uploaded")) == (0, 3, 14, 19, 20)


def test_python_refuses_what_is_not_a_buffer(sb):
    be = sb.BatchEngine.__new__(sb.BatchEngine)
    be._h, be.device, be.n_scenes, be.max_particles, be.max_beams, be._ext_stream = None, 0, 2, 16, 16, None
    import torch
    for call in (lambda: be.summary("no"), lambda: be.summary(torch.zeros((2, 24))), lambda: be.rollout(None),
                 lambda: be.rollout("no", frames=1), lambda: be.rollout(torch.zeros((1, 2, 8))), lambda: be.rollout(frames=-1),
                 lambda: be.rollout(frames=1, out=torch.zeros((1, 2, 24))), lambda: be.rollout(frames=1, summary=False, out=5)):
        with pytest.raises(ValueError):
            call()


def hand_scene(sb):
    """3 particles and 2 beams in capacity 4 / 4 (W = 4 / 4), the particles at data indices 0, 1, 2 -- with x = X, 1, -X where
    X = 2^60: the tree adds leaf 0 to leaf 2 first."""
    buf = sb.Buffers(2, 4, 4)
    X = F(2.0 ** 60)
    pts = np.array([[X, 2.0, 3.0, 4.0, 0.0, 0.0], [1.0, 6.0, -1.0, 2.0, 0.0, 0.0], [-X, -2.0, 0.5, 0.0, 0.0, 0.0]], "f4")
    bb = np.zeros(2, sb.layout.BEAM_DTYPE[2])
    bb[0] = (0, 1, 10, 10, 10, 1, 1, 1, 1, 0.25, -1.0)
    bb[1] = (1, 2, 10, 10, 10, 1, 1, 1, 1, 0.5, 2.0)
    buf.set_scene(pts, bb)
    return buf, X


def test_summary_ref_on_a_scene_worked_out_by_hand(sb):
    buf, X = hand_scene(sb)
    row = sr.summary_ref(buf, buf, 1)
    third = lambda v: F(np.float64(v) / np.float64(3))  # noqa: E731
    # x: (X + -X) + (1 + 0) = 1 -- serially (X + 1) + -X would be 0;  y: (2 + -2) + (6 + 0);  vx: (3 + .5) + -1;  vy: (4 + 0) + 2
    # energy: (12.5 + 0.125) + (2.5 + 0) = 15.125;  max v^2 = 25
    exp = [3, 2, 0, 1, 0, 0, third(1), third(6), third(2.5), third(6), -X, -2, X, 6, 15.125, 25, 0.5, 2, -1, 0.375, 1, 0, 0, 0]
    assert row.dtype == np.float32 and row.shape == (24,)
    assert row.tobytes() == np.array(exp, "f4").tobytes(), (row, exp)
    # a particle that is not finite leaves every statistic; a beam with a non-finite stress likewise; a removed beam is counted
    now = buf.copy()
    now.particles[0, 5] = np.inf
    now.beams[1]["stress"] = np.nan
    row = sr.summary_ref(now, buf, 0)
    exp = [3, 2, 0, 0, 1, 1, (1 - X) / 2, 2, -0.25, 1, -X, -2, 1, 6, 2.625, 5, 0.25, -1, -1, 0.25, 1, 0, 0, 0]
    assert row.tobytes() == np.array(exp, "f4").tobytes(), (row, exp)
    now = buf.copy()
    now.mapping[4] = 1   # the beam slots after a delete pass that removed beam 0
    now.beam_count = 1
    row = sr.summary_ref(now, buf, 0)
    assert list(row[:6]) == [3, 1, 1, 0, 0, 0] and list(row[16:20]) == [0.5, 2, 2, 0.5]
    # nothing finite: NaN (the quiet NaN's bits), counts and the energy 0
    now = buf.copy()
    now.particles[:3, 0] = np.nan
    now.beams["strain"][:2] = np.inf
    row = sr.summary_ref(now, buf, 0)
    assert list(row[:6]) == [3, 2, 0, 0, 3, 2] and row[14] == 0 and row[20] == 1
    nan_words = [6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17, 18, 19]
    assert (row[nan_words].view("u4") == 0x7FC00000).all()
    assert sr.never_uploaded_row()[nan_words].view("u4").tolist() == [0x7FC00000] * 13 and sr.never_uploaded_row()[20] == 0
    # beyond float32: +inf, once, at the end
    now = buf.copy()
    now.particles[1, 2] = F(3e38)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        row = sr.summary_ref(now, buf, 0)
    assert row[14] == np.inf and row[15] == np.inf and np.isfinite(row[8])


def dump_scene(buf, path, removed, pending):
    """the input of tests/summary_math_check.cpp: the finite-or-not records of a scene at their data indices"""
    P, B, maxP = buf.particle_count, buf.beam_count, buf.max_particles
    pidx, bidx = buf.mapping[:P].astype(np.int64), buf.mapping[maxP:maxP + B].astype(np.int64)
    with open(path, "wb") as f:
        np.array([maxP, buf.max_beams, P, B, removed, pending], "<u4").tofile(f)
        rec = np.zeros((P, 7), "<u4")
        rec[:, 0], rec[:, 1:] = pidx, np.ascontiguousarray(buf.particles[pidx], "<f4").view("<u4")
        rec.tofile(f)
        rec = np.zeros((B, 3), "<u4")
        rec[:, 0] = bidx
        rec[:, 1], rec[:, 2] = (np.ascontiguousarray(buf.beams[k][bidx], "<f4").view("<u4") for k in ("strain", "stress"))
        rec.tofile(f)


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_the_header_builds_the_references_row_on_the_host(sb, tmp_path, san):
    """csrc/sb_summary_math.h -- the leaves, the tree over all W leaves, the row former the four kernels call -- compiled for the
    host under sanitizers (tests/summary_math_check.cpp) gives summary_ref's 24 words bit for bit: on the tree-order witnesses, on
    the two scenes of zeros of both signs (min -0.0, max +0.0 in both), and on the hand-made scene with beams, also where a
    particle and a beam are not finite."""
    exe = os.path.join("hostcheck_build", "summary_math_check_" + san)
    p = subprocess.run(["make", "-C", CSRC, exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    hand, _ = hand_scene(sb)
    bad = hand.copy()
    bad.particles[0, 5] = np.inf
    bad.beams[1]["stress"] = np.nan
    scenes = [(c["name"], c["buf"], 0) for c in ec.witness_cases(sb) + ec.zero_sign_scenes(sb)] + [("hand", hand, 1), ("hand, not finite", bad, 0)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")
    for name, buf, pending in scenes:
        path = str(tmp_path / "scene.bin")
        dump_scene(buf, path, 0, pending)
        r = subprocess.run([os.path.join(CSRC, exe), path], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr, (name, r.stdout, r.stderr[-2000:])
        got = np.array([int(w, 16) for w in r.stdout.split()], "<u4").view("f4")
        sr.assert_rows_equal(got, sr.summary_ref(buf, buf, pending), name)
    for c in ec.zero_sign_scenes(sb):
        bits = sr.summary_ref(c["buf"], c["buf"], 0).view(np.uint32)
        assert bits[10] == bits[11] == 0x80000000 and bits[12] == bits[13] == 0, c["name"]


def test_tree_sum_is_the_stride_halving_tree():
    x = np.array([2.0 ** 60, 1.0, -2.0 ** 60, 1.0, 3.0, 0.0, 0.0, 0.0])
    assert sr.tree_sum(x) == ((x[0] + x[4]) + (x[2] + x[6])) + ((x[1] + x[5]) + (x[3] + x[7])) == 2.0 ** 60 - 2.0 ** 60 + 2.0
    assert sr.tree_sum(x[:4]) == 2.0 and sum(x[:4].tolist()) == 1.0
    assert [sr.pow2_at_least(n) for n in (0, 1, 8, 120, 128, 300, 1024, 4096)] == [1, 1, 8, 128, 128, 512, 1024, 4096]


@pytest.fixture(scope="module")
def expected(sb, oracle):
    """Every case's rows on the oracle, computed once, under `warnings as errors`."""
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for case in sc.all_cases(sb):
            out[case["name"]] = (case, sc.expected_rows(oracle, case)[0])
    return out


def test_every_program_runs_the_reference_without_warnings_and_gives_whole_rows(expected):
    assert len(expected) == 6
    for name, (case, rows) in expected.items():
        assert sorted(rows) == sorted(case["compare_after"]), name
        for r in rows.values():
            assert r.shape == (len(case["bufs"]), 24) and r.dtype == np.float32, name
            assert (r[:, 21:] == 0).all() and np.isfinite(r[:, :6]).all(), name


def test_the_cases_bite(sb, expected):
    case, rows = expected["heterogeneous"]
    a, b, c = (rows[k] for k in case["compare_after"])
    assert case["cap"] == (1024, 4096) and a[2, 0] == 1024                                 # the full-width trees
    assert a[4, 20] == 1 and a[4, 0] == 0 and np.isnan(a[4, 6]) and a[4, 14] == 0          # empty
    assert a[5].tobytes() == sr.never_uploaded_row().tobytes()                             # never uploaded
    assert (c[:, 3] > 0).any(), "break flags must be pending after the grab"
    assert not np.array_equal(a[:4], b[:4]) and not np.array_equal(b[:4], c[:4])
    case, rows = expected["yield / break / delete"]
    a, b = (rows[k] for k in case["compare_after"])
    assert (a[:, 2] > 0).any() and (a[:, 2] == 0).any() and (a[:, 3] == 0).all()           # removed beams in some scenes, flags cleared
    assert (b[:, 3] > 0).any() and (b[:, 2] > 0).any()                                     # mid-frame: flags pending
    assert (a[:, 1] + a[:, 2] == [x.beam_count for x in case["bufs"]]).all()
    case, rows = expected["permuted mapping + coincident particles"]
    buf = case["bufs"][0]
    assert not np.array_equal(buf.mapping[:buf.particle_count], np.arange(buf.particle_count))  # data index != slot
    case, rows = expected["default scene at 120 / 300"]
    assert case["cap"] == (120, 300) and sr.pow2_at_least(120) == 128 and sr.pow2_at_least(300) == 512
    case, rows = expected["force saturation"]
    r = rows[case["compare_after"][0]]
    assert case["cap"] == (8, 8)
    assert r[sc.NONFINITE_SCENE, 4] > 0 and r[sc.NONFINITE_SCENE, 5] > 0, "the non-finite path must be exercised"
    assert 0 < r[sc.NONFINITE_SCENE, 4] < r[sc.NONFINITE_SCENE, 0] and 0 < r[sc.NONFINITE_SCENE, 5] < r[sc.NONFINITE_SCENE, 1]
    assert np.isfinite(r[sc.NONFINITE_SCENE, 6:20]).all()                                  # and is left out of every statistic
    assert (r[:3, 4:6] == 0).all()                                                         # the saturation scene itself stays finite
    case, rows = expected["pile"]
    r = rows[case["compare_after"][0]]
    assert r[0, 0] == 256 and r[0, 1] == 0 and np.isnan(r[0, 16:20]).all() and case["cap"][1] == 0


def test_rollout_case_inputs_differ_per_scene_and_per_frame(sb):
    rows = [bc.user_inputs(sb, k) for k in range(3)]
    assert len({r for k in rows for r in k}) == 12
